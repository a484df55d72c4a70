"""ppals_match_columns — the exact rectangular assignment behind the factor match score — through the real
libppals.so, which loads without a device (the call needs no context), and csrc/assignment.h on its own
under AddressSanitizer + UBSan as a stand-alone program (tests/assignment_check/main.cpp). The brute-force
reference is tests/fms_ref.py's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -3


@pytest.fixture(scope="module")
def pp():
    import ppals
    ppals.lib()
    return ppals


def test_the_optimum_is_not_the_greedy_matching(pp):
    perm, total = pp.match_columns([[0.9, 0.8], [0.8, 0.1]])
    assert list(perm) == [1, 0] and total == 0.8 + 0.8      # greedy: 0.9 + 0.1


@pytest.mark.parametrize("ra,rb", [(5, 5), (3, 5), (5, 3)])
def test_random_scores_against_brute_force(pp, ra, rb):
    rng = np.random.default_rng(100 * ra + rb)
    for rep in range(20):
        sc = rng.uniform(-1.0, 1.0, (ra, rb))
        _, want = R.brute_force(sc)
        perm, total = pp.match_columns(sc)
        hit = perm[perm >= 0]
        assert len(hit) == min(ra, rb) == len(set(hit)) and np.all(hit < rb)
        assert total == sum(sc[p, q] for p, q in enumerate(perm) if q >= 0)
        assert abs(total - want) <= 16 * np.finfo(float).eps, (total, want)
        # ld > ra: the rows behind ra are never read
        ld = ra + 3
        padded = np.full((ld, rb), np.nan, order="F")
        padded[:ra] = sc
        perm2, total2 = (C.c_int * ra)(), C.c_double(0)
        assert pp.lib().ppals_match_columns(pp._dp(padded), ra, rb, ld, perm2, C.byref(total2)) == 0
        assert list(perm2) == list(perm) and total2.value == total


@pytest.mark.parametrize("n", [64, 128])
def test_a_planted_permutation_is_recovered(pp, n):
    rng = np.random.default_rng(n)
    pi = rng.permutation(n)
    sc = rng.uniform(-0.05, 0.05, (n, n))
    sc[np.arange(n), pi] = rng.uniform(0.85, 1.0, n)
    perm, total = pp.match_columns(sc)
    assert np.array_equal(perm, pi)
    again, total2 = pp.match_columns(sc)
    assert np.array_equal(again, perm) and total2 == total   # deterministic


def test_refusals(pp):
    L = pp.lib()
    L.ppals_last_error.restype = C.c_char_p
    sc = np.asfortranarray(np.full((3, 5), 0.5))
    perm, total = (C.c_int * 3)(), C.c_double(0)
    calls = [(None, 3, 5, 3), (pp._dp(sc), 0, 5, 3), (pp._dp(sc), 3, 0, 3), (pp._dp(sc), 3, 5, 2)]
    for bad in (np.nan, np.inf, -np.inf):
        s2 = sc.copy(order="F")
        s2[1, 2] = bad
        calls.append((pp._dp(s2), 3, 5, 3))
        calls[-1] = calls[-1] + (s2,)   # (keeps the array alive)
    for c in calls:
        assert L.ppals_match_columns(c[0], c[1], c[2], c[3], perm, C.byref(total)) == ARG
        assert L.ppals_last_error().decode().startswith("ppals_match_columns: ")
    assert L.ppals_match_columns(pp._dp(sc), 3, 5, 3, None, None) == 0   # perm and sum may be NULL


def test_assignment_header_under_sanitizers(tmp_path):
    """a stand-alone program with its own main, run directly: nothing is preloaded, nothing loaded into python"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program where the toolchain has them as archives, so that the program
    # does not depend on the order in which shared libraries are loaded
    for flags in (base + ["-static-libasan", "-static-libubsan"], base):
        p = subprocess.run([cxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
        if p.returncode == 0:
            break
    else:
        pytest.skip("the host compiler lacks the sanitizer runtimes: " + p.stderr.strip().splitlines()[-1])
    exe = tmp_path / "assignment_check"
    subprocess.check_call([cxx] + flags + ["-I", os.path.join(ROOT, "pairwise-perturbation_amd", "csrc"), "-o",
                                           str(exe), os.path.join(ROOT, "tests", "assignment_check", "main.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases hold" in run.stdout
