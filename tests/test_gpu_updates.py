"""The mode-update, Normalize and factor-side kernels of the HIP back end, op by op, against numpy in long double
with derived componentwise bars, the route each call took checked against the route log (ops.h):
tests/update_cases.py through tests/opshim. No torch in this process; no case skips."""
import pytest

import opshim_util
import update_cases as UC

pytestmark = pytest.mark.gpu
_seen = {}  # family -> the tags its cases logged (for the coverage test at the end of the module)


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("hip")
    yield s
    s.close()


@pytest.mark.parametrize("family", UC.FAMILIES)
def test_family(sh, family, capsys):
    cases = [c for c in UC.CASES if c["family"] == family]
    failures, log = [], []
    tags = _seen.setdefault(family, [])
    for c in cases:
        try:
            t = UC.run_with_env("hip", c, True, log=log) if c.get("env") else UC.run_case(sh, c, True, log=log)
            tags += t
            log.append(f"{c['name']}: {t}")
        except (AssertionError, opshim_util.ShimError) as e:
            failures.append(str(e))
    with capsys.disabled():
        print("\n" + "\n".join(log))
        print(f"{family}: largest err/bar {UC.WORST.get(family, 0.0):.3g}")
        for line in sorted({ln.split("scales: ")[1].split(", ")[1] for ln in log if "scales: max |" in ln}):
            print(f"{family}: scale {line}")
        if family == "normalize" and UC.SCALE_DEV:
            print(f"normalize.grid: largest |f_dev / f_ref - 1| = {max(UC.SCALE_DEV):.3g} u")
    assert not failures, f"{len(failures)} of {len(cases)} cases failed:\n" + "\n".join(failures)


def test_every_route_was_taken(sh):
    """the tags of all cases, by family, against the set these launchers can log (a family that test_family has not
    run in this process, whatever the selection or order, is run here)"""
    for family in UC.FAMILIES:
        if family not in _seen:
            _seen[family] = [t for c in UC.CASES if c["family"] == family
                             for t in (UC.run_with_env("hip", c, True) if c.get("env") else UC.run_case(sh, c, True))]
    got = sorted({UC.tag_family(t) for tags in _seen.values() for t in tags})
    assert got == UC.EXPECTED_TAGS, (sorted(set(UC.EXPECTED_TAGS) - set(got)), sorted(set(got) - set(UC.EXPECTED_TAGS)))
