"""The Tucker eigen side of the HIP back end — unfold_gram, top_eigvecs, top_eigvecs_warm with its lazy and deferred
hand-overs, orthonormalize — and the small factor-side ops next to them, op by op, against numpy in long double, the
route each call took checked against the route log (ops.h): tests/tucker_ops_cases.py through tests/opshim. No torch
in this process; no case skips."""
import pytest

import opshim_util
import tucker_ops_cases as TC

pytestmark = pytest.mark.gpu
_seen = {}  # family -> the tags its cases logged (for the coverage test at the end of the module)


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("hip")
    yield s
    s.close()


def _run(sh, c, log=None):
    return TC.run_with_env("hip", c, True, log=log) if c.get("env") else TC.run_case(sh, c, True, log=log)


@pytest.mark.parametrize("family", TC.FAMILIES)
def test_family(sh, family, capsys):
    cases = [c for c in TC.CASES if c["family"] == family]
    failures, log = [], []
    tags = _seen.setdefault(family, [])
    for c in cases:
        try:
            t = _run(sh, c, log)
            tags += t
            log.append(f"{c['name']}: {t}")
        except (AssertionError, opshim_util.ShimError) as e:
            failures.append(str(e))
    with capsys.disabled():
        print("\n" + "\n".join(log))
        print(f"{family}: largest err/bar {TC.WORST.get(family, 0.0):.3g}")
        for (fam, what), r in sorted(TC.RATIOS.items()):
            print(f"{family}: device / reference so far, {fam} {what}: {r:.3g}")
    assert not failures, f"{len(failures)} of {len(cases)} cases failed:\n" + "\n".join(failures)


def test_every_route_was_taken(sh):
    """the tags of all cases, by family, against the set these launchers can log (a family that test_family has not
    run in this process, whatever the selection or order, is run here)"""
    for family in TC.FAMILIES:
        if family not in _seen:
            _seen[family] = [t for c in TC.CASES if c["family"] == family for t in _run(sh, c)]
    got = sorted({TC.tag_family(t) for tags in _seen.values() for t in tags})
    assert got == TC.EXPECTED_TAGS, (sorted(set(TC.EXPECTED_TAGS) - set(got)), sorted(set(got) - set(TC.EXPECTED_TAGS)))
