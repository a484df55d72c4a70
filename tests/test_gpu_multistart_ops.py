"""The multi-start, constraint and diagnostic kernels of the HIP back end, op by op, against numpy in long double
with derived componentwise bars, the route each call took checked against the route log (ops.h):
tests/multistart_ops_cases.py through tests/opshim. No torch in this process; no case skips."""
import pytest

import multistart_ops_cases as MC
import opshim_util

pytestmark = pytest.mark.gpu
_seen = {}  # family -> the tags its cases logged (for the coverage test at the end of the module)


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("hip")
    yield s
    s.close()


@pytest.mark.parametrize("family", MC.FAMILIES)
def test_family(sh, family, capsys):
    cases = [c for c in MC.CASES if c["family"] == family]
    failures, log = [], []
    tags = _seen.setdefault(family, [])
    for c in cases:
        try:
            t = MC.run("hip", sh, c, True, log=log)
            tags += t
            log.append(f"{c['name']}: {t}")
        except (AssertionError, opshim_util.ShimError) as e:
            failures.append(str(e))
    with capsys.disabled():
        print("\n" + "\n".join(log))
        print(f"{family}: largest err/bar {MC.WORST.get(family, 0.0):.3g}")
    assert not failures, f"{len(failures)} of {len(cases)} cases failed:\n" + "\n".join(failures)


def test_every_route_was_taken(sh):
    """the tags of all cases, by family, against the set these launchers can log (a family that test_family has not
    run in this process, whatever the selection or order, is run here)"""
    for family in MC.FAMILIES:
        if family not in _seen:
            _seen[family] = [t for c in MC.CASES if c["family"] == family for t in MC.run("hip", sh, c, True)]
    got = sorted({MC.tag_family(t) for tags in _seen.values() for t in tags})
    assert got == MC.EXPECTED_TAGS, (sorted(set(MC.EXPECTED_TAGS) - set(got)), sorted(set(got) - set(MC.EXPECTED_TAGS)))
