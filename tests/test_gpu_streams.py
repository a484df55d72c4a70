"""The tensor streams of the HIP back end — K10 (fill_rank, residual_sq), the generators, the layout and shard ops —
op by op, against numpy in long double with derived bars, the kernel each K10 call took checked against the route
log (ops.h): tests/stream_cases.py through tests/opshim. No torch in this process. On an MI355X (256 CUs) no case
skips; the multi-chunk cases of rank.mfma and rank.split skip, with a message, elsewhere."""
import pytest

import contraction_cases as CC
import opshim_util
import stream_cases as SC

pytestmark = pytest.mark.gpu
_seen = {}  # family -> the tags its cases logged (for the coverage test at the end of the module)


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("hip")
    yield s
    s.close()


@pytest.fixture(scope="module")
def ncu():
    return opshim_util.compute_units()


def _run_family(sh, ncu, family, log):
    failures, skipped, tags = [], [], []
    for c in [c for c in SC.CASES if c["family"] == family]:
        try:
            t = SC.run_case(sh, c, True, ncu=ncu, log=log)
            tags += t
            if t:
                log.append(f"{c['name']}: {t}")
        except CC.Skip as e:
            skipped.append(str(e))
        except (AssertionError, opshim_util.ShimError) as e:
            failures.append(str(e))
    return tags, failures, skipped


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_family(sh, ncu, family, capsys):
    log = []
    tags, failures, skipped = _run_family(sh, ncu, family, log)
    _seen[family] = tags
    with capsys.disabled():
        print("\n" + "\n".join(log))
        print(f"{family}: largest err/bar {SC.WORST.get(family, 0.0):.3g}")
    assert not failures, f"{len(failures)} cases failed:\n" + "\n".join(failures)
    assert ncu != 256 or not skipped, skipped  # on an MI355X no case may skip
    if skipped:
        pytest.skip(f"{len(skipped)} device-bound cases: " + skipped[0])


def test_every_route_was_taken(sh, ncu):
    """the instantiations the K10 cases logged against the full set the three launchers can log, enumerated in the
    case file from their formulas (a family that test_family has not run in this process is run here)"""
    for family in SC.FAMILIES:
        if family.startswith("rank_") and family not in _seen:
            _seen[family] = _run_family(sh, ncu, family, [])[0]
    got = sorted({SC.tag_family(t) for tags in _seen.values() for t in tags})
    if ncu != 256:
        assert set(got) <= set(SC.EXPECTED_TAGS), sorted(set(got) - set(SC.EXPECTED_TAGS))
        pytest.skip(f"the multi-chunk cases need 256 CUs, this device has {ncu}")
    assert got == SC.EXPECTED_TAGS, (sorted(set(SC.EXPECTED_TAGS) - set(got)), sorted(set(got) - set(SC.EXPECTED_TAGS)))
