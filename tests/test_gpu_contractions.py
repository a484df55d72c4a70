"""The contraction kernels of the HIP back end, op by op, against numpy in fp64 or wider, with the route each
call took checked against the route log (ops.h): tests/contraction_cases.py through tests/opshim. No torch in
this process. On an MI355X (256 CUs) no case skips; the device-bound cases skip, with a message, elsewhere."""
import numpy as np
import pytest

import contraction_cases as CC
import opshim_util

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


@pytest.mark.parametrize("family", CC.FAMILIES)
def test_family(sh, ncu, family, capsys):
    cases = [c for c in CC.CASES if c["family"] == family and not c.get("tail")]
    failures, skipped, log = [], [], []
    tags = _seen.setdefault(family, [])
    for c in cases:
        try:
            t = CC.run_checked(sh, c, hip=True, ncu=ncu, log=log)
            tags += t
            log.append(f"{c['name']}: {t}")
        except CC.Skip as e:
            skipped.append(str(e))
        except (AssertionError, opshim_util.ShimError) as e:
            failures.append(str(e))
    with capsys.disabled():
        print("\n" + "\n".join(log))
    assert not failures, f"{len(failures)} of {len(cases)} cases failed:\n" + "\n".join(failures)
    assert ncu != 256 or not skipped, skipped  # on an MI355X no case may skip
    if skipped:
        pytest.skip(f"{len(skipped)} device-bound cases: " + skipped[0])


def test_tail_mode(sh, ncu, capsys):
    """Tail mode (fp32, two n-tiles, a round and a bit of resident workgroups) at 1, 2 and 10 k-blocks, and: it keeps
    ordinary stores, the same kernel and the same result bits whatever store mode is asked for."""
    if ncu != 256:
        pytest.skip(f"tail-mode shapes are sized for 256 CUs, this device has {ncu}")
    tags, log = _seen.setdefault("tail", []), []
    for c in [c for c in CC.CASES if c.get("tail")]:
        tags += CC.run_checked(sh, c, hip=True, ncu=ncu, log=log)
    with capsys.disabled():
        print("\n" + "\n".join(log))
    (c,) = [c for c in CC.CASES if c["name"] == "scan:f32 tail J=17"]
    posts, routes = [], []
    for mode in (0, 1):
        routes.append(CC.run_case(sh, dict(c, store=mode), hip=True, posts=posts))
    assert routes[0] == routes[1] and len(routes[0]) == 1, routes
    assert np.array_equal(posts[0], posts[1])


def test_every_route_was_taken(ncu):
    """the tags of all cases above, by kernel family, against the set the launchers can log"""
    if not _seen:
        pytest.skip("runs after the cases of this module")
    got = sorted({CC.tag_family(t) for tags in _seen.values() for t in tags})
    if ncu != 256:
        assert set(got) <= set(CC.EXPECTED_TAGS), sorted(set(got) - set(CC.EXPECTED_TAGS))
        pytest.skip(f"device-bound routes need 256 CUs, this device has {ncu}")
    assert got == CC.EXPECTED_TAGS, (sorted(set(CC.EXPECTED_TAGS) - set(got)), sorted(set(got) - set(CC.EXPECTED_TAGS)))
