"""Ops::cp_mode_update_ortho_ragged of the HIP back end at the op level (tests/polar_shim: the op on host arrays,
with its route log): the three launches of kernels_polar.hip.h at rows {1, 63, 64, 65, 130} and ranks {1, 3, 17,
64}, guards around W and grad, leading dimensions wider than the rows, starts of different ranks in one call.
Reference and bars: tests/polar_cases.py."""
import re

import pytest

import polar_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim():
    lib = PC.load(hostsim=False)
    yield lib
    lib.polar_shim_close()


def test_rows_and_ranks_against_numpy(shim):
    tags = PC.case_table(shim)   # (the route of its call with four starts of ranks 2, 64, 5, 17 at 130 rows)
    assert tags == ["update_ortho R=64 starts=4 tiles=3"], tags


def test_route_tag_names_rank_starts_and_tiles(shim):
    tags = PC.run(shim, PC.inputs(10, [2, 17, 5]))[5]
    assert len(tags) == 1 and re.fullmatch(r"update_ortho R=17 starts=3 tiles=1", tags[0]), tags
