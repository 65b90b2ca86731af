"""The launch decision of the heads gathers over bfloat16 rows
(nts_gather_plan_heads_bf16), checked without a GPU.  The rule, as written in
include/nts_hip.h: elements per lane are the widest of 8 / 4 / 2 that divides
the columns per head as well as the width and whose 16- / 8- / 4-byte load
the common alignment of input and output permits, else 4 strided single
elements; the lane group is the smallest power of two in [16, 64] that covers
the width; the grid is (batch + edges / 256 + 1) * slabs * lanes threads in
workgroups of 256, at most 8192 of them.  One head is the scalar bf16
gather's native launch."""
import os

import pytest

from tests.conftest import REPO

SO = os.path.join(REPO, "neutronstarlite_amd", "libnts_hip.so")


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        import neutronstarlite_amd.build as b
        b.build()
    for name in ("NTS_GATHER_SCHED", "NTS_GATHER_WINDOW", "NTS_GATHER_BLOCKS",
                 "NTS_SPLIT", "NTS_MAX_BLOCKS"):
        assert name not in os.environ, f"{name} would change the plan"
    import neutronstarlite_amd.shim as shim
    return shim


def ceil_div(a, b):
    return -(-a // b)


def rule(f, width, batch, edges):
    """(lane_group, grid) of the header's rule for `width` elements per lane."""
    per_lane = width if width > 1 else 4
    need = ceil_div(f, per_lane)
    group = 64
    while group // 2 >= need and group > 16:
        group //= 2
    slabs = ceil_div(f, group * per_lane)
    items = batch + edges // 256 + 1
    return group, min(8192, ceil_div(items * slabs * group, 256))


@pytest.mark.parametrize("heads,c_per,alignment,width", [
    (8, 16, 256, 8),
    (4, 4, 256, 4),
    (4, 6, 256, 2),
    (3, 7, 256, 1),
    (16, 1, 256, 1),
    (8, 16, 8, 4),
    (8, 16, 4, 2),
    (8, 16, 2, 1),
])
def test_vector_width(shim, heads, c_per, alignment, width):
    f = heads * c_per
    for batch, edges in ((2000, 200_000), (7, 3)):
        p = shim.gather_plan_heads_bf16(f, heads, alignment, batch, edges)
        assert p["vector_width"] == width, p
        group, grid = rule(f, width, batch, edges)
        assert p["lane_group"] == group, p
        assert p["grid"] == grid, p


def test_two_slabs_at_eight_wide(shim):
    """f = 1024 at 8 elements per lane: 64 lanes cover 512 columns."""
    p = shim.gather_plan_heads_bf16(1024, 16, 16, 2000, 200_000)
    assert p == {"vector_width": 8, "lane_group": 64,
                 "grid": rule(1024, 8, 2000, 200_000)[1]}
    assert rule(1024, 8, 2000, 200_000)[1] == min(
        8192, ceil_div((2000 + 781 + 1) * 2 * 64, 256))


@pytest.mark.parametrize("f", [1, 33, 128, 130, 136, 602])
@pytest.mark.parametrize("alignment", [256, 16, 8, 4, 2])
def test_one_head_is_the_native_scalar_bf16_launch(shim, f, alignment):
    for batch, edges in ((2000, 200_000), (7, 3), (0, 0)):
        p = shim.gather_plan_heads_bf16(f, 1, alignment, batch, edges)
        q = shim.gather_plan_bf16(f, alignment, batch, batch, edges, 0, -1)
        assert not q["blocked"] and q["schedule"] == 0
        for key in ("lane_group", "vector_width", "grid"):
            assert p[key] == q[key], (key, p, q)


def test_nothing_to_launch_reports_zeros(shim):
    for batch, edges in ((0, 5), (5, 0)):
        p = shim.gather_plan_heads_bf16(128, 8, 16, batch, edges)
        assert p == {"lane_group": 0, "vector_width": 0, "grid": 0}


@pytest.mark.parametrize("f,heads", [(128, 0), (128, 3), (8, 16), (128, -1),
                                     (128, 2.0)])
def test_invalid_heads_raise_before_the_library_is_called(shim, f, heads):
    with pytest.raises(ValueError):
        shim.gather_plan_heads_bf16(f, heads, 16, 2000, 200_000)
