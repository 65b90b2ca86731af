"""The launch decision of the heads gathers (nts_gather_plan_heads), checked
without a GPU: the lane width is the widest of 4 / 2 dwords that divides the
columns per head as well as the width and that the alignment permits, else
the 4-strided-dword path; one head is the scalar gather's native launch."""
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


@pytest.mark.parametrize("f,heads,alignment,width", [
    (128, 8, 16, 4),      # C = 16
    (128, 8, 8, 2),       # alignment permits dwordx2 only
    (128, 8, 4, 1),
    (24, 4, 16, 2),       # C = 6: f % 4 == 0 but C % 4 != 0
    (12, 4, 16, 1),       # C = 3
    (128, 128, 16, 1),    # C = 1, the tensor_weight form
    (512, 8, 16, 4),      # C = 64, two slabs
])
def test_vector_width(shim, f, heads, alignment, width):
    p = shim.gather_plan_heads(f, heads, alignment, 2000, 200_000)
    assert p["vector_width"] == width, p
    # lane group: the smallest power of two in [16, 64] covering a slab
    per_lane = width if width > 1 else 4
    need = ceil_div(f, per_lane)
    group = 64
    while group // 2 >= need and group > 16:
        group //= 2
    assert p["lane_group"] == group, p
    slabs = ceil_div(f, group * per_lane)
    items = 2000 + 200_000 // 256 + 1
    assert p["grid"] == min(8192, ceil_div(items * slabs * group, 256)), p


@pytest.mark.parametrize("f", [1, 33, 128, 130, 602])
@pytest.mark.parametrize("alignment", [16, 8, 4])
def test_one_head_is_the_native_scalar_launch(shim, f, alignment):
    for batch, edges in ((2000, 200_000), (7, 3), (0, 0)):
        p = shim.gather_plan_heads(f, 1, alignment, batch, edges)
        q = shim.gather_plan(f, alignment, batch, batch, edges, 0, -1)
        assert not q["blocked"] and q["schedule"] == 0
        for key in ("lane_group", "vector_width", "grid"):
            assert p[key] == q[key], (key, p, q)


@pytest.mark.parametrize("f,heads", [(128, 0), (128, 3), (8, 16), (128, -1),
                                     (128, 2.0)])
def test_invalid_heads_raise_before_the_library_is_called(shim, f, heads):
    with pytest.raises(ValueError):
        shim.gather_plan_heads(f, heads, 16, 2000, 200_000)
