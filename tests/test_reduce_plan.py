"""The launch decision of the max / min gather (nts_reduce_plan), checked
without a GPU: the geometry is the scalar gather's native launch, and the
hub-merge scratch is absent while no vertex can be split and bounded by
8 bytes per output element otherwise."""
import os

import pytest

from tests.conftest import REPO

SO = os.path.join(REPO, "neutronstarlite_amd", "libnts_hip.so")
SPLIT = 256   # default max edges per work item (NTS_SPLIT)


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


@pytest.mark.parametrize("f", [1, 7, 33, 128, 130, 602])
@pytest.mark.parametrize("alignment", [16, 8, 4])
def test_geometry_is_the_native_gather_launch(shim, f, alignment):
    for batch, edges in ((2000, 200_000), (7, 3), (0, 0)):
        p = shim.reduce_plan(f, alignment, batch, edges)
        q = shim.gather_plan(f, alignment, batch, batch, edges, 0, -1)
        assert not q["blocked"] and q["schedule"] == 0
        for key in ("lane_group", "vector_width", "grid"):
            assert p[key] == q[key], (key, p, q)
        if edges <= SPLIT:
            assert p["scratch_bytes"] == 0, p
        else:
            assert 0 < p["scratch_bytes"] <= 8 * batch * f, p


@pytest.mark.parametrize("edges,needs", [(1, False), (SPLIT, False),
                                         (SPLIT + 1, True)])
def test_scratch_only_when_a_vertex_can_be_split(shim, edges, needs):
    p = shim.reduce_plan(33, 16, 10, edges)
    assert (p["scratch_bytes"] > 0) == needs, p
    assert p["scratch_bytes"] <= 8 * 10 * 33


def test_min_plans_like_max(shim):
    assert (shim.reduce_plan(130, 8, 2000, 200_000, "min")
            == shim.reduce_plan(130, 8, 2000, 200_000, "max"))


@pytest.mark.parametrize("bad", ["sum", "MAX", "", None, 0])
def test_bad_op_raises_before_the_library_is_called(shim, bad):
    with pytest.raises(ValueError):
        shim.reduce_plan(128, 16, 2000, 200_000, bad)
    with pytest.raises(ValueError):
        shim.reduce_op(bad)
    # the stream bindings check first too: no handle is ever touched
    s = shim.Stream.__new__(shim.Stream)
    with pytest.raises(ValueError):
        s.reduce_by_dst_from_src(bad, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 1, 1)
    with pytest.raises(ValueError):
        s.reduce_backward(bad, 0, 0, 0, 0, 0, 1, 1)
