"""The fused GATv2 inference forward in the C-ABI and the Python binding, and
its launch decision (no compute calls: runs without a GPU).  The split is
assumed to be the default of 256."""
import ctypes
import inspect
import os

import pytest

from tests.conftest import REPO

SO = os.path.join(REPO, "neutronstarlite_amd", "libnts_hip.so")
ENTRIES = ("nts_gatv2_forward_fused", "nts_gatv2_forward_fused_bf16")
BATCH, EDGES = 1000, 30000


def _shim():
    import neutronstarlite_amd.shim as shim
    if not os.path.exists(SO):
        import neutronstarlite_amd.build as b
        b.build()
    return shim


def _plan(k, c, align=16, elem=4, edges=EDGES, general=False):
    return _shim().gatv2_forward_fused_plan(k * c, k, elem, align, align,
                                            BATCH, edges, general)


def test_exported_declared_and_bound():
    shim = _shim()
    from neutronstarlite_amd import gat
    l, raw = shim.lib(), ctypes.CDLL(SO)
    hdr = open(os.path.join(REPO, "include", "nts_hip.h")).read()
    assert hasattr(raw, "nts_gatv2_forward_fused_plan")
    assert "void nts_gatv2_forward_fused_plan(" in hdr
    for n in ENTRIES:   # stream, 4 pointers, slope, 2 pointers, 5 counts
        assert hasattr(raw, n) and f"int {n}(" in hdr
        assert len(getattr(l, n).argtypes) == 13
        assert getattr(l, n).restype is ctypes.c_int32
    want = ["self", "x_l", "x_r", "y_ptr", "att", "slope", "row_indices",
            "column_offset", "src_start", "batch", "edges", "f", "heads"]
    got = list(inspect.signature(shim.Stream.gatv2_forward_fused).parameters)
    assert got == want
    got = list(
        inspect.signature(shim.Stream.gatv2_forward_fused_bf16).parameters)
    assert got == ["self", "x_l_bf16", "x_r_bf16"] + want[3:]
    got = list(inspect.signature(shim.gatv2_forward_fused_plan).parameters)
    assert got == ["f", "heads", "elem_bytes", "row_alignment",
                   "fp32_alignment", "batch", "edges", "general"]
    got = list(inspect.signature(gat.GATv2Layer.forward_fused).parameters)
    assert got == ["self", "x_l", "x_r", "att", "negative_slope"]


@pytest.mark.parametrize("align,cols", [(16, 4), (8, 2), (4, 1)])
def test_fast_form_lane_width_follows_alignment(align, cols):
    p = _plan(8, 16, align)
    assert (p["form"], p["cols_per_lane"]) == (1, cols)
    # bf16 rows need R*2 bytes, att and the output R*4
    plan = _shim().gatv2_forward_fused_plan
    assert plan(128, 8, 2, 8, 16, BATCH, EDGES)["cols_per_lane"] == 4
    assert plan(128, 8, 2, 8, 8, BATCH, EDGES)["cols_per_lane"] == 2
    assert _plan(4, 128, 16)["form"] == 1          # L = 32
    assert _plan(1, 2048)["form"] == 0             # C > 1024: nothing runs


@pytest.mark.parametrize("k,c,align,general", [
    (3, 7, 16, False), (5, 33, 16, False), (1, 602, 16, False),
    (8, 16, 16, True),
    (4, 128, 4, False)])   # a power of two, but L = C / R would be 128
def test_general_form(k, c, align, general):
    p = _plan(k, c, align, general=general)
    assert (p["form"], p["cols_per_lane"], p["lane_group"], p["slabs"]) == (
        2, 1, 64, k)


@pytest.mark.parametrize("k,c", [(8, 16), (3, 7)])
def test_scratch_bytes(k, c):
    assert _plan(k, c, edges=256)["scratch_bytes"] == 0
    for edges in (257, EDGES):
        want = (BATCH + edges // 256 + 1) * (k * c + 2 * k) * 4
        assert _plan(k, c, edges=edges)["scratch_bytes"] == want

