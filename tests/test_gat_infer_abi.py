"""The fused GAT inference forward is part of the C-ABI and of the Python
binding (no compute calls: runs without a GPU)."""
import ctypes
import inspect
import os

from tests.conftest import REPO

SO = os.path.join(REPO, "neutronstarlite_amd", "libnts_hip.so")
ENTRIES = ("nts_gat_forward_fused", "nts_gat_forward_fused_bf16")


def _built():
    if not os.path.exists(SO):
        import neutronstarlite_amd.build as b
        b.build()
    return SO


def test_fused_forward_symbols_exported():
    lib = ctypes.CDLL(_built())
    missing = [n for n in ENTRIES if not hasattr(lib, n)]
    assert not missing, f"not exported: {missing}"
    hdr = open(os.path.join(REPO, "include", "nts_hip.h")).read()
    for n in ENTRIES:
        assert f"void {n}(" in hdr


def test_shim_binds_fused_forward():
    import neutronstarlite_amd.shim as shim
    _built()
    l = shim.lib()
    # stream, 6 pointers, slope, column_offset, 8 unsigned counts
    for n in ENTRIES:
        at = getattr(l, n).argtypes
        assert len(at) == 17
        assert at[7] is ctypes.c_float
        assert all(a is ctypes.c_void_p for a in at[:7] + [at[8]])
        assert all(a is ctypes.c_uint32 for a in at[9:])
    want = ["self", "x_ptr", "y_ptr", "s_src_mirror", "s_dst", "row_indices",
            "mirror_index", "slope", "column_offset", "src_s", "src_e",
            "dst_s", "dst_e", "edges", "batch", "f", "heads"]
    got = list(inspect.signature(shim.Stream.gat_forward_fused).parameters)
    assert got == want
    got = list(inspect.signature(shim.Stream.gat_forward_fused_bf16).parameters)
    assert got == ["self", "x_bf16"] + want[2:]


def test_layer_has_infer():
    from neutronstarlite_amd import gat
    params = list(inspect.signature(gat.GATLayer.infer).parameters)
    assert params == ["self", "h", "s_src", "s_dst", "negative_slope"]
    assert not hasattr(gat.GATv2Layer, "infer")   # out of scope: a row pass
