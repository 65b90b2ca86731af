"""nts_gat_backward_fused_plan (no GPU): the form, the columns per lane and
the record scratch the fused GAT backward would launch with, and the new
symbols in the library."""
import ctypes

import pytest

from neutronstarlite_amd import shim

SRC, DST, EDGES = 1000, 700, 20000

# (f, heads, elem_bytes, row alignment, fp32 alignment, general) -> (form, R)
ROWS = [
    ((128, 8, 4, 256, 256, False), (1, 4)),
    ((128, 8, 2, 256, 256, False), (1, 4)),
    ((128, 8, 2, 4, 256, False), (1, 2)),     # bf16 rows: R * 2 bytes
    ((128, 8, 2, 2, 256, False), (1, 1)),
    ((128, 8, 4, 256, 8, False), (1, 2)),     # grad_y | grad_h 8-byte aligned
    ((128, 8, 4, 4, 256, False), (1, 1)),     # fp32 h one float off
    ((4, 2, 4, 256, 256, False), (1, 2)),     # C = 2
    ((16, 16, 4, 256, 256, False), (1, 1)),   # C = 1: one-lane segments
    ((64, 1, 4, 256, 256, False), (1, 4)),
    ((1024, 1, 4, 256, 256, False), (2, 1)),  # C / R = 256 lanes: no segment
    ((21, 3, 4, 256, 256, False), (2, 1)),    # C = 7
    ((128, 8, 4, 256, 256, True), (2, 1)),
    ((2048, 1, 4, 256, 256, False), (0, 0)),
]


@pytest.mark.parametrize("args,want", ROWS)
def test_plan(args, want):
    f, heads = args[:2]
    plan = shim.gat_backward_fused_plan(*args[:5], SRC, DST, EDGES,
                                        general=args[5])
    assert (plan["form"], plan["cols_per_lane"]) == want, plan
    if not want[0]:
        assert plan["scratch_bytes"] == 0 and plan["grid_csr"] == 0
        return
    assert plan["scratch_bytes"] == 16 * DST * heads
    assert plan["grid_csr"] >= plan["grid_csc"] >= 1
    if want[0] == 1:     # slabs of whole heads that cover the row
        width = plan["lane_group"] * plan["cols_per_lane"]
        assert width % (f // heads) == 0 and plan["slabs"] * width >= f
    else:
        assert (plan["lane_group"], plan["slabs"]) == (64, heads)


def test_symbols_and_argument_check():
    lib = ctypes.CDLL(shim._SO)
    for name in ("nts_gat_backward_fused", "nts_gat_backward_fused_bf16",
                 "nts_gat_backward_fused_plan"):
        assert hasattr(lib, name), name
    with pytest.raises(ValueError):          # heads does not divide f
        shim.gat_backward_fused_plan(30, 4, 4, 256, 256, SRC, DST, EDGES)
