"""nts_dot_attention_backward_fused_plan on the host (no GPU): form and lane
width by the header's rule, both grids sized by items * slabs, 16-byte
records per (destination, head), form 0 past C = 1024."""
import pytest

# f, K, elem bytes, row alignment, fp32 alignment, general -> form, R, G, slabs
CASES = [
    (128, 8, 4, 16, 16, False, (1, 4, 32, 1)),
    (128, 8, 2, 8, 16, False, (1, 4, 32, 1)),
    (128, 8, 2, 4, 16, False, (1, 2, 64, 1)),    # bf16 rows 4-byte aligned
    (128, 8, 4, 16, 8, False, (1, 2, 64, 1)),    # a gradient 8-byte aligned
    (128, 8, 4, 4, 16, False, (1, 1, 64, 2)),    # rows one float off
    (128, 8, 2, 2, 16, False, (1, 1, 64, 2)),
    (512, 2, 4, 16, 16, False, (1, 4, 64, 2)),   # C / R = 64, two slabs
    (4, 2, 4, 16, 16, False, (1, 2, 2, 1)),
    (128, 8, 4, 16, 16, True, (2, 1, 64, 8)),    # nts_heads_dbg_general
    (21, 3, 4, 16, 16, False, (2, 1, 64, 3)),    # C no power of two
    (1024, 1, 4, 16, 16, False, (2, 1, 64, 1)),  # C / 4 > 64
]


@pytest.mark.parametrize("f,k,elem,row_al,fp32_al,general,want", CASES)
def test_plan(f, k, elem, row_al, fp32_al, general, want):
    from neutronstarlite_amd import shim
    src, dst, edges = 3000, 700, 22000
    plan = shim.dot_attention_backward_fused_plan(
        f, k, elem, row_al, fp32_al, src, dst, edges, general)
    assert (plan["form"], plan["cols_per_lane"], plan["lane_group"],
            plan["slabs"]) == want, plan
    assert plan["scratch_bytes"] == 16 * dst * k
    # the geometry of the GAT backward; unlike the GATv2 plan's, the CSC grid
    # counts the slabs too: both walks flatten (item, slab) tasks
    assert plan == shim.gat_backward_fused_plan(
        f, k, elem, row_al, fp32_al, src, dst, edges, general)
    def blocks(rows):    # 256 threads; at most rows + edges / 256 + 1 items
        return -(-(rows + edges // 256 + 1) * want[3] * want[2] // 256)

    assert (plan["grid_csr"], plan["grid_csc"]) == (blocks(src), blocks(dst))


@pytest.mark.parametrize("elem", [4, 2])
def test_no_form_past_1024_columns_per_head(elem):
    from neutronstarlite_amd import shim
    plan = shim.dot_attention_backward_fused_plan(
        2050, 2, elem, 16, 16, 3000, 700, 22000)
    assert set(plan.values()) == {0}
