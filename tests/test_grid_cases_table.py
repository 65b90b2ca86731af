"""The case table of tests/grid_cases.py, checked without a device: that it
covers the entry points it is meant to cover, that --only resolves, and that
the graphs and inputs give the checks of tests/test_gpu_grid_cap.py something
to bite on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_cases as GC  # noqa: E402

# The entry points the table must run, with the number of forms of each:
# (widths) x (directions) x (fast / general) x (softmax modes) as listed.
# Written from the list of entries, not from the table: an entry that goes
# missing from grid_cases.py fails test_one_case_per_entry_and_form.
ENTRIES = {
    # gathers: f = 33 and 64, with and without weights; the forward one also
    # in the three forced column schedules of blocks8
    "gather_by_dst_from_src": 4 + 3, "gather_by_src_from_dst": 4,
    "gather_by_dst_from_src_bf16": 4, "gather_by_src_from_dst_bf16": 4,
    # heads pairs at (K, C) = (8, 8) and (3, 7)
    "gather_by_dst_from_src_heads": 2, "gather_by_src_from_dst_heads": 2,
    "gather_by_dst_from_src_heads_bf16": 2,
    "gather_by_src_from_dst_heads_bf16": 2,
    "gather_by_src_from_dst_dot": 1,
    # the five k_edge_items ops at f = 1 and 5
    "scatter_src_mirror_to_msg": 2, "scatter_dst_to_msg": 2,
    "gather_msg_to_src_mirror": 2, "gather_msg_to_dst": 2,
    "scatter_grad_back_to_message": 2,
    # softmax and attention, both modes; the heads entry fast and general
    "edge_softmax_forward": 2, "edge_softmax_forward_dual": 2,
    "edge_softmax_backward": 2, "edge_softmax_backward_fused": 2,
    "edge_attention_forward": 2, "edge_attention_forward_heads": 4,
    "edge_dot": 1, "edge_dot_heads": 3, "edge_dot_heads_bf16": 2,
    "weight_sum": 2, "weight_sum_heads": 4, "permute_f32": 1,
    # dropout at p = 0.3: the forwards in both modes
    "edge_attention_forward_drop": 2, "edge_softmax_forward_drop": 2,
    "edge_softmax_backward_drop": 1,
    # GATv2: fast and general; the backward in both directions
    "edge_gatv2_score": 2, "edge_gatv2_backward": 4,
    "edge_gatv2_score_bf16": 2, "edge_gatv2_backward_bf16": 4,
    # fused: both modes; GATv2 forward and GAT backward fast and general
    "gat_forward_fused": 2, "gat_forward_fused_bf16": 2,
    "gatv2_forward_fused": 4, "gatv2_forward_fused_bf16": 4,
    "gat_backward_fused": 4, "gat_backward_fused_bf16": 4,
    # max / min in the CSC and the message form, and the backward of each
    "reduce_by_dst_from_src": 4, "reduce_backward": 2,
    # sampler at fanout 4 and 10
    "sample_reservoir": 2, "sample_reservoir_dbg_fallback": 2,
    # transfer and row pack at f = 37 and 1
    "deserialize_to_gpu": 2, "aggregate_comm_result": 2, "gather_rows": 2,
    "scatter_rows": 2, "scatter_add_rows": 2,
}


def test_one_case_per_entry_and_form():
    from neutronstarlite_amd import shim
    count = {}
    for c in GC.CASES.values():
        assert hasattr(shim.Stream, c.entry), c.entry
        count[c.entry] = count.get(c.entry, 0) + 1
    assert count == ENTRIES


def test_only_resolves():
    assert GC.resolve("") == list(GC.CASES)
    names = GC.SCALAR_GATHERS + GC.FORCED_GATHERS
    assert GC.resolve(",".join(names)) == names
    assert all(n in GC.CASES for n in names)
    with pytest.raises(SystemExit):
        GC.resolve("permute_f32,no_such_case")


@pytest.mark.parametrize("direction", ["csc", "csr"])
def test_identity_checks_cover_enough_rows(direction):
    deg = GC.degrees(direction)
    assert ((deg > 0) & (deg <= 8)).sum() >= 64
    assert (deg > 8).sum() >= 64
    assert (deg > 256).sum() >= 1
    assert (deg == 0).any()
    # at split 8 the items outnumber the 12 waves of the cap3 grid
    assert GC.item_count(direction, 8) > 12
    assert GC.item_count(direction, 8) > GC.item_count(direction, 256)


def test_csr_graph_keeps_the_shape_of_the_edge_case_graph():
    a, b = GC.R.edge_case_graph(), GC.R.grid_case_graph()
    assert (a.deg == b.deg).all() and a.edges == b.edges
    assert (a.src_start, a.v_src) == (b.src_start, b.v_src)
    assert b.row_indices.min() >= b.src_start
    assert b.row_indices.max() < b.src_start + b.v_src


@pytest.mark.parametrize("form", ["csc", "msg"])
@pytest.mark.parametrize("op", ["max", "min"])
def test_reduce_input_is_tied(form, op):
    assert GC.reduce_tied_pairs(form, op) >= 32


def test_dropout_mask_drops_and_keeps():
    """p = 0.3 on the dropout graph: both kinds of position occur, and the
    library's host mask is the reference's."""
    for width in (GC.DROP_HEADS, GC.DROP_F, 1):
        keep = GC._keep(width)
        assert 0.6 < keep.mean() < 0.8
        assert (keep == GC.D.keep_edges(GC.DROP_SEED, GC.DROP_P, len(keep),
                                        width)).all()


@pytest.mark.parametrize("f", [37, 1])
def test_atomic_transfer_ids_repeat(f):
    ids, payload, _, dense = GC.transfer_case(f, True)
    _, _, terms = GC.transfer_sum(ids, payload, dense)
    assert len(ids) == GC.T_COUNT and ids.min() >= GC.T_START
    assert (terms >= 2).sum() >= 32 and (terms == 0).any()
    ids = GC.transfer_case(f, False)[0]
    assert len(np.unique(ids)) == GC.T_COUNT


def test_every_expectation_matches_its_rows():
    """deg has one entry per leading row of its output; bounds are finite
    and none is negative."""
    for name, c in GC.CASES.items():
        for key, e in c.expect().items():
            ref = np.asarray(e.ref)
            if e.deg is not None:
                assert len(e.deg) == ref.shape[0], (name, key)
            if e.bound is not None:
                b = np.broadcast_to(e.bound, ref.shape)
                assert np.isfinite(b).all() and (b >= 0).all(), (name, key)
            if e.prefill is not None:
                assert np.asarray(e.prefill).shape == ref.shape, (name, key)
