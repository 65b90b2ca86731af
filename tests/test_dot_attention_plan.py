"""nts_dot_attention_forward_fused_plan on the host (no GPU): the geometry and
scratch of nts_gatv2_forward_fused_plan for the same arguments, form 0 exactly
when a head is wider than 1024 columns."""
import itertools

import pytest

SHAPES = [(8, 16), (4, 8), (2, 128), (1, 1), (3, 7), (1, 602), (1, 2048)]


@pytest.mark.parametrize("k,c", SHAPES)
def test_plan_is_the_gatv2_fused_plan(k, c):
    from neutronstarlite_amd import shim
    for elem, align, general, (batch, edges) in itertools.product(
            (4, 2), (16, 8, 4, 2), (False, True), ((700, 22000), (40, 200))):
        args = (k * c, k, elem, align, align, batch, edges, general)
        plan = shim.dot_attention_forward_fused_plan(*args)
        assert plan == shim.gatv2_forward_fused_plan(*args), args
        assert (plan["form"] == 0) == (c > 1024), args
