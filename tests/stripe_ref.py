"""Coverage of the striped gather's task decode, checked on the CPU.

nts_gather_stripe_task evaluates the very function the kernel runs
(stripe_task in csrc/nts_hip.hip).  check_coverage enumerates every wave slot
(workgroup, wave, run index) of a launch and asserts that every live (work
item, window, stripe) comes out exactly once and nothing else does.

The grid cap NTS_GATHER_BLOCKS is read once per process, so the capped cases
run this module as a program in a child process:

    NTS_GATHER_BLOCKS=8 python -m tests.stripe_ref
"""
import sys

import numpy as np

PHASE, FORCE = 1, 1
WINDOW = 128
N_ITEMS = (1, 7, 8, 9, 1000, 1001)
WIDTHS = (32, 130, 602, 608)
STRIPES = (16, 32, 64, 128)


def expected_tasks(n_items, f, window, sf):
    """every live (item, first column, column bound)"""
    cols = [(c, min(f, c + sf))
            for w in range(0, f, window)
            for c in range(w, min(f, w + window), sf)]
    return {(it, a, b) for it in range(n_items) for a, b in cols}


def check_coverage(shim, n_items, f, sf, cap=None, window=WINDOW, run=0):
    """Returns the plan it checked."""
    # bound_items = batch + edges / 256 + 1 >= n_items: one edge per item
    shape = (f, 16, 16, n_items, n_items, n_items)
    req = dict(schedule=PHASE, window=window, stage=FORCE, stripe=sf,
               run=run)
    plan = shim.gather_stripe_plan(*shape, **req)
    what = f"n_items={n_items} f={f} sf={sf} cap={cap}: {plan}"
    assert plan["stripe"] == sf and plan["staged"], what
    assert (plan["schedule"], plan["window"]) == (PHASE, window), what
    assert plan["stripe_lanes"] == sf // 4, what
    assert plan["subgroups"] * plan["stripe_lanes"] == 64, what
    assert plan["stripes"] * sf == window, what
    assert plan["grid"] % 8 == 0 and plan["grid"] >= 8, what
    assert plan["tasks_per_wave"] >= max(run, 1), what
    if cap is not None:
        assert plan["grid"] <= cap, what
    slots = plan["grid"] * 4 * plan["tasks_per_wave"]
    # past the grid: nothing
    it, c0, c1 = shim.gather_stripe_tasks(*shape, n_items, 0, slots + 64,
                                          **req)
    assert not (c0[slots:] < c1[slots:]).any(), what
    live = c0 < c1
    got = list(zip(it[live].tolist(), c0[live].tolist(), c1[live].tolist()))
    want = expected_tasks(n_items, f, window, sf)
    assert len(got) == len(set(got)), f"a task runs twice; {what}"
    assert set(got) == want, (
        f"{len(want - set(got))} tasks missing, {len(set(got) - want)} "
        f"outside; {what}")
    assert all(b <= f for _, _, b in got), what
    return plan


def check_all(shim, cap=None):
    runs = set()
    for n_items in N_ITEMS:
        for f in WIDTHS:
            for sf in STRIPES:
                runs.add(check_coverage(shim, n_items, f, sf, cap)
                         ["tasks_per_wave"])
    return runs


if __name__ == "__main__":
    import os
    from neutronstarlite_amd import shim
    cap = int(os.environ["NTS_GATHER_BLOCKS"])
    runs = check_all(shim, cap)
    print("tasks_per_wave", sorted(runs))
    sys.exit(0)
