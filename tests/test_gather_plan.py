"""The gather launch decision (nts_gather_plan), checked without a GPU.

plan_gather maps (feature width, pointer alignment, rows, batch, edges,
request) to schedule, window, lane group, vector width, grid and the blocked
flag; launch_gather runs exactly what it returns.  The expected (schedule,
window) pairs are the ones tests/test_gpu_gather_sched.py asserts on hardware;
lane groups, vector widths and grids are worked out by hand from the rules in
include/nts_hip.h and DESIGN.md section 3 (defaults: NTS_SPLIT=256, 8192
workgroups at most for the one-tile launch, 2^20 for the blocked one)."""
import os

import pytest

from tests.conftest import REPO

SO = os.path.join(REPO, "neutronstarlite_amd", "libnts_hip.so")

ITEM, PHASE, XCD = 0, 1, 2


@pytest.fixture(scope="module")
def plan():
    if not os.path.exists(SO):
        import neutronstarlite_amd.build as b
        b.build()
    for name in ("NTS_GATHER_SCHED", "NTS_GATHER_WINDOW", "NTS_GATHER_BLOCKS",
                 "NTS_SPLIT", "NTS_MAX_BLOCKS"):
        assert name not in os.environ, f"{name} would change the plan"
    import neutronstarlite_amd.shim as shim
    return shim.gather_plan


def ceil_div(a, b):
    return -(-a // b)


def test_requested_schedules(plan):
    """The request table of test_requested_schedules_really_run: f=602,
    16-byte alignment (dwordx2), V=2000, ~200 000 edges."""
    for sched, window, ran in [
            (PHASE, 0, (PHASE, 128)), (PHASE, 64, (PHASE, 64)),
            (PHASE, 75, (PHASE, 76)),            # rounded up to dwordx2
            (XCD, 0, (XCD, 64)), (XCD, 38, (XCD, 38)), (XCD, 76, (XCD, 76)),
            (XCD, 152, (XCD, 152)), (XCD, 302, (XCD, 302)),  # 4 and 2 windows
            (XCD, 128, (ITEM, 128)),             # 5 windows: not one a class
            (PHASE, 2000, (ITEM, 128)),          # one window
            (ITEM, 76, (ITEM, 76)), (ITEM, -1, (ITEM, 128))]:
        p = plan(602, 16, 2000, 2000, 200_000, sched, window)
        assert (p["schedule"], p["window"]) == ran, (sched, window, p)
        assert p["vector_width"] == 2
        # blocked exactly when it is not the native one-tile ITEM launch
        assert p["blocked"] == (ran != (ITEM, 128)), (sched, window, p)
        if p["schedule"] == XCD:
            assert p["grid"] % 8 == 0 and p["grid"] >= 8
    # the native launch: one 64-lane group per (item, 128-float slab)
    p = plan(602, 16, 2000, 2000, 200_000, ITEM, -1)
    items = 2000 + 200_000 // 256 + 1
    assert p["lane_group"] == 64
    assert p["grid"] == ceil_div(items * 5 * 64, 256)
    # 76-float windows of dwordx2 lanes: 3 tiles of 16 lanes (48 lane slots)
    # beat 2 of 32 and 1 of 64
    p = plan(602, 16, 2000, 2000, 200_000, XCD, 76)
    assert p["lane_group"] == 16
    assert p["grid"] == ceil_div(ceil_div(items * 8 * 3 * 16, 256), 8) * 8


@pytest.mark.parametrize("v,e,f,ran", [
    (70_000, 2_800_000, 128, (ITEM, 128)),    # one window
    (115_000, 575_000, 602, (ITEM, 128)),     # 277 MB, ~5 edges per row
    (20_000, 800_000, 602, (ITEM, 128)),      # 48 MB fits the Infinity Cache
    (112_000, 3_700_000, 602, (PHASE, 128)),  # every condition met
])
def test_automatic_choice(plan, v, e, f, ran):
    p = plan(f, 16, v, v, e)
    assert (p["schedule"], p["window"]) == ran, p
    assert p["blocked"] == (ran[0] == PHASE)
    # an unknown row count never engages
    p0 = plan(f, 16, 0, v, e)
    assert (p0["schedule"], p0["window"], p0["blocked"]) == (ITEM, 128, False)


def test_headline_launch_geometry(plan):
    """Default workload of bench.py: phase-major over five 128-float
    windows, one task per 64-lane group (the grid stays under its 2^20 cap)."""
    v, e = 232_965, 114_232_965
    p = plan(602, 16, v, v, e)
    items = v + e // 256 + 1
    assert p == {"schedule": PHASE, "window": 128, "lane_group": 64,
                 "vector_width": 2, "grid": ceil_div(items * 5 * 64, 256),
                 "blocked": True}
    assert p["grid"] < 1 << 20


@pytest.mark.parametrize("f,align,elem,group,window", [
    (1, 16, 1, 16, 64),     # 4 strided dwords per lane: a 16-lane slab is 64
    (2, 16, 2, 16, 32),
    (7, 16, 1, 16, 64),
    (33, 16, 1, 16, 64),    # 9 lanes of 4 dwords: still the 16-lane group
    (34, 16, 2, 32, 64),    # 17 dwordx2 lanes
    (128, 16, 4, 32, 128),
    (256, 16, 4, 64, 256),
    (602, 8, 2, 64, 128),
    (602, 4, 1, 64, 256),   # unaligned rows: strided dwords, 3 slabs
    (604, 16, 4, 64, 256),
    (604, 8, 2, 64, 128),
])
def test_geometry_at_the_narrow_ends(plan, f, align, elem, group, window):
    v, e = 1000, 20_000
    p = plan(f, align, v, v, e)
    assert p == {"schedule": ITEM, "window": window, "lane_group": group,
                 "vector_width": elem, "blocked": False,
                 "grid": ceil_div((v + e // 256 + 1) * ceil_div(f, window)
                                  * group, 256)}


@pytest.mark.parametrize("f", [1, 2, 7, 33, 602])
@pytest.mark.parametrize("sched", [ITEM, PHASE, XCD])
def test_window_wider_than_f_is_one_window(plan, f, sched):
    """One window is the native launch under every schedule."""
    native = plan(f, 16, 1000, 1000, 20_000, ITEM, -1)
    assert not native["blocked"]
    assert plan(f, 16, 1000, 1000, 20_000, sched, 2000) == native


def test_xcd_falls_back_to_the_native_launch(plan):
    native = plan(602, 16, 2000, 2000, 200_000, ITEM, -1)
    # 5 windows of 128: neither one a class nor an even share of one
    assert plan(602, 16, 2000, 2000, 200_000, XCD, 128) == native
    # V=2, E=3 (test_tiny_grid_covers_every_column): 3 items at most, so 5
    # or 6 workgroups — fewer than the 8 classes
    tiny = plan(602, 16, 2, 2, 3, ITEM, -1)
    assert (tiny["schedule"], tiny["window"], tiny["blocked"]) == (
        ITEM, 128, False)
    for window in (76, 38, 64, 152):
        assert plan(602, 16, 2, 2, 3, XCD, window) == tiny
    # V=10 has the workgroups: the request runs
    p = plan(602, 16, 10, 10, 30, XCD, 76)
    assert (p["schedule"], p["window"], p["blocked"]) == (XCD, 76, True)


def test_nothing_to_launch(plan):
    for f, batch, edges in [(0, 10, 10), (602, 0, 10), (602, 10, 0)]:
        p = plan(f, 16, 10, batch, edges)
        assert p["grid"] == 0 and not p["blocked"]
