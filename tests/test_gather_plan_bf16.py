"""The launch decision of the bfloat16 gather (nts_gather_plan_bf16), checked
without a GPU.

Same rules as tests/test_gather_plan.py with a 2-byte row element: a lane
takes the widest of 16, 8 or 4 bytes of a row that the width and the
pointers' common alignment allow (8, 4 or 2 elements), else 4 strided single
elements; the lane group is the smallest power of two in [16,64] whose slab
covers the width; and the automatic choice compares the REAL bytes of the
gathered matrix (rows x f x 2) with the 256 MiB Infinity Cache.  The fp32
plan must not move."""
import os

import pytest

from tests.conftest import REPO

SO = os.path.join(REPO, "neutronstarlite_amd", "libnts_hip.so")

ITEM, PHASE, XCD = 0, 1, 2
CAP = 1 << 20        # grid cap of the column-blocked launches
CACHE = 256 << 20    # Infinity Cache


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


@pytest.fixture(scope="module")
def plan(shim):
    return shim.gather_plan_bf16


def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("f,align,elem", [
    (608, 16, 8), (608, 8, 4), (604, 16, 4), (602, 16, 2), (608, 4, 2),
    (601, 16, 1), (602, 2, 1),
    (608, 2, 1), (8, 16, 8), (2, 16, 2), (1, 16, 1),
])
def test_lane_width_from_width_and_alignment(plan, f, align, elem):
    assert plan(f, align, 1000, 1000, 20_000)["vector_width"] == elem


@pytest.mark.parametrize("f,align,elem,group,window", [
    (1, 16, 1, 16, 64),      # 4 strided elements per lane: 16 lanes cover 64
    (7, 16, 1, 16, 64),
    (33, 16, 1, 16, 64),
    (130, 16, 2, 64, 128),   # 65 lanes of 2: two slabs
    (132, 16, 4, 64, 256),   # 33 lanes of 4
    (136, 16, 8, 32, 256),   # 17 lanes of 8
    (128, 16, 8, 16, 128),
    (602, 16, 2, 64, 128),   # the headline width: 1204-byte pitch
    (602, 2, 1, 64, 256),
    (608, 16, 8, 64, 512),
    (608, 8, 4, 64, 256),
    (608, 4, 2, 64, 128),
    (1433, 16, 1, 64, 256),
])
def test_lane_group_and_native_slab(plan, f, align, elem, group, window):
    """The smallest power of two in [16,64] covering ceil(f / elements per
    lane), the slab that group spans, and the one-tile grid."""
    v, e = 1000, 20_000
    p = plan(f, align, v, v, e)
    assert p == {"schedule": ITEM, "window": window, "lane_group": group,
                 "vector_width": elem, "blocked": False,
                 "grid": ceil_div((v + e // 256 + 1) * ceil_div(f, window)
                                  * group, 256)}


def test_engagement_counts_real_bytes(shim, plan):
    """270 MB of fp32 rows exceed the Infinity Cache and engage the blocked
    schedule; the same matrix in bf16 is 135 MB, fits, and runs the native
    launch."""
    v, e, f = 112_000, 3_700_000, 602
    assert v * f * 4 > CACHE > v * f * 2
    p32 = shim.gather_plan(f, 16, v, v, e)
    assert (p32["schedule"], p32["window"], p32["blocked"]) == (
        PHASE, 128, True)
    p16 = plan(f, 16, v, v, e)
    assert (p16["schedule"], p16["window"], p16["blocked"]) == (
        ITEM, 128, False)
    assert p16["vector_width"] == 2 and p16["lane_group"] == 64


def test_engaged_bf16_plan_is_self_consistent(plan):
    """277 MB in bf16 at ~35 edges per row meets every engagement condition.
    Which schedule then runs is a measured choice; whatever it is, the
    window is whole lanes, the windows cover f and the grid fits its cap."""
    v, e, f = 230_000, 8_000_000, 602
    assert v * f * 2 > CACHE and e // 32 >= v
    p = plan(f, 16, v, v, e)
    assert p["vector_width"] == 2
    assert p["schedule"] in (ITEM, PHASE, XCD)
    assert p["window"] > 0 and p["window"] % p["vector_width"] == 0
    assert ceil_div(f, p["window"]) * p["window"] >= f
    assert p["lane_group"] in (16, 32, 64)
    assert 0 < p["grid"] <= CAP
    if p["schedule"] == XCD:
        assert p["grid"] % 8 == 0
    if not p["blocked"]:
        assert (p["schedule"], p["window"]) == (ITEM, 128)
    # unknown rows, few edges per row, or a matrix that fits: never engaged
    for rows, edges in [(0, e), (v, 5 * v), (100_000, 4_000_000)]:
        q = plan(f, 16, rows, rows or v, edges)
        assert (q["schedule"], q["window"], q["blocked"]) == (
            ITEM, 128, False), (rows, edges, q)


def test_headline_launch_geometry(plan):
    """The bench.py graph with bf16 rows (280 MB): the measured automatic
    choice, XCD-affine over two 302-column windows; 302 columns of 2-element
    lanes are 5 tiles of 32 lanes (160 lane slots against 192 for 3 x 64)."""
    v, e = 232_965, 114_232_965
    items = v + e // 256 + 1
    assert plan(602, 16, v, v, e) == {
        "schedule": XCD, "window": 302, "lane_group": 32, "vector_width": 2,
        "grid": ceil_div(ceil_div(items * 2 * 5 * 32, 256), 8) * 8,
        "blocked": True}
    assert plan(602, 16, v, v, e)["grid"] < CAP
    # the padded width: 8-element lanes round the window to 304
    p = plan(608, 16, v, v, e)
    assert (p["schedule"], p["window"], p["vector_width"]) == (XCD, 304, 8)
    # a width that 302-column windows cut into 5: the native launch
    p = plan(1433, 16, v, v, e)
    assert (p["schedule"], p["window"], p["blocked"]) == (ITEM, 256, False)


def test_requested_schedules(plan):
    """The request table of tests/test_gather_plan.py at f=602: a 2-element
    bf16 lane rounds windows exactly as a dwordx2 fp32 lane does."""
    for sched, window, ran in [
            (PHASE, 0, (PHASE, 128)), (PHASE, 64, (PHASE, 64)),
            (PHASE, 75, (PHASE, 76)),            # rounded up to 2 elements
            (XCD, 0, (XCD, 64)), (XCD, 38, (XCD, 38)), (XCD, 76, (XCD, 76)),
            (XCD, 152, (XCD, 152)), (XCD, 302, (XCD, 302)),  # 4 and 2 windows
            (XCD, 128, (ITEM, 128)),             # 5 windows: not one a class
            (PHASE, 2000, (ITEM, 128)),          # one window
            (ITEM, 76, (ITEM, 76)), (ITEM, -1, (ITEM, 128))]:
        p = plan(602, 16, 2000, 2000, 200_000, sched, window)
        assert (p["schedule"], p["window"]) == ran, (sched, window, p)
        assert p["vector_width"] == 2
        assert p["blocked"] == (ran != (ITEM, 128)), (sched, window, p)
        if p["schedule"] == XCD:
            assert p["grid"] % 8 == 0 and p["grid"] >= 8


def test_windows_round_to_the_bf16_lane(plan):
    """f=608 on 8-element lanes: requested windows round up to 8 columns."""
    for window, ran in [(64, 64), (76, 80), (38, 40), (152, 152), (150, 152)]:
        p = plan(608, 16, 2000, 2000, 200_000, PHASE, window)
        assert (p["schedule"], p["window"], p["vector_width"]) == (
            PHASE, ran, 8), (window, p)
        assert p["blocked"]
    # 8-byte alignment: 4-element lanes round to 4
    p = plan(608, 8, 2000, 2000, 200_000, PHASE, 38)
    assert (p["window"], p["vector_width"]) == (40, 4)


def test_tiny_and_empty(plan):
    tiny = plan(602, 16, 2, 2, 3, ITEM, -1)
    assert (tiny["schedule"], tiny["window"], tiny["blocked"]) == (
        ITEM, 128, False)
    for window in (76, 38, 64, 152):   # fewer workgroups than XCD classes
        assert plan(602, 16, 2, 2, 3, XCD, window) == tiny
    p = plan(602, 16, 10, 10, 30, XCD, 76)
    assert (p["schedule"], p["window"], p["blocked"]) == (XCD, 76, True)
    for f, batch, edges in [(0, 10, 10), (602, 0, 10), (602, 10, 0)]:
        p = plan(f, 16, 10, batch, edges)
        assert p["grid"] == 0 and not p["blocked"]


def test_fp32_plan_unchanged(shim):
    """Spot re-check of what tests/test_gather_plan.py pins."""
    v, e = 232_965, 114_232_965
    items = v + e // 256 + 1
    assert shim.gather_plan(602, 16, v, v, e) == {
        "schedule": PHASE, "window": 128, "lane_group": 64,
        "vector_width": 2, "grid": ceil_div(items * 5 * 64, 256),
        "blocked": True}
    for f, align, elem, group, window in [
            (1, 16, 1, 16, 64), (128, 16, 4, 32, 128), (602, 8, 2, 64, 128),
            (602, 4, 1, 64, 256), (604, 16, 4, 64, 256), (608, 16, 4, 64, 256)]:
        p = shim.gather_plan(f, align, 1000, 1000, 20_000)
        assert (p["vector_width"], p["lane_group"], p["window"]) == (
            elem, group, window), (f, align, p)
