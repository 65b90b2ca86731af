"""The stripe decision (nts_gather_stripe_plan) and the striped kernel's task
decode (nts_gather_stripe_task), checked without a GPU.

plan_stripe sits on top of plan_stage: a staged PHASE launch may cut its
window into stripes owned by XCD classes (include/nts_hip.h, DESIGN.md
section 3, Stripes).  Automatic stripes need fp32 rows and a launch that is
staged and PHASE by automatic choice; any schedule or staging request without
a stripe request leaves the launch as it was.  nts_gather_stage_plan and
nts_gather_plan keep reporting the launch without stripes."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stripe_ref
from tests.conftest import REPO

SO = os.path.join(REPO, "neutronstarlite_amd", "libnts_hip.so")

ITEM, PHASE, XCD = 0, 1, 2
AUTO, FORCE, NEVER = 0, 1, -1
# the automatic constants (NTS_AUTO_STRIPE_STAGED, NTS_AUTO_STRIPE_RUN)
AUTO_STRIPE, AUTO_RUN = 64, 16
GRID_CAP = 1 << 20  # NTS_GATHER_BLOCKS

ENV = ("NTS_GATHER_SCHED", "NTS_GATHER_WINDOW", "NTS_GATHER_BLOCKS",
       "NTS_SPLIT", "NTS_MAX_BLOCKS", "NTS_GATHER_STAGE",
       "NTS_GATHER_STAGE_PITCH", "NTS_GATHER_STRIPE", "NTS_GATHER_STRIPE_RUN")

STRIPE_KEYS = ("stripe", "stripe_lanes", "subgroups", "stripes",
               "tasks_per_wave")
HEADLINE = (602, 8, 8, 232_965, 232_965, 114_232_965)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        import neutronstarlite_amd.build as b
        b.build()
    for name in ENV:
        assert name not in os.environ, f"{name} would change the plan"
    import neutronstarlite_amd.shim as shim
    return shim


def ceil_div(a, b):
    return -(-a // b)


def stage_part(p):
    return {k: v for k, v in p.items() if k not in STRIPE_KEYS}


def assert_no_stripes(shim, p, args, **req):
    """the plan is the stage plan of the same arguments, nothing more"""
    assert [p[k] for k in STRIPE_KEYS] == [0] * 5, p
    req.pop("stripe", None)
    req.pop("run", None)
    assert stage_part(p) == shim.gather_stage_plan(*args, **req), p


def test_headline_plan(shim):
    v, e = HEADLINE[3], HEADLINE[5]
    p = shim.gather_stripe_plan(*HEADLINE)
    items = v + e // 256 + 1
    # two stripes: each class deals every fourth item over the four full
    # windows; the 90-float last window has 2 live stripes of 64 as well
    per_class = 5 * ceil_div(items, 4)
    grid = 8 * ceil_div(ceil_div(per_class, AUTO_RUN), 4)
    assert p == {"staged": True, "pitch": 608, "schedule": PHASE,
                 "window": 128, "lane_group": AUTO_STRIPE // 4,
                 "vector_width": 4, "store_width": 2, "grid": grid,
                 "blocked": True, "stripe": AUTO_STRIPE,
                 "stripe_lanes": AUTO_STRIPE // 4,
                 "subgroups": 256 // AUTO_STRIPE,
                 "stripes": 128 // AUTO_STRIPE, "tasks_per_wave": AUTO_RUN}
    assert p["grid"] % 8 == 0 and 8 <= p["grid"] <= GRID_CAP
    # the reports without stripes are what they were
    assert shim.gather_stage_plan(*HEADLINE) == {
        "staged": True, "pitch": 608, "schedule": PHASE, "window": 128,
        "lane_group": 32, "vector_width": 4, "store_width": 2,
        "grid": ceil_div(items * 5 * 32, 256), "blocked": True}
    assert shim.gather_plan(602, 8, v, v, e) == {
        "schedule": PHASE, "window": 128, "lane_group": 64,
        "vector_width": 2, "grid": ceil_div(items * 5 * 64, 256),
        "blocked": True}


@pytest.mark.parametrize("v,e,f,why", [
    (112_000, 3_700_000, 602, "33 edges per row"),
    (20_000, 800_000, 602, "48 MB fits the Infinity Cache"),
    (115_000, 575_000, 602, "5 edges per row"),
    (232_965, 114_232_965, 608, "the pitch is whole lines already"),
    (1_000_000, 114_232_965, 256, "the pitch is whole lines already"),
    (2_000_000, 200_000_000, 128, "the pitch is whole lines already"),
    (70_000, 2_800_000, 128, "one window"),
])
def test_stripes_stay_off_where_staging_does(shim, v, e, f, why):
    """every row of test_gather_stage_plan.test_automatic_staging_stays_off"""
    for align in (16, 8, 4):
        args = (f, align, align, v, v, e)
        p = shim.gather_stripe_plan(*args)
        assert not p["staged"], why
        assert_no_stripes(shim, p, args)


def test_stripes_stay_off(shim):
    f, ai, ao, v, b, e = HEADLINE
    # bf16 rows
    p = shim.gather_stripe_plan(f, 4, 8, v, b, e, elem_bytes=2)
    assert_no_stripes(shim, p, (f, 4, 8, v, b, e), elem_bytes=2)
    p = shim.gather_stripe_plan(f, 4, 8, v, b, e, elem_bytes=2, stripe=32)
    assert_no_stripes(shim, p, (f, 4, 8, v, b, e), elem_bytes=2)
    # unknown row count
    for stripe in (0, 32):
        p = shim.gather_stripe_plan(f, ai, ao, 0, b, e, stripe=stripe)
        assert_no_stripes(shim, p, (f, ai, ao, 0, b, e))
    # a schedule or staging request without a stripe request
    for req in (dict(schedule=PHASE, window=128), dict(schedule=PHASE),
                dict(window=-1), dict(schedule=XCD, window=152),
                dict(stage=FORCE), dict(stage=NEVER),
                dict(schedule=PHASE, window=128, stage=FORCE)):
        p = shim.gather_stripe_plan(*HEADLINE, **req)
        assert_no_stripes(shim, p, HEADLINE, **req)
    # never
    p = shim.gather_stripe_plan(*HEADLINE, stripe=NEVER)
    assert_no_stripes(shim, p, HEADLINE)
    p = shim.gather_stripe_plan(*HEADLINE, schedule=PHASE, window=128,
                                stage=FORCE, stripe=NEVER)
    assert_no_stripes(shim, p, HEADLINE, schedule=PHASE, window=128,
                      stage=FORCE)
    # forced, but the launch neither runs PHASE nor was asked to
    for req in (dict(window=-1), dict(schedule=XCD, window=152)):
        p = shim.gather_stripe_plan(*HEADLINE, stage=FORCE, stripe=32, **req)
        assert_no_stripes(shim, p, HEADLINE, stage=FORCE, **req)
    # forced on a launch that is not staged
    p = shim.gather_stripe_plan(*HEADLINE, stage=NEVER, stripe=32)
    assert_no_stripes(shim, p, HEADLINE, stage=NEVER)


@pytest.mark.parametrize("sf,lanes", [(16, 4), (32, 8), (64, 16), (128, 32)])
def test_forced_widths(shim, sf, lanes):
    for args in (HEADLINE, (602, 16, 16, 2000, 2000, 200_000),
                 (32, 16, 16, 2000, 2000, 200_000)):
        p = shim.gather_stripe_plan(*args, schedule=PHASE, window=128,
                                    stage=FORCE, stripe=sf)
        assert p["staged"] and (p["schedule"], p["window"]) == (PHASE, 128)
        assert (p["stripe"], p["stripe_lanes"], p["subgroups"],
                p["stripes"]) == (sf, lanes, 64 // lanes, 128 // sf), p
        assert p["lane_group"] == lanes and p["blocked"]
        assert p["grid"] % 8 == 0 and 8 <= p["grid"] <= GRID_CAP
        # tasks per wave: the fewest that fit the grid cap
        f, v, e = args[0], args[3], args[5]
        items = v + e // 256 + 1
        stripes = 128 // sf
        last_live = ceil_div(f % 128, sf) if f % 128 else 0
        if last_live == stripes:
            last_live = 0
        n_full = ceil_div(f, 128) - (1 if last_live else 0)
        per_class = (n_full * ceil_div(items, 8 // stripes)
                     + ceil_div(items * last_live, 8))
        run = ceil_div(per_class, GRID_CAP // 8 * 4)
        assert p["tasks_per_wave"] == run, (p, per_class)
        assert p["grid"] == 8 * ceil_div(ceil_div(per_class, run), 4)
    # a forced width on the automatic launch, and more tasks per wave
    p = shim.gather_stripe_plan(*HEADLINE, stripe=sf, run=24)
    assert (p["stripe"], p["window"], p["tasks_per_wave"]) == (sf, 128, 24)


@pytest.mark.parametrize("window,sf", [
    (128, 8), (128, 48), (128, 96), (128, 256), (128, 20), (152, 32),
    (256, 16), (512, 32)])
def test_width_that_does_not_cut_the_window_falls_back(shim, window, sf):
    """not 1, 2, 4 or 8 stripes of 4 to 64 dwordx4 lanes"""
    req = dict(schedule=PHASE, window=window, stage=FORCE)
    p = shim.gather_stripe_plan(*HEADLINE, stripe=sf, **req)
    assert_no_stripes(shim, p, HEADLINE, **req)


def test_window_256(shim):
    p = shim.gather_stripe_plan(*HEADLINE, schedule=PHASE, window=256,
                                stage=FORCE, stripe=32)
    assert (p["window"], p["stripe"], p["stripes"], p["subgroups"]) == (
        256, 32, 8, 8)
    p = shim.gather_stripe_plan(*HEADLINE, schedule=PHASE, window=256,
                                stage=FORCE, stripe=256)
    assert (p["stripe"], p["stripes"], p["stripe_lanes"],
            p["subgroups"]) == (256, 1, 64, 1)


@pytest.mark.parametrize("n_items", stripe_ref.N_ITEMS)
def test_coverage_uncapped(shim, n_items):
    """every live (item, window, stripe) exactly once, nothing else"""
    for f in stripe_ref.WIDTHS:
        for sf in stripe_ref.STRIPES:
            p = stripe_ref.check_coverage(shim, n_items, f, sf)
            assert p["tasks_per_wave"] == 1
            # and with a run request: R > 1 without a cap
            stripe_ref.check_coverage(shim, n_items, f, sf, run=3)


@pytest.mark.parametrize("cap", [8, 64])
def test_coverage_under_a_grid_cap(shim, cap):
    """The cap is read once per process: the same check in a child process.
    It prints the tasks per wave it met; a cap of 8 or 64 workgroups forces
    runs of more than one task."""
    env = dict(os.environ, NTS_GATHER_BLOCKS=str(cap))
    r = subprocess.run([sys.executable, "-m", "tests.stripe_ref"], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    runs = ast.literal_eval(r.stdout.strip().splitlines()[-1].split(" ", 1)[1])
    assert max(runs) > 1, runs


def test_coverage_headline_shape_counts(shim):
    """At the headline plan the slots of the first and of the last workgroups
    decode to tasks of window 0 and of the last window (window-major)."""
    p = shim.gather_stripe_plan(*HEADLINE)
    n_items = 634_280
    per_block = 4 * p["tasks_per_wave"]
    it, c0, c1 = shim.gather_stripe_tasks(*HEADLINE, n_items, 0,
                                          8 * per_block)
    assert (c0 < c1).all() and (c0 < 128).all()
    # class c = block % 8 owns stripe c % 2 and items c // 2 + 4 k
    for block in range(8):
        sl = slice(block * per_block, (block + 1) * per_block)
        assert (c0[sl] == (block % 2) * 64).all()
        assert (it[sl] == block // 2 + 4 * range_array(per_block)).all()
    last = (p["grid"] - 8) * per_block
    it, c0, c1 = shim.gather_stripe_tasks(*HEADLINE, n_items, last,
                                          8 * per_block)
    live = c0 < c1
    assert (c0[live] >= 512).all() and (c1[live] <= 602).all()


def range_array(n):
    return np.arange(n, dtype=np.uint32)
