"""Every kernel's grid-stride loop and split merge at small sizes (marked gpu).

NTS_SPLIT, NTS_MAX_BLOCKS and NTS_GATHER_BLOCKS are latched once per process,
so each configuration below runs the case driver tests/grid_cases.py in a
fresh child; the checks then only read the children's .npz files.

  base         the defaults: one work item per wave, hubs alone are split
  cap1, cap3   one and three workgroups (4 and 12 waves; a stride that is no
               power of two): every wave walks many items
  split8       most destinations are split and merged
  split8_cap1  both
  blocks8      the column-blocked and striped gather launches under a cap of
               8 workgroups (the scalar gather cases only)

Not vacuous: test_loops_really_wrap asserts from each child's own report that
the work items outnumber the waves (or lane groups, or threads) of the grid
that ran, so a loop that were right on its first iteration only would leave
most of the outputs unwritten and fail the float64 check.

Once a child dies of a signal, an abort or its time limit, no later child is
started: nothing goes to the GPU after a fault or hang.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "base": {},
    "cap1": {"NTS_MAX_BLOCKS": "1"},
    "cap3": {"NTS_MAX_BLOCKS": "3"},
    "split8": {"NTS_SPLIT": "8"},
    "split8_cap1": {"NTS_SPLIT": "8", "NTS_MAX_BLOCKS": "1"},
    "blocks8": {"NTS_GATHER_BLOCKS": "8"},
}
BLOCKS8_CASES = GC.SCALAR_GATHERS + GC.FORCED_GATHERS
# the base child takes 2.2 s on an MI355X with torch warm in the page cache
# (122 cases, import and context creation included); four times that is 9 s,
# and the rest allows for a cold import of torch on a fresh machine
CHILD_TIMEOUT = 30
DEAD_STATUS = (134, 139, 124, 137)

# (configuration, the one it must equal bit for bit, edges per work item)
IDENTITY = {"cap1": ("base", 256), "cap3": ("base", 256),
            "blocks8": ("base", 256), "split8_cap1": ("split8", 8)}
CAPPED = {"cap1": 1, "cap3": 3, "split8_cap1": 1}

# grid-strided over count * f = 300 elements: one workgroup wraps, the three
# of cap3 (768 threads) do not; the f = 37 twin of each wraps in both
TOO_SMALL_TO_WRAP = {("cap3", f"{e}_f1") for e in GC.TRANSFER_ENTRIES}


def cases_of(cfg):
    return BLOCKS8_CASES if cfg == "blocks8" else list(GC.CASES)


def pairs(configs):
    return [(c, n) for c in configs for n in cases_of(c)]


class Run:
    def __init__(self, failure=None, arrays=None, meta=None):
        self.failure, self.arrays, self.meta = failure, arrays, meta

    def get(self, case, key):
        return self.arrays[f"{case}/{key}"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out, dead = {}, None
    tmp = tmp_path_factory.mktemp("grid_cases")
    for cfg, extra in CONFIGS.items():
        if dead:
            out[cfg] = Run(failure=f"not started: {dead}")
            continue
        env = {k: v for k, v in os.environ.items() if not k.startswith("NTS_")}
        env.update(extra)
        path = str(tmp / f"{cfg}.npz")
        cmd = [sys.executable, "-m", "tests.grid_cases", "--out", path]
        if cfg == "blocks8":
            cmd += ["--only", ",".join(BLOCKS8_CASES)]
        t0 = time.time()
        try:
            p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                               text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            err = e.stderr.decode(errors="replace") if isinstance(
                e.stderr, bytes) else (e.stderr or "")
            dead = f"child {cfg} hit its {CHILD_TIMEOUT} s limit\n{err[-2000:]}"
            out[cfg] = Run(failure=dead)
            continue
        print(f"child {cfg}: {time.time() - t0:.1f} s, exit {p.returncode}")
        if p.returncode < 0 or p.returncode in DEAD_STATUS:
            dead = (f"child {cfg} died with status {p.returncode}\n"
                    f"{p.stderr[-2000:]}")
            out[cfg] = Run(failure=dead)
        elif p.returncode != 0:
            out[cfg] = Run(failure=f"child {cfg} failed with status "
                                   f"{p.returncode}\n{p.stderr[-2000:]}")
        else:
            with np.load(path) as z:
                arrays = {k: z[k] for k in z.files}
            meta = json.loads(str(arrays.pop("__meta__")))
            assert meta["env"] == extra, (meta["env"], extra)
            out[cfg] = Run(arrays=arrays, meta=meta)
    return out


def _run(runs, cfg):
    r = runs[cfg]
    assert r.failure is None, r.failure
    return r


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _rows(e, limit):
    """Rows whose value does not depend on the order of any merge."""
    return np.asarray(e.deg) <= (1 if e.atomic else limit)


# --------------------------------------------------------------------------
# against float64, and the exact results, in every configuration
# --------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,case", pairs(CONFIGS))
def test_against_reference(runs, cfg, case):
    """Every output within the bound the entry's own GPU test holds it to
    against the same reference (grid_cases.py names it per case); exact
    outputs (copies, max / min and arg, the sampler) equal; rows without
    terms still hold the prefill bit for bit."""
    r = _run(runs, cfg)
    worst = 0.0
    for key, e in GC.CASES[case].expect().items():
        got = r.get(case, key)
        name = f"{cfg} {case} {key}"
        ref = np.asarray(e.ref)
        assert got.shape == ref.shape, f"{name}: shape {got.shape}"
        if e.bound is None:
            want = ref.astype(got.dtype)
            bad = (got != want) if e.exact == "value" else (
                _bits(got) != _bits(want))
            assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} differ"
        else:
            assert np.isfinite(got).all(), f"{name}: non-finite output"
            err = np.abs(got.astype(np.float64) - ref)
            bound = np.broadcast_to(e.bound, err.shape)
            ratio = np.where(err > 0,
                             err / np.where(bound > 0, bound, 1e-300), 0.0)
            worst = max(worst, float(ratio.max()))
            bad = err > bound
            assert not bad.any(), (f"{name}: {bad.sum()}/{bad.size} out of "
                                   f"bound, worst {ratio.max():.3e} of it")
        if e.prefill is not None:
            empty = np.asarray(e.deg) == 0
            assert empty.any(), name
            assert (_bits(got[empty]) == _bits(
                np.asarray(e.prefill, dtype=got.dtype)[empty])).all(), (
                f"{name}: a row without terms was written")
    print(f"worst err/bound {cfg} {case}: {worst:.3e}")


# --------------------------------------------------------------------------
# bit-identity across grids
# --------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,case", pairs(IDENTITY))
def test_bit_identical_across_grids(runs, cfg, case):
    """An output element of a vertex that is one work item is one lane's
    chain in edge order, whatever the grid: equal to the uncapped run on the
    rows of at most 256 (8) edges.  Rows fed by atomics of several items
    count only with at most one term; grad_input of the indexed
    reduce_backward takes no part (its order is not fixed)."""
    base_cfg, limit = IDENTITY[cfg]
    r, b = _run(runs, cfg), _run(runs, base_cfg)
    checked = 0
    for key, e in GC.CASES[case].expect().items():
        if e.deg is None:
            continue
        rows = _rows(e, limit)
        got, want = r.get(case, key), b.get(case, key)
        bad = _bits(got[rows]) != _bits(want[rows])
        assert not bad.any(), (f"{cfg} {case} {key}: {bad.sum()}/{bad.size} "
                               f"elements differ from {base_cfg}")
        checked += int(rows.sum())
    assert checked or case == "reduce_backward_csc"


@pytest.mark.parametrize("case", GC.FORCED_GATHERS)
@pytest.mark.parametrize("cfg", ["base", "blocks8"])
def test_requested_gather_form_ran(runs, cfg, case):
    """(schedule, window, staged, pitch, stripe, tasks per wave) the launch
    reports: the forced form, not a fallback."""
    sched, window, stage, stripe = GC.FORCED[case.rsplit("_", 1)[1]]
    ran = _run(runs, cfg).get(case, "ran").tolist()
    assert ran[:2] == [sched, window], ran
    assert bool(ran[2]) == bool(stage), ran
    assert ran[4] == stripe and (ran[5] >= 1) == bool(stripe), ran
    if cfg == "blocks8" and stripe:
        assert ran[5] > 1, f"{case}: one task per wave, nothing wraps"


# --------------------------------------------------------------------------
# not vacuous
# --------------------------------------------------------------------------
def _units(cfg, case, info):
    """Waves, lane groups or threads of the grid that ran."""
    c = GC.CASES[case]
    plan = info["plan"]
    grid = plan["grid"] if plan else CAPPED[cfg]
    if c.unit == "thread":
        return grid * GC.BLOCK
    if c.unit == "group" and not plan.get("stripe"):
        return grid * GC.BLOCK // plan["lane_group"]
    return grid * 4


def _wrap_pairs():
    """The forced gather forms are capped by NTS_GATHER_BLOCKS alone."""
    out = [(c, n) for c, n in pairs(CAPPED) if not GC.CASES[n].blocked]
    out += [("blocks8", n) for n in GC.FORCED_GATHERS]
    return [p for p in out if p not in TOO_SMALL_TO_WRAP]


@pytest.mark.parametrize("cfg,case", _wrap_pairs())
def test_loops_really_wrap(runs, cfg, case):
    r = _run(runs, cfg)
    info = r.meta["cases"][case]
    if info["plan"] and cfg in CAPPED:
        assert info["plan"]["grid"] <= CAPPED[cfg], info
    units = _units(cfg, case, info)
    assert info["work"] > units, (
        f"{cfg} {case}: {info['work']} work items on {units} {info['unit']}s")


def test_split8_splits_most_destinations(runs):
    """The child really ran at split 8, where more than three quarters of
    the non-empty destinations of the edge-case graph are several work items
    (its sources mostly have fewer than 8 edges; there the 118 larger ones of
    grid_case_graph are split)."""
    assert _run(runs, "split8").meta["split"] == 8
    assert _run(runs, "base").meta["split"] == 256
    deg = GC.degrees("csc")
    assert (deg > 8).sum() > 0.75 * (deg > 0).sum()
    assert (GC.degrees("csr") > 8).sum() >= 64
