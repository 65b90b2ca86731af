"""The automatic coalescing rule (nts_coalesce_plan, no device access): a
request of the chunk wins, then the environment's NTS_GATHER_COALESCE, then
the edge-count threshold NTS_COALESCE_MIN_EDGES of include/nts_hip.h."""
import os
import subprocess
import sys

import pytest

from tests.conftest import REPO

MIN_EDGES = 1 << 24   # NTS_COALESCE_MIN_EDGES
HEADLINE_EDGES = 114_232_965


@pytest.fixture(scope="module")
def shim():
    import neutronstarlite_amd.build as b
    import neutronstarlite_amd.shim as shim
    b.build()
    assert "NTS_GATHER_COALESCE" not in os.environ, "would change the plan"
    return shim


def test_threshold_constant(shim):
    assert shim.COALESCE_MIN_EDGES == MIN_EDGES
    text = open(os.path.join(REPO, "include", "nts_hip.h")).read()
    assert "#define NTS_COALESCE_MIN_EDGES (1u << 24)" in text


def test_forced_on_and_off(shim):
    for edges in (0, 1, MIN_EDGES - 1, MIN_EDGES, HEADLINE_EDGES):
        assert shim.coalesce_plan(edges, True) is True
        assert shim.coalesce_plan(edges, False) is False


def test_automatic_threshold(shim):
    assert shim.coalesce_plan(0) is False
    assert shim.coalesce_plan(3_700_000) is False      # largest test graph
    assert shim.coalesce_plan(MIN_EDGES - 1) is False
    assert shim.coalesce_plan(MIN_EDGES) is True
    assert shim.coalesce_plan(HEADLINE_EDGES) is True
    assert shim.coalesce_plan(HEADLINE_EDGES, None) is True


@pytest.mark.parametrize("bad", [0, 1, -1, "yes"])
def test_request_must_be_none_or_bool(shim, bad):
    with pytest.raises(ValueError):
        shim.coalesce_plan(100, bad)


CHILD = """
import neutronstarlite_amd.shim as shim
print([shim.coalesce_plan(e, c) for e in (100, 1 << 24)
       for c in (None, True, False)])
"""


@pytest.mark.parametrize("value,auto", [("1", True), ("-1", False),
                                        ("0", None), ("", None)])
def test_environment_overrides_the_automatic_choice(shim, value, auto):
    """The environment is read once per process, so a child reports.  It
    replaces the automatic choice alone; a request of the chunk still wins."""
    env = dict(os.environ, NTS_GATHER_COALESCE=value)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    small = False if auto is None else auto
    large = True if auto is None else auto
    assert r.stdout.strip().splitlines()[-1] == str(
        [small, True, False, large, True, False])
