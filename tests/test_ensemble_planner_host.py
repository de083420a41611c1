"""The planner's parameter sets per group and an Ensemble's global planner, as far as they can be checked without a device: the
binding declares the new functions with the header's arity, mgx_plan_done carries `group`, the Ensemble's validation of rrt.* and
of the world it is given, and what tools/run_scenarios.py makes of the new combinations of arguments."""
import copy
import os
import re
import subprocess
import sys

import pytest

from magics_amd import config, hostlib
from magics_amd.ensemble import RRT_KEYS, Ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mgx_planner_set_group_params", "mgx_planner_group_params", "mgx_plan_paths_groups", "mgx_plan_submit_groups")


def _prototypes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_sys
    finally:
        sys.path.pop(0)
    return {name: params for name, _, params in gen_rust_sys.c_prototypes()}


def test_the_binding_declares_the_new_functions_with_the_headers_arity():
    protos = _prototypes()
    for name in NEW:
        assert name in protos, name
        restype, argtypes = hostlib.SYMBOLS[name]
        assert len(argtypes) == len(protos[name]), name
    # the plain calls and their _groups forms differ by the one array of groups
    assert len(protos["mgx_plan_paths_groups"]) == len(protos["mgx_plan_paths"]) + 1
    assert len(protos["mgx_plan_submit_groups"]) == len(protos["mgx_plan_submit"]) + 1
    assert [t for t, n in protos["mgx_plan_submit_groups"] if n == "groups"] == ["const uint32_t *"]


def test_plan_done_carries_the_group():
    dt = hostlib.plan_done_dtype()
    assert dt.names == ("ticket", "slices", "group", "result") and dt.itemsize == 16 + hostlib.plan_result_dtype().itemsize
    assert dt.fields["group"][1] == 12
    header = open(os.path.join(ROOT, "include", "mgx.h"), encoding="utf-8").read()
    body = re.search(r"typedef struct mgx_plan_done \{(.*?)\} mgx_plan_done;", header, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == ["ticket", "slices", "group", "result"]


# ---- Ensemble validation against worlds that are none ----------------------------------------------------------------------------------
GP = os.path.join("tests", "golden", "scenario_files", "Collaborative GP")


def _scenario():
    return config.load_scenario(os.path.join(ROOT, GP))


class _NoWorld:
    """validation comes before the world is touched"""


class _Groups:
    """as much of an engine world as the validation looks at: robot groups, no planner"""

    def mission_tick_begin_groups(self, *a, **k):
        raise AssertionError("not reached")


class _Planner(_Groups):
    """... and the planner's calls, without a parameter set per group.  planner_enable is where validation has ended"""

    class Reached(Exception):
        pass

    def set_environment(self, env):
        pass

    def reserve(self, n):
        pass

    def collisions_enable(self, *a, **k):
        pass

    def tracks_enable(self, *a, **k):
        pass

    def mission_tick_begin(self, *a, **k):
        pass

    def planner_enable(self, env, params=None):
        raise self.Reached()

    def planner_set_tick_budget(self, n):
        pass

    def plan_submit(self, requests, groups=None):
        pass

    def plan_collect(self, **k):
        pass

    def apply_global_paths(self, *a, **k):
        pass


def _set(cfg, key, value):
    *path, last = key.split(".")
    for part in path:
        cfg = cfg[part]
    cfg[last] = value


@pytest.mark.parametrize("key", RRT_KEYS)
def test_rrt_differing_without_sets_per_group_names_the_key(key):
    a, b = _scenario(), _scenario()
    node = a["config"]["rrt"]
    for part in key.split("."):
        node = node[part]
    _set(b["config"]["rrt"], key, (not node) if isinstance(node, bool) else node + 1)
    with pytest.raises(ValueError, match=re.escape("rrt." + key)):
        Ensemble([a, b], _Planner(), global_planner="sliced")
    # the restatement plans every member under its own parameters: nothing is held once (validation is through, and stops at
    # the world that is none)
    with pytest.raises(NotImplementedError, match="robot groups"):
        Ensemble([copy.deepcopy(a), copy.deepcopy(b)], _NoWorld(), global_planner="host")
    # members that agree pass under "sliced" too, up to the world's planner
    with pytest.raises(_Planner.Reached):
        Ensemble([copy.deepcopy(a), copy.deepcopy(a)], _Planner(), global_planner="sliced")


def test_sliced_needs_a_world_with_the_planner_calls():
    with pytest.raises(NotImplementedError, match="needs an engine world that offers planner_enable"):
        Ensemble([_scenario()], _Groups(), global_planner="sliced")


def test_the_synchronous_planner_is_refused_and_points_to_sliced():
    with pytest.raises(NotImplementedError, match=r"global_planner=True.*slowest plan.*sliced"):
        Ensemble([_scenario()], _Planner(), global_planner=True)


def test_plan_budget_and_overrides_are_shared_options():
    with pytest.raises(ValueError, match="plan_budget"):
        Ensemble([_scenario()], _Planner(), global_planner="sliced", plan_budget=0)
    with pytest.raises(_Planner.Reached):
        Ensemble([_scenario()], _Planner(), global_planner="sliced", plan_budget=16, planner_overrides={"max_iterations": 100})


# ---- the runner's arguments ------------------------------------------------------------------------------------------------------------
def _runner(*args):
    r = subprocess.run([sys.executable, os.path.join("tools", "run_scenarios.py"), *args], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120)
    return r.returncode, r.stdout.decode()


@pytest.mark.parametrize("mode", [["device"], []], ids=["device", "no-mode"])
def test_runner_refuses_the_synchronous_planner_in_an_ensemble(mode):
    rc, out = _runner("--ensemble-seeds", "0,1", "--global-planner", *mode, GP)
    assert rc != 0 and "sliced" in out and "--global-planner" in out and "Traceback" not in out


def test_runner_arguments_of_the_radius_sweep():
    rc, out = _runner("--ensemble-rrt-collision-radii", "1.5,3", "--global-planner", "sliced", GP)
    assert rc != 0 and "--ensemble-seeds" in out and "Traceback" not in out
    rc, out = _runner("--ensemble-seeds", "0", "--ensemble-rrt-collision-radii", "1.5,3", GP)
    assert rc != 0 and "--global-planner sliced" in out and "Traceback" not in out
    rc, out = _runner("--ensemble-seeds", "0", "--ensemble-rrt-collision-radii", "-1", "--global-planner", "sliced", GP)
    assert rc != 0 and "--ensemble-rrt-collision-radii" in out and "Traceback" not in out
    rc, out = _runner("--ensemble-seeds", "0", "--global-planner", "host", "--host-trackers", GP)
    assert rc != 0 and "host trackers" in out and "Traceback" not in out
    # accepted as far as a machine without a device goes: one scenario must be named
    for mode in ("sliced", "host"):
        rc, out = _runner("--ensemble-seeds", "0,1", "--ensemble-rrt-collision-radii", "1.5,3", "--global-planner", mode)
        assert rc != 0 and "name it" in out and "Traceback" not in out
