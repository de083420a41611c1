"""Robot groups without a device (include/mgx.h, ROBOT GROUPS): the host's tables of the grouped search (group_tables,
magics_amd/csrc/mgx_search.h) in a stand-alone C++ program under the sanitizers — tests/cpu_groups/groups_harness.cpp, in the
manner of tests/cpu_search — the validation of Ensemble.__init__, and the argument checks of the new entry points."""
import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from magics_amd import config, hostlib, scenarios
from magics_amd.ensemble import Ensemble

HERE = os.path.dirname(os.path.abspath(__file__))


def test_group_tables_under_sanitizers(tmp_path):
    src = os.path.join(HERE, "cpu_groups", "groups_harness.cpp")
    exe = str(tmp_path / "groups_harness")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    # the sanitizers' runtimes inside the program where the toolchain has them as archives (tests/test_search_host.py says why)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "groups harness: 0 failed checks" in out, out[-3000:]


# ---- Ensemble.__init__ ------------------------------------------------------------------------------------------------------------
def _scenario(name="Environment Obstacles Experiment"):
    with open(os.path.join(HERE, "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


class _NoWorld:
    """validation comes before the world is touched"""


def _differing(change):
    a, b = _scenario(), _scenario()
    change(b)
    return [a, b]


@pytest.mark.parametrize("key, change", [
    ("params.sigma_interrobot", lambda sc: sc["config"]["gbp"].__setitem__("sigma-factor-interrobot", 0.123)),
    ("params.sigma_dynamics", lambda sc: sc["config"]["gbp"].__setitem__("sigma-factor-dynamics", 0.5)),
    ("gbp.iteration-schedule", lambda sc: sc["config"]["gbp"]["iteration-schedule"].__setitem__("internal", 7)),
    ("robot.communication.radius", lambda sc: sc["config"]["robot"]["communication"].__setitem__("radius", 12.5)),
    ("robot.target-speed", lambda sc: sc["config"]["robot"].__setitem__("target-speed", 1.25)),
    ("simulation.hz", lambda sc: sc["config"]["simulation"].__setitem__("hz", 20.0)),
    ("environment", lambda sc: sc["environment"]["tiles"]["settings"].__setitem__("tile-size", 51.0)),
])
def test_what_the_world_holds_once_must_be_equal(key, change):
    scs = _differing(change)
    assert scs[0] != scs[1]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")) as e:
        Ensemble(scs, _NoWorld())
    assert "member 1" in str(e.value)


def test_members_may_differ_in_seed_failure_rate_and_formation():
    def change(sc):
        sc["config"]["simulation"]["prng-seed"] = 7
        sc["config"]["robot"]["communication"]["failure-rate"] = 0.4
        sc["formation"]["formations"][0]["robots"] = 3
    with pytest.raises(NotImplementedError, match="engine world"):   # (the validation is through: it stops at the world that is none)
        Ensemble(_differing(change), _NoWorld())


@pytest.mark.parametrize("option", [{"environment_collisions": True}, {"goal_areas": "junction"}, {"device_metrics": True}, {"global_planner": True}])
def test_unsupported_options_say_so(option):
    with pytest.raises(NotImplementedError, match=next(iter(option))):
        Ensemble([_scenario()], _NoWorld(), **option)


def test_rrt_star_formations_say_so():
    sc = _scenario()
    sc["formation"]["formations"][0]["planning-strategy"] = "rrt-star"
    with pytest.raises(NotImplementedError, match="rrt-star"):
        Ensemble([_scenario(), sc], _NoWorld())


def test_an_ensemble_needs_members():
    with pytest.raises(ValueError):
        Ensemble([], _NoWorld())


# ---- argument validation that needs no device ------------------------------------------------------------------------------------
# (no device, no world: mgx_world_create needs one.  What the arguments alone say is checked in front of the world — below; what
# needs a world's robots — a robot's group not below n_groups, ghosts and groups in one world — runs on the device:
# tests/test_gpu_groups_topology.py::test_arguments_that_need_a_world)
def _desc(group, ghost=0):
    mean0, prior, dt = scenarios.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), scenarios.timesteps_for_K(10), 1.0, 5.0, 5.0)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (mean0, prior, dt)]
    d = hostlib.RobotDesc()
    d.K = len(keep[1])
    d.mean0, d.prior_diag, d.dt = (a.ctypes.data_as(hostlib.c_double_p) for a in keep)
    d.radius, d.order_key, d.ghost, d.group = 1.0, 0, ghost, group
    return d, keep


def test_a_group_id_has_to_be_below_groups_max():
    L = hostlib.lib()
    d, _keep = _desc(hostlib.GROUPS_MAX)
    assert L.mgx_robot_add(None, C.byref(d), None) == -1 and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    d, _keep = _desc(2 ** 32 - 1)
    assert L.mgx_robot_add(None, C.byref(d), None) == -1 and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    d, _keep = _desc(hostlib.GROUPS_MAX - 1)      # in range: the call gets as far as the world that is none
    assert L.mgx_robot_add(None, C.byref(d), None) == -1 and b"null" in L.mgx_last_error()
    d, _keep = _desc(3, ghost=1)
    assert L.mgx_robot_add(None, C.byref(d), None) == -1 and b"ghost" in L.mgx_last_error()


def test_per_group_calls_check_their_arguments_first():
    L = hostlib.lib()
    pos = np.zeros((2, 3), np.float32)
    ok = np.ones(3, np.uint64)

    def topo(n_groups, numbers):
        return L.mgx_update_topology_groups(None, pos.ctypes.data, 5.0, 0, n_groups, None if numbers is None else numbers.ctypes.data, None)

    def tick(n_groups, numbers):
        return L.mgx_mission_tick_begin_groups(None, 5.0, 0, n_groups, None if numbers is None else numbers.ctypes.data, 1, None)
    for call in (topo, tick):
        assert call(3, None) == -1 and b"number_next" in L.mgx_last_error()             # a null number_next
        assert call(0, ok) == -1 and b"n_groups" in L.mgx_last_error()
        assert call(hostlib.GROUPS_MAX + 1, ok) == -1 and b"n_groups" in L.mgx_last_error()
        zero = np.array([1, 0, 1], np.uint64)
        assert call(3, zero) == -1 and b"NonZeroUsize" in L.mgx_last_error()            # a zero generator
        assert list(zero) == [1, 0, 1]
        assert call(3, ok) == -1 and b"null" in L.mgx_last_error()                      # all well, but for the world
    assert L.mgx_update_topology_groups(None, pos.ctypes.data, 5.0, 9, 3, ok.ctypes.data, None) == -1 and b"method" in L.mgx_last_error()


def test_world_params_are_what_an_ensemble_compares():
    sc = _scenario()
    assert set(config.world_params(sc["config"])) >= {"sigma_dynamics", "sigma_interrobot", "sigma_obstacle", "sigma_tracking", "enable_mask"}
    assert copy.deepcopy(sc) == sc
