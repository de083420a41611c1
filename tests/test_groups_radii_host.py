"""The per-group comms radius without a device (include/mgx.h, ROBOT GROUPS): the threshold table of the grouped search
(group_tables + group_thresholds, magics_amd/csrc/mgx_search.h) in a stand-alone C++ program under the sanitizers —
tests/cpu_groups_radii/radii_harness.cpp, in the manner of tests/test_groups_host.py — the binding's handling of a scalar against
one radius per group, the argument checks of the radii calls, and what an Ensemble accepts now."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from magics_amd import hostlib
from magics_amd.ensemble import UNSUPPORTED, Ensemble
from magics_amd.world import group_radii

HERE = os.path.dirname(os.path.abspath(__file__))


def test_threshold_table_under_sanitizers(tmp_path):
    src = os.path.join(HERE, "cpu_groups_radii", "radii_harness.cpp")
    exe = str(tmp_path / "radii_harness")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    # the sanitizers' runtimes inside the program where the toolchain has them as archives (tests/test_search_host.py says why)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "radii harness: 0 failed checks" in out, out[-3000:]


# ---- the binding: a scalar is the scalar call, a sequence one radius per group ----------------------------------------------------
def test_a_scalar_radius_stays_the_scalar_call():
    for r in (5.0, np.float32(5.0), np.float64(2.5), 3, float("nan"), np.array(7.0)):
        assert group_radii(r, 4) is None


def test_one_radius_per_group_becomes_f32():
    got = group_radii([5.0, np.nextafter(np.float32(5), np.float32(0)), float("nan"), -1.0], 4)
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and got.shape == (4,)
    assert got[0] == 5.0 and got[1] < 5.0 and np.isnan(got[2]) and got[3] == -1.0
    assert group_radii(np.array([20.0, 40.0])[::-1], 2).tolist() == [40.0, 20.0]
    assert group_radii((8.0,), 1).tolist() == [8.0]


@pytest.mark.parametrize("radius, n_groups", [([5.0, 6.0], 3), ([5.0, 6.0, 7.0], 2), ([], 1), ([[1.0, 2.0]], 2), ([5.0], 0)])
def test_a_wrong_number_of_radii_is_refused(radius, n_groups):
    with pytest.raises(ValueError, match="per group"):
        group_radii(radius, n_groups)


# ---- argument validation that needs no device -----------------------------------------------------------------------------------
# (what needs a world's robots — a robot's group not below n_groups — runs on the device: tests/test_gpu_groups_radii_topology.py)
def test_radii_calls_check_their_arguments_first():
    L = hostlib.lib()
    pos = np.zeros((2, 3), np.float32)
    ok = np.ones(3, np.uint64)
    radii = np.array([2.0, 4.0, 8.0], np.float32)
    ptr = np.zeros(3, np.int32)

    def p(a):
        return None if a is None else a.ctypes.data

    def topo(n_groups, numbers, rad, method=0):
        return L.mgx_update_topology_groups_radii(None, p(pos), p(rad), method, n_groups, p(numbers), None)

    def tick(n_groups, numbers, rad, method=0):
        return L.mgx_mission_tick_begin_groups_radii(None, p(rad), method, n_groups, p(numbers), 1, None)
    for call in (topo, tick):
        assert call(3, None, radii) == -1 and b"number_next" in L.mgx_last_error()
        assert call(3, ok, None) == -1 and b"radii" in L.mgx_last_error()                 # null radii
        assert call(0, ok, radii) == -1 and b"n_groups" in L.mgx_last_error()
        assert call(hostlib.GROUPS_MAX + 1, ok, radii) == -1 and b"n_groups" in L.mgx_last_error()
        zero = np.array([1, 0, 1], np.uint64)
        assert call(3, zero, radii) == -1 and b"NonZeroUsize" in L.mgx_last_error()
        assert list(zero) == [1, 0, 1]
        assert call(3, ok, radii, method=9) == -1 and b"method" in L.mgx_last_error()
        assert call(3, ok, radii) == -1 and b"null" in L.mgx_last_error()                 # all well, but for the world
        assert list(ok) == [1, 1, 1] and radii.tolist() == [2.0, 4.0, 8.0]

    def search(n_groups, rad, method=0):
        return L.mgx_neighbours_groups(None, p(pos), p(rad), n_groups, method, p(ptr), None, 0, None)
    assert search(3, None) == -1 and b"radii" in L.mgx_last_error()
    assert search(0, radii) == -1 and b"n_groups" in L.mgx_last_error()
    assert search(hostlib.GROUPS_MAX + 1, radii) == -1 and b"n_groups" in L.mgx_last_error()
    assert search(3, radii, method=9) == -1 and b"method" in L.mgx_last_error()
    assert search(3, radii) == -1 and b"null" in L.mgx_last_error()
    nan = np.array([np.nan, -1.0, 0.0], np.float32)      # any value is a radius: the call gets as far as the world that is none
    assert search(3, nan) == -1 and b"null" in L.mgx_last_error()


def test_the_signatures_are_bound():
    L = hostlib.lib()
    for name in ("mgx_neighbours_groups", "mgx_update_topology_groups_radii", "mgx_mission_tick_begin_groups_radii"):
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes


# ---- Ensemble.__init__: what is per member now, what is still refused -----------------------------------------------------------
def _scenario(name="Varying Network Connectivity Experiment"):
    with open(os.path.join(HERE, "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


class _GroupsWorld:
    """a world that takes a radius per group and offers the device observers — validation comes before it is touched further"""
    def mission_tick_begin_groups(self, *a, **k): raise AssertionError("not in __init__")
    neighbours_groups = env_collisions_enable = goal_areas_enable = track_metrics_enable = mission_tick_begin_groups


def test_members_may_differ_in_comms_radius():
    a, b = _scenario(), _scenario()
    b["config"]["robot"]["communication"]["radius"] = 20.0
    assert a["config"]["robot"]["communication"]["radius"] != 20.0
    with pytest.raises((AttributeError, AssertionError, TypeError)):     # (the validation is through: it stops at the world that is a stub)
        Ensemble([a, b], _GroupsWorld())
    b["config"]["robot"]["target-speed"] = 1.25                            # ... and everything else is still compared
    with pytest.raises(ValueError, match=r"robot\.target-speed"):
        Ensemble([a, b], _GroupsWorld())


def test_only_the_global_planner_is_unsupported():
    assert UNSUPPORTED == ("global_planner",)
    with pytest.raises(NotImplementedError, match="global_planner"):
        Ensemble([_scenario()], _GroupsWorld(), global_planner=True)


@pytest.mark.parametrize("option, word", [({"environment_collisions": "host"}, "environment_collisions"), ({"goal_areas": "junction", "device_goal_areas": False}, "device_goal_areas"),
                                          ({"device_trackers": False}, "device_trackers")])
def test_options_that_need_the_transforms_on_the_host_say_so(option, word):
    with pytest.raises(NotImplementedError, match=word):
        Ensemble([_scenario()], _GroupsWorld(), **option)
