"""One GBP iteration schedule per robot group without a device (include/mgx.h, ROBOT GROUPS: mgx_iterate_groups,
mgx_mission_tick_end_groups): the plan arithmetic (plan_group_launches, group_steps_equal, group_steps_check:
magics_amd/csrc/mgx_resident.h) in a stand-alone C++ program under the sanitizers — tests/cpu_group_schedules/plan_harness.cpp, built
as tests/test_groups_radii_host.py builds its harness — the binding's packing of one schedule against one per group, the argument
checks of the new calls through the library with a null world, and what an Ensemble accepts now."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from magics_amd import hostlib
from magics_amd.ensemble import Ensemble
from magics_amd.world import group_steps

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1   # MGX_ERR_INVALID
I, E, IE = hostlib.STEP_INTERNAL, hostlib.STEP_EXTERNAL, hostlib.STEP_INTERNAL | hostlib.STEP_EXTERNAL


def test_plan_arithmetic_under_sanitizers(tmp_path):
    src = os.path.join(HERE, "cpu_group_schedules", "plan_harness.cpp")
    exe = str(tmp_path / "plan_harness")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    # the sanitizers' runtimes inside the program where the toolchain has them as archives (tests/test_search_host.py says why)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "group plan harness: 0 failed checks" in out, out[-3000:]


# ---- the binding: one schedule is the plain call, a sequence of schedules one per group ------------------------------------------
def test_one_schedule_stays_the_plain_call():
    for steps in ([IE, I, IE], (I, E), b"\x03\x01", bytearray(b"\x01"), np.array([IE, IE], np.uint8), [], hostlib.schedule(hostlib.SCHEDULE_CENTERED, 5, 2),
                  [np.uint8(1), np.int64(3)]):
        assert group_steps(steps) is None


def test_one_schedule_per_group_is_packed():
    steps, first = group_steps([[IE, I, IE], [], (E, E, IE, E), b"\x01\x01", np.array([IE], np.uint8)])
    assert steps == bytes([IE, I, IE, E, E, IE, E, I, I, IE])
    assert first.dtype == np.uint32 and first.flags["C_CONTIGUOUS"] and first.tolist() == [0, 3, 3, 7, 9, 10]
    steps, first = group_steps([[I]])                      # one group is a sequence of one schedule
    assert steps == bytes([I]) and first.tolist() == [0, 1]
    steps, first = group_steps([[], []])                   # nobody runs anything
    assert steps == b"" and first.tolist() == [0, 0, 0]


@pytest.mark.parametrize("steps", [[IE, [I]], [[I], IE], [[[I]]], [[I, [E]]]])
def test_a_sequence_that_is_neither_is_refused(steps):
    with pytest.raises(ValueError, match="per group"):
        group_steps(steps)


# ---- argument validation that needs no device: every MGX_ERR_INVALID case the arrays alone decide, the null world last ------------
def test_group_schedule_calls_check_their_arguments_first():
    L = hostlib.lib()
    good = bytes([IE, I, E])
    first = np.array([0, 2, 2, 3], np.uint32)

    def p(a):
        return None if a is None else a.ctypes.data

    def iterate(n_groups, steps, step_first):
        return L.mgx_iterate_groups(None, n_groups, steps, p(step_first))

    def tick_end(n_groups, steps, step_first):
        return L.mgx_mission_tick_end_groups(None, None, 1.0, 0.1, n_groups, steps, p(step_first))
    for call in (iterate, tick_end):
        assert call(3, good, None) == INVALID and b"step_first" in L.mgx_last_error()
        assert call(0, good, first) == INVALID and b"n_groups" in L.mgx_last_error()
        assert call(hostlib.GROUPS_MAX + 1, good, first) == INVALID and b"n_groups" in L.mgx_last_error()
        assert call(3, None, first) == INVALID and b"steps" in L.mgx_last_error()             # null steps with steps to read
        assert call(3, bytes([IE, 4, E]), first) == INVALID and b"bad step 1" in L.mgx_last_error()     # the byte's index is named
        assert call(3, bytes([IE, I, 128]), first) == INVALID and b"bad step 2" in L.mgx_last_error()
        assert call(3, good, np.array([1, 2, 2, 3], np.uint32)) == INVALID and b"ascend" in L.mgx_last_error()   # not from 0
        assert call(3, good, np.array([0, 2, 1, 3], np.uint32)) == INVALID and b"ascend" in L.mgx_last_error()   # descends
        assert call(3, good, first) == INVALID and b"null" in L.mgx_last_error()              # all well, but for the world
        assert call(2, None, np.zeros(3, np.uint32)) == INVALID and b"null" in L.mgx_last_error()  # (no steps to read: null steps are fine)
        assert first.tolist() == [0, 2, 2, 3]
    assert L.mgx_group_schedule_stats(None, None, None, None) == INVALID and b"null" in L.mgx_last_error()


def test_the_signatures_are_bound():
    L = hostlib.lib()
    for name in ("mgx_iterate_groups", "mgx_mission_tick_end_groups", "mgx_group_schedule_stats"):
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes


# ---- Ensemble.__init__: the iteration schedule is per member where the world offers the call ------------------------------------
def _scenario(name="Iteration Amount Experiment"):
    with open(os.path.join(HERE, "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


class _GroupsWorld:
    """a world that takes a radius per group and offers the device observers, but no schedule per group"""
    def mission_tick_begin_groups(self, *a, **k): raise AssertionError("not in __init__")
    neighbours_groups = env_collisions_enable = goal_areas_enable = track_metrics_enable = mission_tick_begin_groups


class _SchedulesWorld(_GroupsWorld):
    """... and one that does (validation comes before it is touched further)"""
    group_schedule_stats = _GroupsWorld.mission_tick_begin_groups


def _differing():
    a, b = _scenario(), _scenario()
    b["config"]["gbp"]["iteration-schedule"].update({"internal": 1, "external": 34, "schedule": "centered"})
    assert a["config"]["gbp"]["iteration-schedule"] != b["config"]["gbp"]["iteration-schedule"]
    return a, b


def test_members_may_differ_in_iteration_schedule():
    a, b = _differing()
    with pytest.raises((AttributeError, AssertionError, TypeError)):     # (the validation is through: it stops at the world that is a stub)
        Ensemble([a, b], _SchedulesWorld())
    b["config"]["gbp"]["lookahead-multiple"] = 5                          # ... and everything else is still compared
    with pytest.raises(ValueError, match=r"gbp\.lookahead-multiple"):
        Ensemble([a, b], _SchedulesWorld())


def test_a_world_without_the_call_names_the_key():
    with pytest.raises(ValueError, match=r"gbp\.iteration-schedule") as e:
        Ensemble(list(_differing()), _GroupsWorld())
    assert "member 1" in str(e.value)
