"""Enabled factor kinds per robot group without a device (include/mgx.h, ROBOT GROUPS: mgx_set_group_enabled,
mgx_get_group_enabled, mgx_group_enabled_stats): the argument checks of the new calls through the library with a null world, in
the stated order; the binding; and what an Ensemble accepts now — on the pattern of tests/test_group_schedules_host.py.  (The
per-robot counters read the robot's mask where they read the world's: no host helper of its own, so no stand-alone program here;
tests/test_gpu_groups_factors.py compares every robot's message counts with a world of its own.)"""
import ctypes as C
import json
import os

import pytest

from magics_amd import config, hostlib
from magics_amd.ensemble import Ensemble, _shared_settings
from magics_amd.world import World

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1   # MGX_ERR_INVALID


# ---- argument validation that needs no device: unknown kind bits, then the group, the null world (or out-pointer) last --------
def test_group_enabled_calls_check_their_arguments_first():
    L = hostlib.lib()
    out = C.c_uint32(77)
    assert L.mgx_set_group_enabled(None, hostlib.GROUPS_MAX, 16) == INVALID and b"unknown factor kind" in L.mgx_last_error()
    assert L.mgx_set_group_enabled(None, 0, 0xffffffff) == INVALID and b"unknown factor kind" in L.mgx_last_error()
    assert L.mgx_set_group_enabled(None, hostlib.GROUPS_MAX, 15) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    assert L.mgx_set_group_enabled(None, 0xffffffff, 0) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    for mask in (0, 7, 13, 15):
        assert L.mgx_set_group_enabled(None, hostlib.GROUPS_MAX - 1, mask) == INVALID and b"null" in L.mgx_last_error()   # all well, but for the world
    assert L.mgx_get_group_enabled(None, hostlib.GROUPS_MAX, C.byref(out)) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    assert L.mgx_get_group_enabled(None, hostlib.GROUPS_MAX, None) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    assert L.mgx_get_group_enabled(None, 3, C.byref(out)) == INVALID and b"null" in L.mgx_last_error()
    assert L.mgx_get_group_enabled(None, 3, None) == INVALID and b"null" in L.mgx_last_error()
    assert out.value == 77
    assert L.mgx_group_enabled_stats(None, None, None) == INVALID and b"null" in L.mgx_last_error()


def test_the_signatures_are_bound():
    L = hostlib.lib()
    for name in ("mgx_set_group_enabled", "mgx_get_group_enabled", "mgx_group_enabled_stats"):
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes
    assert list(L.mgx_set_group_enabled.argtypes[1:]) == [C.c_uint32, C.c_uint32]
    for name in ("set_group_enabled", "group_enabled", "group_enabled_stats"):
        assert callable(getattr(World, name))


class _Recorder:
    """the library as World sees it, for the binding's argument conversion: records the call, fills the out-pointers"""

    def __init__(self):
        self.calls = []

    def mgx_set_group_enabled(self, w, group, mask):
        self.calls.append(("set", group, mask))
        return 0

    def mgx_get_group_enabled(self, w, group, out):
        self.calls.append(("get", group))
        out._obj.value = 11
        return 0

    def mgx_group_enabled_stats(self, w, a, b):
        a._obj.value, b._obj.value = 2 ** 40, 3
        return 0


def test_the_binding_converts_its_arguments():
    import numpy as np
    w = World.__new__(World)
    w._L, w._w = _Recorder(), None
    w._chk = lambda rc: None if rc == 0 else (_ for _ in ()).throw(AssertionError(rc))
    w.set_group_enabled(np.int64(3), np.uint8(7))
    w.set_group_enabled(4, True | 4)
    assert w._L.calls == [("set", 3, 7), ("set", 4, 5)] and all(type(x) is int for c in w._L.calls for x in c[1:])
    assert w.group_enabled(np.uint32(9)) == 11 and w._L.calls[-1] == ("get", 9)
    assert w.group_enabled_stats() == (2 ** 40, 3)


# ---- Ensemble.__init__: dynamic, obstacle and tracking are per member where the world offers the call ---------------------------
def _scenario(name="Structured Junction Twoway"):
    with open(os.path.join(HERE, "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


class _SchedulesWorld:
    """a world that takes a radius and a schedule per group and offers the device observers, but no enabled kinds per group"""
    def mission_tick_begin_groups(self, *a, **k): raise AssertionError("not in __init__")
    neighbours_groups = env_collisions_enable = goal_areas_enable = track_metrics_enable = group_schedule_stats = mission_tick_begin_groups


class _KindsWorld(_SchedulesWorld):
    """... and one that does: it records the masks it is given (validation comes before it is touched further)"""

    def __init__(self):
        self.masks = []

    def set_group_enabled(self, group, mask):
        self.masks.append((group, mask))


def _differing(kind):
    a, b = _scenario(), _scenario()
    b["config"]["gbp"]["factors-enabled"][kind] = not a["config"]["gbp"]["factors-enabled"][kind]
    return a, b


@pytest.mark.parametrize("kind,bit", [("dynamic", 1), ("obstacle", 4), ("tracking", 8)])
def test_members_may_differ_in_the_internal_kinds(kind, bit):
    a, b = _differing(kind)
    w = _KindsWorld()
    with pytest.raises((AttributeError, AssertionError, TypeError)):     # (the validation is through: it stops at the world that is a stub)
        Ensemble([a, b, a], w)
    assert w.masks == [(0, 15), (1, 15 & ~bit), (2, 15)]                  # every member's mask, before any robot is added
    b["config"]["gbp"]["lookahead-multiple"] = 5                          # ... and everything else is still compared
    with pytest.raises(ValueError, match=r"gbp\.lookahead-multiple"):
        Ensemble([a, b], _KindsWorld())


def test_members_that_agree_set_no_masks():
    w = _KindsWorld()
    with pytest.raises((AttributeError, AssertionError, TypeError)):
        Ensemble([_scenario(), _scenario()], w)
    assert w.masks == []                                                  # the unmasked world it was


def test_the_interrobot_kind_stays_the_worlds():
    w = _KindsWorld()
    with pytest.raises(ValueError, match=r"gbp\.factors-enabled\.interrobot") as e:
        Ensemble(list(_differing("interrobot")), w)
    assert "member 1" in str(e.value) and w.masks == []


@pytest.mark.parametrize("kind", ["dynamic", "interrobot", "obstacle", "tracking"])
def test_a_world_without_the_call_holds_the_whole_mask_once(kind):
    with pytest.raises(ValueError, match=r"params\.enable_mask") as e:
        Ensemble(list(_differing(kind)), _SchedulesWorld())
    assert "member 1" in str(e.value)


def test_shared_settings_name_the_interrobot_kind_only_with_the_call():
    sc = _scenario()
    plain, per_group = dict(_shared_settings(sc)), dict(_shared_settings(sc, True))
    assert plain["params.enable_mask"] == config.enable_mask(sc["config"]) == 15 and "gbp.factors-enabled.interrobot" not in plain
    assert "params.enable_mask" not in per_group and per_group["gbp.factors-enabled.interrobot"] is True
    assert {k: v for k, v in plain.items() if k != "params.enable_mask"} == {k: v for k, v in per_group.items() if k != "gbp.factors-enabled.interrobot"}
