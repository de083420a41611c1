"""Factor sigmas per robot group without a device (include/mgx.h, ROBOT GROUPS: mgx_set_group_sigmas, mgx_get_group_sigmas): the
argument checks through the library with a null world, in the stated order; the binding's set / get round trip against a
recording library; and what an Ensemble decides — on the pattern of tests/test_group_factors_host.py.  (A world needs a device, so
"a set equal to the world's is none" is checked on a real world in tests/test_gpu_groups_sigmas.py.)"""
import ctypes as C
import json
import math
import os

import pytest

from magics_amd import config, hostlib
from magics_amd.ensemble import SIGMAS, Ensemble, _shared_settings
from magics_amd.world import World

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1   # MGX_ERR_INVALID
GOOD = (0.1, 0.01, 0.01, 0.15)


def _sig(*v):
    return C.byref(hostlib.GroupSigmas(*v))


# ---- argument validation that needs no device: the struct, its values, the group; the null world last ---------------------------
@pytest.mark.parametrize("bad", [0.0, -0.0, -0.1, math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("field", range(4))
def test_every_sigma_must_be_finite_and_positive(bad, field):
    L = hostlib.lib()
    v = list(GOOD)
    v[field] = bad
    # (reported before the group and before the world: both are wrong here as well)
    assert L.mgx_set_group_sigmas(None, hostlib.GROUPS_MAX, _sig(*v)) == INVALID and b"finite and positive" in L.mgx_last_error()
    assert L.mgx_set_group_sigmas(None, 0, _sig(*v)) == INVALID and b"finite and positive" in L.mgx_last_error()


def test_group_sigmas_calls_check_their_arguments_first():
    L = hostlib.lib()
    assert L.mgx_set_group_sigmas(None, hostlib.GROUPS_MAX, None) == INVALID and b"null sigmas" in L.mgx_last_error()
    assert L.mgx_set_group_sigmas(None, 0, None) == INVALID and b"null sigmas" in L.mgx_last_error()
    assert L.mgx_set_group_sigmas(None, hostlib.GROUPS_MAX, _sig(*GOOD)) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    assert L.mgx_set_group_sigmas(None, 0xffffffff, _sig(*GOOD)) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    for tiny in (GOOD, (5e-324, 1e300, 1.0, 2.0 ** -30)):                 # all well, but for the world
        assert L.mgx_set_group_sigmas(None, hostlib.GROUPS_MAX - 1, _sig(*tiny)) == INVALID and b"null world" in L.mgx_last_error()
    out = hostlib.GroupSigmas(7.0, 7.0, 7.0, 7.0)
    assert L.mgx_get_group_sigmas(None, hostlib.GROUPS_MAX, C.byref(out)) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    assert L.mgx_get_group_sigmas(None, hostlib.GROUPS_MAX, None) == INVALID and b"MGX_GROUPS_MAX" in L.mgx_last_error()
    assert L.mgx_get_group_sigmas(None, 3, C.byref(out)) == INVALID and b"null" in L.mgx_last_error()
    assert L.mgx_get_group_sigmas(None, 3, None) == INVALID and b"null" in L.mgx_last_error()
    assert (out.dynamics, out.interrobot, out.obstacle, out.tracking) == (7.0, 7.0, 7.0, 7.0)


def test_the_signatures_are_bound():
    L = hostlib.lib()
    for name in ("mgx_set_group_sigmas", "mgx_get_group_sigmas"):
        assert getattr(L, name).restype is C.c_int
        assert list(getattr(L, name).argtypes[1:]) == [C.c_uint32, C.POINTER(hostlib.GroupSigmas)]
    assert C.sizeof(hostlib.GroupSigmas) == 32 and [f for f, _ in hostlib.GroupSigmas._fields_] == list(SIGMAS)
    for name in ("set_group_sigmas", "group_sigmas"):
        assert callable(getattr(World, name))


class _Recorder:
    """the library as World sees it: a world whose sigmas are 0.1 / 0.01 / 0.01 / 0.01, and a table of the groups' own"""
    WORLD = (0.1, 0.01, 0.01, 0.01)

    def __init__(self):
        self.own, self.calls = {}, []

    def mgx_set_group_sigmas(self, w, group, s):
        v = tuple(getattr(s._obj, k) for k in SIGMAS)
        self.calls.append(("set", group, v))
        self.own[group] = v
        return 0

    def mgx_get_group_sigmas(self, w, group, out):
        self.calls.append(("get", group))
        for k, x in zip(SIGMAS, self.own.get(group, self.WORLD)):
            setattr(out._obj, k, x)
        return 0


def test_the_binding_round_trip():
    import numpy as np
    w = World.__new__(World)
    w._L, w._w = _Recorder(), None
    w._chk = lambda rc: None if rc == 0 else (_ for _ in ()).throw(AssertionError(rc))
    assert w.group_sigmas(np.int64(2)) == dict(zip(SIGMAS, _Recorder.WORLD))          # never set: the world's
    w.set_group_sigmas(np.int64(2), tracking=np.float32(0.5))                          # one named: the others stay the group's
    assert w._L.calls[-1] == ("set", 2, (0.1, 0.01, 0.01, 0.5)) and type(w._L.calls[-1][1]) is int
    w.set_group_sigmas(2, dynamics=0.05)                                               # ... its own, once it has some
    assert w._L.calls[-1] == ("set", 2, (0.05, 0.01, 0.01, 0.5))
    assert w.group_sigmas(2) == {"dynamics": 0.05, "interrobot": 0.01, "obstacle": 0.01, "tracking": 0.5}
    w.set_group_sigmas(3, dynamics=1, interrobot=2, obstacle=3, tracking=4)
    assert w._L.calls[-1] == ("set", 3, (1.0, 2.0, 3.0, 4.0)) and all(type(x) is float for x in w._L.calls[-1][2])
    assert w.group_sigmas(0) == dict(zip(SIGMAS, _Recorder.WORLD))                     # other groups: untouched


# ---- Ensemble.__init__: the four sigmas are per member where the world offers the call ------------------------------------------
def _scenario(name="Structured Junction Twoway"):
    with open(os.path.join(HERE, "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


class _KindsWorld:
    """a world that takes a radius, a schedule and the enabled kinds per group, but no sigmas"""
    def mission_tick_begin_groups(self, *a, **k): raise AssertionError("not in __init__")
    neighbours_groups = env_collisions_enable = goal_areas_enable = track_metrics_enable = group_schedule_stats = mission_tick_begin_groups

    def __init__(self):
        self.masks, self.sigmas = [], []

    def set_group_enabled(self, group, mask):
        self.masks.append((group, mask))


class _SigmasWorld(_KindsWorld):
    """... and one that does: it records what it is given (validation comes before it is touched further)"""

    def set_group_sigmas(self, group, **sigmas):
        self.sigmas.append((group, sigmas))


def _differing(which, value=0.5):
    a, b = _scenario(), _scenario()
    b["config"]["gbp"]["sigma-factor-" + which] = config.f32(value)
    assert b["config"]["gbp"]["sigma-factor-" + which] != a["config"]["gbp"]["sigma-factor-" + which]
    return a, b


@pytest.mark.parametrize("which", SIGMAS)
def test_members_may_differ_in_every_sigma(which):
    a, b = _differing(which)
    w = _SigmasWorld()
    with pytest.raises((AttributeError, AssertionError, TypeError)):     # (the validation is through: it stops at the world that is a stub)
        Ensemble([a, b, a], w)
    own = {k: config.world_params(a["config"])["sigma_" + k] for k in SIGMAS}
    assert w.sigmas == [(0, own), (1, {**own, which: config.f32(0.5)}), (2, own)]   # every member's, before any robot is added
    assert w.masks == []                                                  # (the kinds agree: no masks)
    b["config"]["gbp"]["lookahead-multiple"] = 5                          # ... and everything else is still compared
    with pytest.raises(ValueError, match=r"gbp\.lookahead-multiple"):
        Ensemble([a, b], _SigmasWorld())


def test_members_that_agree_set_nothing():
    w = _SigmasWorld()
    with pytest.raises((AttributeError, AssertionError, TypeError)):
        Ensemble([_scenario(), _scenario()], w)
    assert w.sigmas == [] and w.masks == []                               # the world it was


@pytest.mark.parametrize("which", SIGMAS)
def test_a_world_without_the_call_holds_the_sigmas_once(which):
    w = _KindsWorld()
    with pytest.raises(ValueError, match=r"params\.sigma_" + which) as e:
        Ensemble(list(_differing(which)), w)
    assert "member 1" in str(e.value) and w.masks == []


def test_shared_settings_drop_the_sigmas_only_with_the_call():
    sc = _scenario()
    keys = {"params.sigma_" + k for k in SIGMAS}
    for kinds in (False, True):
        plain, per_group = dict(_shared_settings(sc, kinds)), dict(_shared_settings(sc, kinds, True))
        assert keys <= set(plain) and not keys & set(per_group)
        assert {k: v for k, v in plain.items() if k not in keys} == per_group
        assert [k for k, _ in _shared_settings(sc, kinds) if k not in keys] == [k for k, _ in _shared_settings(sc, kinds, True)]   # the order stays
    assert dict(_shared_settings(sc)) == dict(_shared_settings(sc, False, False))
