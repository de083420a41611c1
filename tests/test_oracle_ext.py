"""The checker of the two run-time mutators (tests/cpu_oracle_ext/oracle_ext.c through tests/oracle_ext.py): the extended
library is the stock oracle until one of the new functions is called, and each of them has a known answer —
update_inter_robot_safety_distance_multiplier (factorgraph.rs:892-910, interrobot.rs:87-89,213-226) and
set_tracking_path (tracking.rs:134-136,373-379).  Plus the argument errors of the engine's two entry points that need no
device."""
import ctypes as C

import numpy as np

import oracle
from magics_amd import hostlib, scenarios as S
from oracle_ext import ExtOracleWorld

WHITE = np.full((8, 8, 3), 255, np.uint8)


def test_extended_library_is_the_stock_oracle_until_called():
    """4 robots x K = 10, inter-robot + tracking factors, 3 ticks: bit for bit"""
    sc = S.grid_scenario(4, 10, interrobot=True, tracking=True, pitch=2.0, comm_radius=5.0)
    worlds = oracle.OracleWorld(sc["params"]), ExtOracleWorld(sc["params"])
    tick = S.tick_inputs(sc)
    for w in worlds:
        S.populate(w, sc)
    for t in range(3):
        for w in worlds:
            w.tick(steps=sc["steps"], **tick)
        for name, a, b in zip(("eta", "lam", "mean"), *(w.read_beliefs() for w in worlds)):
            assert np.array_equal(a, b, equal_nan=True), f"tick {t}: {name} differs from the stock oracle"
        assert [worlds[0].message_counts(r) for r in range(4)] == [worlds[1].message_counts(r) for r in range(4)]


def _pair_world(multiplier, gap=3.0, K=4, connect=True):
    """two robots of radius 1 whose variables i lie exactly `gap` apart"""
    params = dict(S.JUNCTION_PARAMS, enable_mask=S.EN_DYN | S.EN_IR, safety_multiplier=multiplier)
    w = ExtOracleWorld(params)
    w.set_sdf(WHITE, 100.0, 100.0)
    prior = np.full(K, np.inf)
    prior[0] = prior[-1] = 1e30
    ids = []
    for k in range(2):
        mean0 = np.tile(np.array([gap * k, 0.0, 0.3, -0.2]), (K, 1)) + np.arange(K)[:, None] * 0.01
        ids.append(w.add_robot(mean0, prior, np.full(K - 1, 0.1), 1.0, order_key=k))
    if connect:
        w.ir_connect(ids[0], ids[1], 1)
        w.ir_connect(ids[1], ids[0], 1 + (K - 1))
    return w, ids


def _foreign_present(w, ids, K=4):
    """per (robot, variable 1..K-1): is the message of the other robot's inter-robot factor a message (not empty)?"""
    out = []
    for r, o in ((0, 1), (1, 0)):
        for i in range(1, K):
            foreign = [b for b in w.variable_inbox(ids[r], i) if b[0] == ids[o]]
            assert len(foreign) == 1
            out.append(foreign[0][2])
    return out


def test_multiplier_known_answer():
    """radius 1, variables 3 apart: 2.5 * 1 < 3 < 4 * 1 — skipped (the empty message) under 2.5, evaluated under 4"""
    w, ids = _pair_world(2.5)
    w.iterate([3, 3, 3])
    assert not any(_foreign_present(w, ids))
    w.set_safety_multiplier(4.0)
    w.iterate([3])
    assert all(_foreign_present(w, ids))
    w.set_safety_multiplier(2.5)  # and back: the same factors skip again
    w.iterate([3])
    assert not any(_foreign_present(w, ids))


def test_connection_made_after_the_call_carries_the_new_distance():
    w, ids = _pair_world(2.5, connect=False)
    w.iterate([1, 1])
    w.set_safety_multiplier(4.0)  # (the config entry: ui/settings.rs:586-590 writes it before it walks the graphs)
    w.ir_connect(ids[0], ids[1], 1)
    w.ir_connect(ids[1], ids[0], 4)
    w.iterate([3, 3])
    assert all(_foreign_present(w, ids))
    ctl, cids = _pair_world(2.5, connect=False)  # control: without the call the same connections skip
    ctl.iterate([1, 1])
    ctl.ir_connect(cids[0], cids[1], 1)
    ctl.ir_connect(cids[1], cids[0], 4)
    ctl.iterate([3, 3])
    assert not any(_foreign_present(ctl, cids))


def test_multiplier_must_be_strictly_positive_and_finite():
    w, ids = _pair_world(2.5, connect=False)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert w._L.orc_set_safety_multiplier(w._w, bad) < 0
    # nothing changed: a connection made now still carries 2.5 * 1 < 3 and skips
    w.ir_connect(ids[0], ids[1], 1)
    w.ir_connect(ids[1], ids[0], 4)
    w.iterate([3, 3])
    assert not any(_foreign_present(w, ids))


K = 10


def _tracking_world(path):
    """one robot heading along +x, tracking factors on variables 1 .. K-2; returns the world and its initial means"""
    params = dict(S.JUNCTION_PARAMS, enable_mask=S.EN_DYN | S.EN_TRK)
    w = ExtOracleWorld(params)
    w.set_sdf(WHITE, 100.0, 100.0)
    ts = S.timesteps_for_K(K)
    mean0, prior, dt = S.robot_initial_state((0.0, 0.0, 5.0, 0.0), (1000.0, 0.0, 5.0, 0.0), ts, 1.0, 5.0, S.HORIZON_FOR_K[K] / 5.0)
    w.add_robot(mean0, prior, dt, 1.0, path=path)
    return w, mean0


def _tracking_present(w):
    """per variable 1 .. K-2: is the message of its tracking factor (node K + (K-1) + (K-2) + i-1) a message?"""
    first = K + (K - 1) + (K - 2)
    out = []
    for i in range(1, K - 1):
        mine = [b for b in w.variable_inbox(0, i) if b[0] == 0 and b[1] == first + i - 1]
        assert len(mine) == 1
        out.append(mine[0][2])
    return out


def _corner_path():
    """a corner half a metre beyond variable K-2: that variable's factor (and only it) comes within the switch padding of
    the first segment's end, so its record advances to 1 (tracking.rs:294-296)"""
    _, mean0 = _tracking_world(None)
    corner = float(mean0[K - 2, 0]) + 0.5
    assert corner - float(mean0[K - 3, 0]) > 2.0  # (the next factor stays well outside the padding of 1)
    return np.array([(0.0, 0.0), (corner, 0.0), (corner, 20.0)], dtype=np.float32)


def test_factor_whose_record_advanced_is_skipped_under_a_two_point_path():
    path3 = _corner_path()
    w, _ = _tracking_world(path3)
    ctl, _ = _tracking_world(path3)
    for x in (w, ctl):
        x.iterate([1] * 12)  # (tracking factors sit out the graph's first ten factor iterations, factorgraph.rs:701)
        assert all(_tracking_present(x))
    w.set_tracking_path(0, path3[:2])  # record 1 >= n_path - 1 = 1: skipped from now on (tracking.rs:373-379); record 0 goes on
    for x in (w, ctl):
        x.iterate([1])
    assert _tracking_present(w) == [True] * (K - 3) + [False]
    assert all(_tracking_present(ctl))
    # ... and the record was kept, not reset: the three-point path again, and the factor is back on its second segment
    w.set_tracking_path(0, path3)
    w.iterate([1])
    assert all(_tracking_present(w))


def test_robot_without_a_path_starts_tracking():
    w, _ = _tracking_world(None)
    w.iterate([1] * 12)
    assert not any(_tracking_present(w))
    w.set_tracking_path(0, _corner_path())
    w.iterate([1])
    assert all(_tracking_present(w))


def test_path_arguments():
    w, _ = _tracking_world(None)
    p = np.zeros((3, 2), np.float32)
    assert w._L.orc_set_tracking_path(w._w, 0, p.ctypes.data, 1) < 0
    assert w._L.orc_set_tracking_path(w._w, 0, None, 3) < 0
    assert w._L.orc_set_tracking_path(w._w, 1, p.ctypes.data, 3) < 0
    assert w._L.orc_set_tracking_path(w._w, -1, p.ctypes.data, 3) < 0


def test_engine_argument_errors_need_no_device():
    """what the two entry points refuse before they look at a device (tests/test_abi.py: a machine without a GPU has no
    world to hand them, so the world is null throughout and each call names the first thing wrong with it)"""
    L = hostlib.lib()
    for bad in (0.0, -2.2, float("inf"), float("-inf"), float("nan")):
        assert L.mgx_set_safety_multiplier(None, bad) == -1
        assert b"finite and > 0" in L.mgx_last_error()
    assert L.mgx_set_safety_multiplier(None, 2.2) == -1
    assert b"null world" in L.mgx_last_error()
    p = (C.c_float * 6)()
    for n in (0, 1):
        assert L.mgx_set_tracking_path(None, 0, p, n) == -1
        assert b"n_path" in L.mgx_last_error()
    assert L.mgx_set_tracking_path(None, 0, None, 3) == -1
    assert b"null path" in L.mgx_last_error()
    for robot in (0, -1):
        assert L.mgx_set_tracking_path(None, robot, p, 3) == -1
        assert b"bad robot" in L.mgx_last_error()
