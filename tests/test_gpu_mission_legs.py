"""Missions of several legs on the device (include/mgx.h, MISSIONS OF SEVERAL LEGS): `DeviceDriver(legs=...)` on the engine
against `Driver(legs=...)` on the CPU oracle, tick by tick and bit for bit — who ended a leg, who completed, the idle flags, the
Transforms, every belief, the message counters and the legs the device has left; what a robot between two legs does and does not
do; mgx_mission_run, which stops behind every tick in which a leg ended; the same script without lingering launches; and worlds
without legs, which see none of it.  The scenario and the script of hand-overs: tests/mission_legs_common.py (three robots — two
legs, three legs, a plain route — and a mirrored pair of which, in one and the same tick, one ends a leg and the other completes)."""
import functools

import numpy as np
import pytest

from magics_amd import World, scenarios as S
from magics_amd.driver import DeviceDriver, Driver
from magics_amd.hostlib import MgxError
from mission_legs_common import K, LEGS, PLANNING_HORIZON, driver_kwargs, leg_path, legs_scenario, Script
from oracle_ext import ExtOracleWorld

pytestmark = pytest.mark.gpu

TICKS = 60


def _oracle_run(ticks, legs):
    sc, n = legs_scenario(pair=True)
    ref = ExtOracleWorld(sc["params"])
    S.populate(ref, sc)
    dr = Driver(ref, n, K, **driver_kwargs(sc, n, legs=legs))
    script, rec = Script(), []
    for tick in range(ticks):
        script.hand_over(tick, dr)
        before = dr.finished_at.copy()
        events = dr.tick()
        script.ended(tick, dr.legs_ended)
        rec.append(dict(events=tuple(int(x) for x in events), legs_ended=list(dr.legs_ended),
                        completed=[r for r in range(n) if before[r] < 0 <= dr.finished_at[r]], idle=dr.idle.copy(),
                        translation=dr.translation.copy(), finished_at=dr.finished_at.copy(), legs_left=dr.legs_left.copy(),
                        beliefs=[b.copy() for b in ref.read_beliefs()], messages=[ref.message_counts(r) for r in range(n)]))
    handed = {}
    for tick, r, k in script.handed:
        handed.setdefault(tick, []).append((r, k))
    return sc, n, rec, handed


@functools.lru_cache(maxsize=None)
def reference():
    """the oracle's run of the script, made once and only read: per tick what the engine must equal, and who was handed which leg
    before which tick"""
    return _oracle_run(TICKS, True)


def _engine(sc, n, **kw):
    eng = World(sc["params"])
    S.populate(eng, sc)
    return eng, DeviceDriver(eng, n, K, **driver_kwargs(sc, n, **kw))


def _hand_over(de, handed, tick):
    for r, k in handed.get(tick, []):
        de.global_path(r, leg_path(r, k), PLANNING_HORIZON)


def _same_state(eng, de, want, what):
    tr, _, fin = de.state()
    assert np.array_equal(tr, want["translation"]), what
    assert np.array_equal(fin, want["finished_at"]), what
    alive = want["finished_at"] < 0  # (a completed robot is despawned: its flags mean nothing any more)
    assert np.array_equal(eng.idle_flags()[alive], want["idle"][alive]), what
    assert np.array_equal(eng.mission_legs_read(), want["legs_left"]), what
    for name, a, b in zip(("eta", "lam", "mean"), eng.read_beliefs(), want["beliefs"]):
        assert np.array_equal(a, b, equal_nan=True), (what, name)
    assert [eng.message_counts(r) for r in range(de.n)] == want["messages"], what


def _run_script(eng, de, rec, handed, every=1):
    for tick, want in enumerate(rec):
        _hand_over(de, handed, tick)
        assert tuple(int(x) for x in de.tick()) == want["events"], tick
        assert de.legs_ended == want["legs_ended"] and de.completed == want["completed"], (tick, de.legs_ended, de.completed)
        if tick % every == every - 1 or tick == len(rec) - 1:
            _same_state(eng, de, want, f"tick {tick}")


def test_the_script_runs_every_leg_and_the_pair_shares_a_tick():
    """conditions of the tests below, on the oracle's run: every leg is run to its end, and robots 3 and 4 — one ends a leg, the
    other completes — do so in the same tick, so that both kinds of event are in one list"""
    _, n, rec, handed = reference()
    assert sorted(x for xs in handed.values() for x in xs) == [(0, 1), (1, 1), (1, 2), (3, 1)]
    assert (rec[-1]["finished_at"] >= 0).all() and rec[-1]["legs_left"].tolist() == [0] * n
    both = [t for t, x in enumerate(rec) if 3 in x["legs_ended"] and 4 in x["completed"]]
    assert len(both) == 1
    assert np.isfinite(rec[-1]["beliefs"][2]).all()


def test_device_driver_with_legs_equals_the_oracle_tick_by_tick():
    sc, n, rec, handed = reference()
    eng, de = _engine(sc, n, legs=LEGS[:n])
    _run_script(eng, de, rec, handed)


def test_without_lingering_launches_the_results_are_the_same():
    sc, n, rec, handed = reference()
    eng, de = _engine(sc, n, legs=LEGS[:n])
    eng.set_linger(0)
    _run_script(eng, de, rec, handed, every=10)


def test_what_a_robot_between_two_legs_does_and_does_not_do():
    sc, n, rec, handed = reference()
    eng, de = _engine(sc, n, legs=LEGS[:n])
    t_pair = next(t for t, x in enumerate(rec) if 3 in x["legs_ended"])
    t_path = next(t for t, xs in handed.items() if (3, 1) in xs)
    assert t_path - t_pair >= 3  # (it waits for two whole ticks)
    nfin = None
    for tick in range(t_pair + 1):
        _hand_over(de, handed, tick)
        de.next_number, _, _, nfin = eng.mission_tick(de.comms_radius, de.next_number, de.steps, de.max_speed, de.delta_t, despawn_finished=True)
    # robot 3 ended a leg and robot 4 completed: one completion, and only robot 4 is gone
    assert nfin == len(rec[t_pair]["completed"]) and eng.mission_finished().tolist() == rec[t_pair]["completed"] and 4 in rec[t_pair]["completed"]
    assert 3 in eng.mission_legs_ended().tolist() and 3 not in eng.mission_finished().tolist()
    with pytest.raises(MgxError, match="removed"):
        eng.set_idle(4, True)
    assert eng.idle_flags()[3] and eng.mission_legs_read()[3] == 0
    tr, tg, fin = eng.mission_read()
    assert fin[3] == -1 and fin[4] == t_pair and tg[3] == 1  # (the next waypoint index is the route's length: nothing to head for)
    mine = slice(3 * K, 4 * K)
    held = [b[mine].copy() for b in eng.read_beliefs()]
    sent = eng.message_counts(3)
    for tick in range(t_pair + 1, t_path):
        _hand_over(de, handed, tick)
        de.next_number, _, _, nfin = eng.mission_tick(de.comms_radius, de.next_number, de.steps, de.max_speed, de.delta_t, despawn_finished=True)
        assert 3 not in eng.mission_legs_ended().tolist() and 3 not in eng.mission_finished().tolist()
        assert np.array_equal(eng.mission_read()[0][3], tr[3]), tick
        for a, b in zip(eng.read_beliefs(), held):
            assert np.array_equal(a[mine], b), tick
        assert eng.message_counts(3) == sent and eng.idle_flags()[3]
    # the hand-over of the next leg: in place, as at spawn
    stats = eng.layout_stats()
    _hand_over(de, handed, t_path)
    assert eng.layout_stats() == stats and not eng.idle_flags()[3]
    assert eng.mission_read()[1][3] == 0 and eng.mission_read()[2][3] == -1
    eng.mission_tick(de.comms_radius, de.next_number, de.steps, de.max_speed, de.delta_t, despawn_finished=True)
    assert eng.layout_stats() == stats
    assert not np.array_equal(eng.mission_read()[0][3], tr[3])  # (on its way again)
    assert np.array_equal(eng.mission_read()[0], rec[t_path]["translation"])


def test_mission_run_stops_behind_every_tick_in_which_a_leg_ended():
    sc, n, rec, handed = reference()
    eng, de = _engine(sc, n, legs=LEGS[:n])
    tick, stops = 0, []
    while tick < TICKS:
        _hand_over(de, handed, tick)
        until = min([t for t in handed if t > tick] + [TICKS])  # (the next hand-over is the caller's: the call ends before it)
        out = eng.mission_run(until - tick, de.comms_radius, de.next_number, de.steps, de.max_speed, de.delta_t, despawn_finished=True)
        t = out["ticks"]
        assert t >= 1
        de.next_number = out["next_number"]
        for j in range(t):
            want = rec[tick + j]
            assert (int(out["created"][j]), int(out["deleted"][j])) == want["events"], tick + j
            assert out["finished"][j].tolist() == want["completed"], tick + j
            assert out["legs_ended"][j].tolist() == want["legs_ended"], tick + j
            assert np.array_equal(out["translations"][j], want["translation"]), tick + j
        if t < until - tick:  # it returned early: behind a tick in which a leg ended, and for nothing else
            assert rec[tick + t - 1]["legs_ended"]
            stops.append(tick + t - 1)
        assert all(not rec[tick + j]["legs_ended"] for j in range(t - 1))
        tick += t
        de.tick_no = tick
        _same_state(eng, de, rec[tick - 1], f"behind tick {tick - 1}")
    assert eng.mission_legs_ended().tolist() == rec[-1]["legs_ended"]
    ended = [t for t, x in enumerate(rec) if x["legs_ended"]]
    assert stops and set(stops) <= set(ended)


def test_worlds_without_legs_see_none_of_it():
    """legs_after = 0 everywhere — by default and spelled out — is a world of single routes: the events of the host chain without
    legs, and no robot is ever listed as having ended a leg"""
    sc, n, rec, _ = _oracle_run(20, False)
    assert (rec[-1]["finished_at"] >= 0).all() and not any(x["legs_ended"] for x in rec)
    for legs in (None, [0] * n):
        eng, de = _engine(sc, n, legs=legs)
        for tick, want in enumerate(rec):
            assert tuple(int(x) for x in de.tick()) == want["events"], tick
            assert de.legs_ended == [] and de.completed == want["completed"], tick
            assert len(eng.mission_legs_ended()) == 0
        _same_state(eng, de, rec[-1], "legless")
