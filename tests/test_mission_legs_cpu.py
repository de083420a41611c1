"""Missions of several legs on the host chain (no GPU): `Driver(legs=...)` on the CPU oracle against the same run composed by
hand from primitives that have tests of their own — a single-leg Driver, world.set_idle(r, True) in the tick a route empties with
legs left (Mission::next_route, robot.rs:966-993, sets Idle inside reached_waypoint) and `global_path` before the same tick as in
the legs= run.  Bit-identical, tick by tick: Transforms, every belief mean, completion ticks, message counts."""
import numpy as np

from magics_amd import scenarios as S
from magics_amd.driver import Driver
from mission_legs_common import LEGS, Script, driver_kwargs, legs_scenario
from oracle_ext import ExtOracleWorld

TICKS = 60


class ByHand(Driver):
    """a single-leg Driver (no legs=) whose caller does what Mission::next_route does: a route that empties with legs left is not
    the mission's end — the robot goes Idle in that very tick, ahead of the topology pass and the sweeps"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.left, self.ended = list(LEGS[:self.n]), []

    def _reached_waypoint(self):
        before = self.finished_at.copy()
        super()._reached_waypoint()
        self.ended = [r for r in range(self.n) if before[r] < 0 <= self.finished_at[r] and self.left[r] > 0]
        for r in self.ended:
            self.left[r] -= 1
            self.finished_at[r] = -1
            self.w.set_idle(r, True)
            self.idle[r] = True


def _world(sc):
    w = ExtOracleWorld(sc["params"])
    S.populate(w, sc)
    return w


def test_driver_with_legs_equals_the_hand_composition():
    sc, n = legs_scenario()
    wa, wb = _world(sc), _world(sc)
    a = Driver(wa, n, 10, **driver_kwargs(sc, n, despawn_when_finished=False))
    b = ByHand(wb, n, 10, **driver_kwargs(sc, n, legs=False, despawn_when_finished=False))
    script = Script()
    waited = 0
    for tick in range(TICKS):
        script.hand_over(tick, a, b)
        assert a.tick() == b.tick(), tick
        assert a.legs_ended == b.ended, tick
        script.ended(tick, a.legs_ended)
        assert np.array_equal(a.translation, b.translation), tick
        assert np.array_equal(a.finished_at, b.finished_at), tick
        assert np.array_equal(a.idle, b.idle), tick
        for x, y in zip(wa.read_beliefs(), wb.read_beliefs()):
            assert np.array_equal(x, y), tick
        assert [wa.message_counts(r) for r in range(n)] == [wb.message_counts(r) for r in range(n)], tick
        waited += int(a.idle.sum())
    assert np.isfinite(wa.read_beliefs()[2]).all()
    # every leg of the script was run: one hand-over for robot 0, two for robot 1, and robot 1 waited for one of them
    assert sorted((r, k) for _, r, k in script.handed) == [(0, 1), (1, 1), (1, 2)]
    assert waited >= 3 and a.legs_left.tolist() == [0, 0, 0]
    # a leg's end is not a completion: the missions complete at their last taskpoints, after their last hand-over
    last = {r: t for t, r, _ in script.handed}
    assert all(a.finished_at[r] > last[r] for r in (0, 1)) and a.finished_at[2] >= 0, (a.finished_at, script.handed)


def test_a_robot_between_two_legs_waits_where_it_is():
    sc, n = legs_scenario()
    w = _world(sc)
    d = Driver(w, n, 10, **driver_kwargs(sc, n))
    for tick in range(TICKS):
        d.tick()
        if 0 in d.legs_ended:
            break
    assert 0 in d.legs_ended and d.idle[0] and d.alive[0] and d.finished_at[0] < 0 and d.legs_left[0] == 0
    at, sent = d.translation[0].copy(), w.message_counts(0)[0]
    for _ in range(4):
        d.tick()
        assert 0 not in d.legs_ended and np.array_equal(d.translation[0], at) and d.way[0] == []
    assert w.message_counts(0)[0] == sent  # (an idle robot's own graph sends nothing)
