"""Schedules longer than one resident launch holds (MAX_SEGS = 32 segments), and the prior updates that ride in them: a schedule
cut into two launches whose first is confirmed before the second is built, long ticks with the updates in the first part only and
the last part lingering, the same launch by launch, mission ticks (updates in device memory) with resident launches on and off, a
batch cut at the fit check.  The bar is the oracle's beliefs and message counts bit for bit, and the launch counts written here.
A schedule of n steps of 3 (internal + external) is n + 1 segments: I, n - 1 times E I, E."""
import numpy as np
import pytest

import oracle
from magics_amd import World, scenarios as S
from magics_amd.driver import DeviceDriver, Driver

from parity import assert_identical, make_pair

pytestmark = pytest.mark.gpu

LONG = [3] * 34  # 35 segments: 32 + 3
ROBOTS = (0, 17, 63)


def segments(steps):
    """launches of a schedule run launch by launch: its phases (per step internal, then external) grouped as [E] I*"""
    ph = "".join(("I" if s & 1 else "") + ("E" if s & 2 else "") for s in steps)
    return ph.count("E") + (1 if ph.startswith("I") else 0)


class Frozen:
    """what the oracle held at some point: beliefs and a few robots' message counts"""

    def __init__(self, ref):
        self.beliefs = [np.array(x) for x in ref.read_beliefs()]
        self.counts = {r: ref.message_counts(r) for r in ROBOTS}

    def read_beliefs(self):
        return self.beliefs

    def message_counts(self, r):
        return self.counts[r]


@pytest.fixture(scope="module")
def sc():
    return S.grid_scenario(64, 16, interrobot=True)


@pytest.fixture(scope="module")
def long_ticks_ref(sc):
    """the oracle after three ticks of 34 steps, and after two ticks of the scenario's own schedule behind them"""
    ref = oracle.OracleWorld(sc["params"])
    S.populate(ref, sc)
    tick = S.tick_inputs(sc)
    for _ in range(3):
        ref.tick(steps=LONG, **tick)
    after_long = Frozen(ref)
    for _ in range(2):
        ref.tick(steps=sc["steps"], **tick)
    return after_long, Frozen(ref)


def same_as(eng, ref, what):
    assert_identical(eng, ref, what=what)
    assert all(np.isfinite(x).all() for x in eng.read_beliefs())
    for r in ROBOTS:
        assert eng.message_counts(r) == ref.message_counts(r), (what, r)


def test_long_schedules_are_cut_into_launches(sc):
    """31, 32 and 34 steps: 32 segments in one launch, 33 and 35 in two — the second one partial, built once the first is decided"""
    eng, ref = make_pair(sc)
    eng.set_linger(0)
    for n_steps, want in ((31, 1), (32, 2), (34, 2)):
        before = eng.resident_stats()[0]
        eng.iterate([3] * n_steps)
        ref.iterate([3] * n_steps)
        got = (eng.last_launch_count(), eng.resident_stats()[0] - before)
        print(f"[long schedules] {n_steps} steps: launches, resident launches = {got}")
        assert got == (want, want), (n_steps, got)
        same_as(eng, ref, f"iterate of {n_steps} steps")
    assert eng.resident_stats()[1:] == (0, 0) and eng.linger_stats() == (0, 0, 0, 0)


def test_long_ticks_linger_in_their_last_part(sc, long_ticks_ref):
    """ticks of 35 segments: the prior updates ride in the first part, the last part lingers, and the next long tick — too long
    for a post — ends the launch; the scenario's own ticks behind them are posted"""
    after_long, after_short = long_ticks_ref
    eng = World(sc["params"])
    S.populate(eng, sc)
    eng.set_linger(20000)  # (a bound no host jitter reaches)
    tick = S.tick_inputs(sc)
    for i in range(3):
        eng.tick(steps=LONG, **tick)
        assert eng.last_launch_count() == 2, i
    print("[long ticks] linger_stats, resident_stats =", eng.linger_stats(), eng.resident_stats())
    assert eng.linger_stats() == (3, 0, 0, 0) and eng.resident_stats() == (6, 0, 0)
    posted = World(sc["params"])  # (the same ticks on a second world: what a read between them would have ended)
    S.populate(posted, sc)
    posted.set_linger(20000)
    for _ in range(3):
        posted.tick(steps=LONG, **tick)
    for _ in range(2):
        posted.tick(steps=sc["steps"], **tick)
        assert posted.last_launch_count() == 1
    print("[long ticks + two short] linger_stats, resident_stats =", posted.linger_stats(), posted.resident_stats())
    assert posted.linger_stats() == (3, 2, 0, 0) and posted.resident_stats() == (6, 0, 0)
    same_as(eng, after_long, "three ticks of 34 steps")
    same_as(posted, after_short, "three ticks of 34 steps, two posted ticks")


def test_long_ticks_launch_by_launch(sc, long_ticks_ref):
    """resident launches switched off: 35 launches per tick, the prior updates in the first of them"""
    eng = World(sc["params"])
    S.populate(eng, sc)
    eng.set_resident_launches(False)
    tick = S.tick_inputs(sc)
    for i in range(3):
        eng.tick(steps=LONG, **tick)
        assert eng.last_launch_count() == 35, i
    assert eng.resident_stats() == (0, 0, 0) and eng.linger_stats() == (0, 0, 0, 0)
    same_as(eng, long_ticks_ref[0], "three ticks of 34 steps, launch by launch")


def test_mission_ticks_resident_and_launch_by_launch(sc):
    """mgx_mission_tick: the prior updates live in device memory (no ring slot).  Three ticks with resident launches, three
    without, against the host-driven chain on the oracle"""
    n, K = len(sc["robots"]), sc["K"]
    sc = dict(sc, ir=[])  # (the drivers' topology pass connects the robots)
    eng, ref = make_pair(sc)
    kw = dict(waypoints=[[tuple(rb["goal"])] for rb in sc["robots"]], radii=[rb["radius"] for rb in sc["robots"]],
              t0=[rb["t0"] for rb in sc["robots"]], steps=sc["steps"], comms_radius=8.0, target_speed=sc["target_speed"])
    de, dr = DeviceDriver(eng, n, K, **kw), Driver(ref, n, K, **kw)
    for phase, resident in (("resident", True), ("launch by launch", False)):
        eng.set_resident_launches(resident)
        before = eng.resident_stats()[0]
        for t in range(3):
            assert de.tick() == dr.tick(), (phase, t)
        grown = eng.resident_stats()[0] - before
        print(f"[mission ticks] {phase}: resident launches + {grown}, last launch count {eng.last_launch_count()}")
        assert grown == (3 if resident else 0) and eng.last_launch_count() == (1 if resident else segments(sc["steps"]))
        assert np.array_equal(de.state()[0], dr.translation)
        same_as(eng, ref, f"mission ticks, {phase}")
    assert eng.resident_stats()[1] == 0


def test_batch_cut_at_the_fit_check(sc):
    """four schedules in one batch: three fit a launch, the fourth makes a second submission — equal to four plain calls"""
    eng, ref = make_pair(sc)
    plain = World(sc["params"])
    S.populate(plain, sc)
    with eng.batch() as b:
        for _ in range(4):
            eng.iterate(sc["steps"])
    print("[batch of four] schedules, launches =", (b.schedules, b.launches))
    assert (b.schedules, b.launches) == (4, 2)
    for _ in range(4):
        plain.iterate(sc["steps"])
        ref.iterate(sc["steps"])
    same_as(eng, ref, "a batch of four schedules")
    same_as(plain, ref, "four plain calls")
    for a, c in zip(eng.read_beliefs(), plain.read_beliefs()):
        assert np.array_equal(a, c)
