"""Robot-robot collision bookkeeping on the device (mgx_collisions_*, magics_amd/csrc/mgx_collisions.hip) against the host pass
`sim.Simulation._collide` (the restatement of planner/collisions.rs:72-140,455-495): same (pass, a, b) events, AABBs equal as
f32 bit patterns, same per-robot counts — for both search methods, both libraries, inside the mission chain tick by tick and
many ticks per call, across relayouts, with a full log, and switched off."""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
from magics_amd import World, config, hostlib, scenarios, sim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(x):
    return int(np.float32(x).view(np.uint32))


class Checker:
    """the host pass on a bare Simulation, and the events it makes: (pass, a, b, mins bits, maxs bits)"""

    def __init__(self):
        self.s = sim.Simulation.__new__(sim.Simulation)
        self.s.collisions = {}
        self.events, self.seen, self.n_pass = [], {}, 0

    def step(self, ids, radii, pos):
        self.s._collide([{"id": int(i), "radius": F(radii[i])} for i in ids], pos)
        fresh = []
        for (a, b), h in self.s.collisions.items():
            k = self.seen.get((a, b), 0)
            assert len(h["aabbs"]) - k in (0, 1)
            if len(h["aabbs"]) > k:
                box = h["aabbs"][-1]
                fresh.append((self.n_pass, a, b, tuple(_bits(v) for v in box["mins"]), tuple(_bits(v) for v in box["maxs"])))
                self.seen[(a, b)] = k + 1
        self.events += sorted(fresh)
        self.n_pass += 1
        return len(fresh)

    def per_robot(self, n):
        out = np.zeros(n, np.uint32)
        for (a, b), h in self.s.collisions.items():
            out[a] += h["times"]
            out[b] += h["times"]
        return out


def _device_events(ev):
    return [(int(e["pass"]), int(e["robot_a"]), int(e["robot_b"]), tuple(_bits(v) for v in e["mins"]), tuple(_bits(v) for v in e["maxs"]))
            for e in ev]


def _bare_world(radii, fma=None):
    """robots that only stand for their radii (the passes below get their positions handed in)"""
    w = World(scenarios.JUNCTION_PARAMS, fma=fma)
    mean0, prior, dt = scenarios.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), scenarios.timesteps_for_K(10), 1.0, 5.0, 5.0)
    for r in radii:
        w.add_robot(mean0, prior, dt, float(r))
    return w


def test_state_machine_touching_counts_and_contacts_count_once():
    w, chk = _bare_world([1.0, 1.5]), Checker()
    w.collisions_enable(True)
    for x, times in ((3.0, 0), (2.5, 1), (2.0, 1), (2.6, 1), (2.4, 2), (0.0, 2)):
        pos = np.array([[0.0, -1.5, 0.0], [x, -1.5, 0.0]], dtype=F)
        w.collisions_update(pos)
        chk.step([0, 1], [1.0, 1.5], pos)
        ev, total, dropped, per = w.collisions_read()
        assert (total, dropped, list(per)) == (times, 0, [times, times]), x
    ev, total, _, per = w.collisions_read()
    assert _device_events(ev) == chk.events and [int(e["pass"]) for e in ev] == [1, 4]
    assert list(ev[0]["mins"]) == [1.0, -1.0] and list(ev[0]["maxs"]) == [1.0, 1.0]
    w.collisions_clear()                           # clear_robot_robot_collisions: everybody Free, nothing logged
    w.collisions_update(np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], dtype=F))
    ev, total, _, per = w.collisions_read()
    assert total == 1 and int(ev[0]["pass"]) == 0 and list(per) == [1, 1]


def _crowd(n, seed, passes=30):
    """the passes of a crowd that ignores each other: [(alive ids, positions [n, 3])], radii"""
    rng = np.random.default_rng(seed)
    side = np.sqrt(25.0 * n)
    x = rng.uniform(0.0, side, n).astype(F)
    z = rng.uniform(0.0, side, n).astype(F)
    radii = (0.5 + rng.random(n)).astype(F)
    alive = np.ones(n, bool)
    out = []
    for p in range(passes):
        if p == 10:
            alive[rng.choice(n, n // 20, replace=False)] = False
        if p >= 5:
            x[3] = np.nan
        pos = np.zeros((n, 3), F)
        pos[:, 0], pos[:, 1], pos[:, 2] = x, -1.5, z
        out.append((np.nonzero(alive)[0], pos))
        x = (x + rng.normal(0.0, 0.25, n).astype(F)).astype(F)
        z = (z + rng.normal(0.0, 0.25, n).astype(F)).astype(F)
    return out, radii


def _check_crowd(n, seed):
    passes, radii = _crowd(n, seed)
    chk, per_pass = Checker(), []
    for ids, pos in passes:
        per_pass.append(chk.step(ids, radii, pos))
    return passes, radii, chk, per_pass


def _run_crowd(w, passes):
    gone = set()
    for ids, pos in passes:
        for r in sorted(set(range(len(pos))) - set(int(i) for i in ids) - gone):
            w.remove_robot(r)
            gone.add(r)
        w.collisions_update(pos)


_CROWDS = {}


def _crowd_checked(n, seed):
    if (n, seed) not in _CROWDS:
        _CROWDS[(n, seed)] = _check_crowd(n, seed)
    return _CROWDS[(n, seed)]


@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
@pytest.mark.parametrize("method", [hostlib.NEIGHBOURS_PAIRS, hostlib.NEIGHBOURS_GRID, hostlib.NEIGHBOURS_AUTO], ids=["pairs", "grid", "auto"])
def test_crowd_of_a_thousand_equals_the_host_pass(method, fma):
    passes, radii, chk, per_pass = _crowd_checked(1000, 7)
    recontact = sum(1 for k in chk.seen.values() if k >= 2)
    print(f"checker: {len(chk.events)} events, {recontact} pairs with two or more contacts, fewest per pass {min(per_pass)}")
    assert len(chk.events) >= 500 and recontact >= 100 and min(per_pass) >= 1   # (the test cannot pass on an empty log)
    w = _bare_world(radii, fma=fma)
    w.collisions_enable(True, method=method)
    _run_crowd(w, passes)
    ev, total, dropped, per = w.collisions_read()
    assert (total, dropped) == (len(chk.events), 0)
    assert _device_events(ev) == chk.events
    assert np.array_equal(per, chk.per_robot(len(radii)))
    again, _, _, _ = w.collisions_read(first=total - 7)                      # a cursor into the log
    assert _device_events(again) == chk.events[-7:]


def test_small_world_under_auto_equals_the_host_pass():
    passes, radii, chk, per_pass = _crowd_checked(300, 11)
    recontact = sum(1 for k in chk.seen.values() if k >= 2)
    print(f"checker: {len(chk.events)} events, {recontact} pairs with two or more contacts")
    assert len(chk.events) >= 100 and recontact >= 20
    w = _bare_world(radii)
    w.collisions_enable(True)
    _run_crowd(w, passes)
    ev, total, dropped, per = w.collisions_read()
    assert (total, dropped) == (len(chk.events), 0) and _device_events(ev) == chk.events
    assert np.array_equal(per, chk.per_robot(len(radii)))


def test_a_full_log_drops_nothing_silently():
    """event_capacity = 300: the third pass fills the log — what did not fit is counted, what is there is right, and the
    per-robot counts stay exact"""
    passes, radii, chk, per_pass = _crowd_checked(1000, 7)
    assert per_pass[0] < 300 < sum(per_pass[:3]) and sum(per_pass[:2]) < 300, per_pass[:4]
    w = _bare_world(radii)
    w.collisions_enable(True, event_capacity=300)
    _run_crowd(w, passes)
    ev, total, dropped, per = w.collisions_read()
    assert total == 300 and len(ev) == 300
    assert total + dropped == len(chk.events)
    got = _device_events(ev)
    filling = next(p for p in range(len(per_pass)) if sum(per_pass[:p + 1]) > 300)
    before = [e for e in chk.events if e[0] < filling]
    assert got[:len(before)] == before
    rest = got[len(before):]
    assert rest and set(rest) <= {e for e in chk.events if e[0] == filling} and len(set(rest)) == len(rest)
    assert np.array_equal(per, chk.per_robot(len(radii)))


# ---- inside the mission chain ------------------------------------------------------------------------------------------
def _scenario(name):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


def _blind_circle():
    sc = _scenario("Circle Experiment")
    f = sc["formation"]["formations"][0]
    f["robots"] = 6
    f["initial-position"]["shape"]["radius"] = 14.0
    f["waypoints"][0]["shape"]["radius"] = 14.0
    sc["config"]["gbp"]["factors-enabled"]["interrobot"] = False
    return sc


def _engine(sc, device_collisions):
    return sim.Simulation(sc, World(config.world_params(sc["config"])), device_collisions=device_collisions)


def _export(s):
    return json.dumps(s.export(), sort_keys=True)


def test_blinded_circle_inside_the_mission_chain():
    sc, ticks = _blind_circle(), 40
    dev, host, ref = _engine(sc, True), _engine(sc, False), sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"])))
    assert dev._dev_coll and not host._dev_coll and not ref._dev_coll
    for _ in range(ticks):
        for s in (dev, host, ref):
            s.tick()
    ex = dev.export()
    assert sum(r["collisions"]["robots"] for r in ex["robots"].values()) > 0
    assert _export(dev) == _export(host) == _export(ref)
    chunked = _engine(sc, True).run(max_ticks=ticks, chunk=256)
    assert chunked.tick_no == ticks and _export(chunked) == _export(ref)
    # the same ticks through World.mission_run without a Transform coming back, one read at the end
    raw = _engine(sc, True)
    while not raw.robots:
        raw.tick()
    assert raw.tick_no < ticks and len(raw.robots) == len(dev.robots)  # (nobody spawns in the ticks that follow)
    out = raw.w.mission_run(ticks - raw.tick_no, raw.comms_radius, raw.next_number, raw.steps, float(raw.max_speed), float(raw.dt32),
                            despawn_finished=raw.despawn, method=raw.method, failure_rate=raw.failure_rate, wyrand_state=raw.rng.state,
                            want_translations=False)
    assert out["ticks"] == ticks - raw.tick_no and out["translations"] is None
    a, b = raw.w.collisions_read(), dev.w.collisions_read()
    assert a[1] == b[1] > 0 and a[2] == b[2] == 0
    assert _device_events(a[0]) == _device_events(b[0]) and np.array_equal(a[3], b[3])


def test_robots_that_join_while_others_overlap():
    """Junction Twoway without inter-robot factors: robots keep spawning while others drive through each other — the overlap
    state is carried over under the robots' ids when the world's arrays are laid out again"""
    sc = _scenario("Junction Twoway")
    sc["config"]["gbp"]["factors-enabled"]["interrobot"] = False
    dev, host = _engine(sc, True), _engine(sc, False)
    joined_during_overlap = 0
    for t in range(130):
        n_before, overlapping = len(host.robots), any(h["colliding"] for h in host.collisions.values())
        dev.tick()
        host.tick()
        host._flush_trackers(synchronise=True)     # (the host pass of this tick, one tick behind otherwise)
        if len(host.robots) > n_before and overlapping:
            joined_during_overlap += 1
    assert joined_during_overlap >= 1
    assert len(dev.robots) == len(host.robots) >= 20
    ex = dev.export()
    assert sum(r["collisions"]["robots"] for r in ex["robots"].values()) > 0
    assert _export(dev) == _export(host)


@pytest.mark.parametrize("method", [hostlib.NEIGHBOURS_PAIRS, hostlib.NEIGHBOURS_GRID], ids=["pairs", "grid"])
def test_robots_join_across_the_first_sizing_while_a_pair_overlaps(method):
    """The first sizing (for the two robots of the first pass) leaves room for R + R/4 + 64 per-robot counts
    and a pair-bit stride of that rounded up to 32.  One robot more than the stride holds joins while pair (0, 1) overlaps:
    the counts move to the front of a longer array and the pair's bit is set again under the new stride (k_collisions_rebits
    with a list that is not empty) — no second event for the held pair, one for a pair with an id beyond the old stride,
    and the state machine goes on as before."""
    first = 2
    room = first + first // 4 + 64                     # DevBuf::reserve: the room the first sizing leaves for the counts
    stride = (room + 31) & ~31
    n = stride + 1
    assert first < room < n                            # (both growth paths are crossed)
    radii = np.ones(n, F)
    w, chk = _bare_world(radii[:first]), Checker()
    w.collisions_enable(True, method=method)

    def run(pos, fresh):
        w.collisions_update(pos)
        assert chk.step(list(range(len(pos))), radii, pos) == fresh
        ev, total, dropped, per = w.collisions_read()
        assert (total, dropped) == (len(chk.events), 0) and _device_events(ev) == chk.events
        assert np.array_equal(per, chk.per_robot(len(pos)))
    pos = np.zeros((n, 3), F)
    pos[:, 0], pos[:, 1], pos[:, 2] = 10.0 * np.arange(n), -1.5, 100.0   # apart from everyone ...
    pos[0], pos[1] = (0.0, -1.5, 0.0), (1.0, -1.5, 0.0)                  # ... but (0, 1), which overlap from the start
    pos[n - 1, 0] = pos[n - 2, 0] + 0.5                                  # ... and the last two, which overlap each other
    run(pos[:first], 1)
    mean0, prior, dt = scenarios.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), scenarios.timesteps_for_K(10), 1.0, 5.0, 5.0)
    for _ in range(n - first):
        w.add_robot(mean0, prior, dt, 1.0)
    run(pos, 1)
    assert chk.events[-1][:3] == (1, n - 2, n - 1) and n - 1 >= stride
    pos[1, 0] = 5.0                                                      # (0, 1) part for a pass ...
    run(pos, 0)
    pos[1, 0] = 1.0                                                      # ... and meet again
    run(pos, 1)
    assert [e[:3] for e in chk.events] == [(0, 0, 1), (1, n - 2, n - 1), (3, 0, 1)]


def test_off_means_off():
    L = hostlib.lib()
    sc = _scenario("Circle Experiment")
    sc["formation"]["formations"][0]["robots"] = 12
    on, off = _engine(sc, True), _engine(sc, False)
    n = ctypes.c_uint64()
    assert L.mgx_collisions_read(off.w._w, 0, None, 0, ctypes.byref(n), ctypes.byref(n), None) == -4   # MGX_ERR_STATE
    assert L.mgx_collisions_update(off.w._w, None) == -4 and L.mgx_collisions_clear(off.w._w) == -4
    for t in range(20):
        on.tick()
        off.tick()
        assert on.w.last_sweep() == off.w.last_sweep(), t
        assert on.w.last_launch_count() == off.w.last_launch_count(), t
    assert len(on.robots) == 12
    for x, y in zip(on.w.read_beliefs(), off.w.read_beliefs()):
        assert np.array_equal(x, y)
    assert np.array_equal(on.translation, off.translation)
    assert on.w.collisions_read()[2] == 0


_LATTICE = {}


def _tangent_lattice():
    """1024 robots of radius 0.5 on the integer lattice [-16, 16)^2: every 4-neighbour pair exactly tangent (1 <= 1 in f32: a
    contact), every diagonal pair apart, and with cells of 1.001 tangent pairs in different cells on both sides of zero.  Three
    passes: the lattice, the lattice x 1.5 (everyone parts), the lattice again — and what the host pass makes of them."""
    if not _LATTICE:
        k = np.arange(1024)
        pos = np.zeros((1024, 3), F)
        pos[:, 0], pos[:, 1], pos[:, 2] = (k % 32) - 16, -1.5, (k // 32) - 16
        passes = [pos, (pos * F(1.5)).astype(F), pos.copy()]
        radii = np.full(1024, 0.5, F)
        chk = Checker()
        _LATTICE["x"] = (passes, radii, chk, [chk.step(range(1024), radii, p) for p in passes])
    return _LATTICE["x"]


@pytest.mark.parametrize("method", [hostlib.NEIGHBOURS_PAIRS, hostlib.NEIGHBOURS_GRID], ids=["pairs", "grid"])
def test_tangent_lattice_on_both_sides_of_zero(method):
    passes, radii, chk, per_pass = _tangent_lattice()
    assert per_pass == [1984, 0, 1984] and len(chk.events) == 3968       # 2 * 32 * 31 tangent pairs, twice
    assert {e[0] for e in chk.events} == {0, 2}
    w = _bare_world(radii)
    w.collisions_enable(True, method=method)
    for pos in passes:
        w.collisions_update(pos)
    ev, total, dropped, per = w.collisions_read()
    assert (total, dropped) == (3968, 0)
    assert _device_events(ev) == chk.events
    assert np.array_equal(per, chk.per_robot(1024))
