"""Trackers on the device (mgx_tracks_*, magics_amd/csrc/mgx_tracks.hip) against the host trackers `sim.Simulation._track` /
`_tracks` (the restatement of planner/tracking.rs:117-136, 210-240) and the distance `Driver.tick` sums: same (tick, robot)
samples, positions and velocities equal as f32 bit patterns, same measuring spans, distances equal as f64 bit patterns — for both
libraries, over handed-in positions and inside the mission chain tick by tick and many ticks per call, with a full log, with robots
that join (appended in place and through a relayout), switched off and cleared."""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
from magics_amd import World, config, hostlib, scenarios, sim
from magics_amd.driver import DeviceDriver, Driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PERIOD = 100_000_000


def _bits(v):
    return tuple(int(x) for x in np.asarray(v, dtype=F).view(np.uint32))


class Checker:
    """the host trackers on a bare Simulation, one tick at a time, and the samples they make:
    (tick, robot, position bits [3], velocity bits [3], span in ticks)"""

    def __init__(self, n, tick_ns):
        s = sim.Simulation.__new__(sim.Simulation)
        s._dev_trk, s._trk_log, s.dt_ns, s.robots = False, [], int(tick_ns), []
        self.s, self.samples, self.prev_tick, self.over = s, [], {}, []
        self.grow(n)

    def grow(self, n):
        while len(self.s.robots) < n:
            self.s.robots.append({"id": len(self.s.robots), "positions": [], "velocities": [], "trk_elapsed": 0, "trk_prev": None})

    def step(self, k, moved, pos):
        s = self.s
        pos = np.ascontiguousarray(pos, dtype=F)
        had = [(len(r["positions"]), len(r["velocities"])) for r in s.robots]
        s._track([s.robots[int(i)] for i in moved], pos, (k + 1) * s.dt_ns * 1e-9)
        s._tracks()
        fresh = []
        for r, (n_p, n_v) in zip(s.robots, had):
            if len(r["positions"]) == n_p:
                assert len(r["velocities"]) == n_v
                continue
            i = r["id"]
            assert len(r["positions"]) == n_p + 1 and _bits(r["positions"][-1]) == _bits(pos[i, [0, 2]])
            span = k - self.prev_tick[i] if i in self.prev_tick else 0
            assert (len(r["velocities"]) == n_v + 1) == (span != 0)
            vel = r["velocities"][-1]["velocity"] if span else [0.0, 0.0, 0.0]
            if span:
                self.over.append((span, r["velocities"][-1]["timestamp"] - (k - span + 1) * s.dt_ns * 1e-9))
            fresh.append((int(k), i, _bits(pos[i]), _bits(vel), int(span)))
            self.prev_tick[i] = k
        self.samples += fresh
        return fresh


def _device_samples(samples):
    return [(int(e["tick"]), int(e["robot"]), _bits(e["position"]), _bits(e["velocity"]), int(e["span_ticks"])) for e in samples]


def _bare_world(n, fma=None):
    """robots that only stand for their ids (the passes below get their positions handed in)"""
    w = World(scenarios.JUNCTION_PARAMS, fma=fma)
    mean0, prior, dt = scenarios.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), scenarios.timesteps_for_K(10), 1.0, 5.0, 5.0)
    for _ in range(n):
        w.add_robot(mean0, prior, dt, 1.0)
    return w


def _walk(n, ticks, seed):
    """[ticks][n][3] f32 random walks (robot 1 never changes position) and [ticks][n] moved bytes: about one robot in ten rests in
    a tick, and robot n // 2 toggles every three ticks"""
    rng = np.random.default_rng(seed)
    pos = np.zeros((ticks, n, 3), F)
    p = rng.uniform(-50.0, 50.0, (n, 3)).astype(F)
    for t in range(ticks):
        step = rng.normal(0.0, 0.3, (n, 3)).astype(F)
        if n > 1:
            step[1] = 0.0
        p = (p + step).astype(F)
        pos[t] = p
    moved = (rng.random((ticks, n)) > 0.1).astype(np.uint8)
    if n > 1:
        moved[:, 1] = 1
    moved[:, n // 2] = ((np.arange(ticks) // 3) % 2 == 0).astype(np.uint8)
    return pos, moved


# ---- 1. handed-in positions -----------------------------------------------------------------------------------------------------
# (tick_ns, ticks, first tick): a remainder carried over the periods; a sample in every tick; several periods per tick (one sample,
# the remainder by %); a clock so large that t(k) - t(k - span) is not span * tick_ns * 1e-9 to the last bit
CLOCKS = [(16_666_667, 45, 0), (PERIOD, 12, 0), (250_000_000, 8, 3), (16_666_667, 45, 10**7)]


@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_handed_in_positions_equal_the_host_trackers(n, fma):
    w = _bare_world(n, fma)
    for ci, (tick_ns, ticks, k0) in enumerate(CLOCKS):
        pos, moved = _walk(n, ticks, 100 * n + ci)
        chk = Checker(n, tick_ns)
        w.tracks_enable(True, period_ns=PERIOD, tick_ns=tick_ns, next_tick=k0)
        for t in range(ticks):
            every = tick_ns == PERIOD and t % 2 == 0            # moved = NULL: every live robot
            w.tracks_update(k0 + t, pos[t], None if every else moved[t])
            chk.step(k0 + t, range(n) if every else np.nonzero(moved[t])[0], pos[t])
        got, in_log, dropped, dist = w.tracks_take()
        assert (in_log, dropped) == (len(chk.samples), 0) and len(chk.samples) > 0
        assert _device_samples(got) == chk.samples, (n, tick_ns, k0)
        assert not dist.any()                                   # (mgx_tracks_update adds no distance)
        if n > 1:  # the robot that never moved: velocity exactly +0
            still = [s for s in chk.samples if s[1] == 1 and s[4]]
            assert still and all(s[3] == (0, 0, 0) for s in still)
        if tick_ns == 250_000_000:
            assert {s[4] for s in chk.samples} >= {0, 1} and max(len([s for s in chk.samples if s[0] == k0 + t]) for t in range(ticks)) <= n
        if k0 >= 10**7:  # the times are where rounding shows: some measured span is not the product to the last bit
            assert any(over != span * tick_ns * 1e-9 for span, over in chk.over)
        assert w.tracks_take()[:3][1:] == (0, 0)                # taken: the log is empty again
        w.tracks_enable(False)


# ---- 2. a full log ----------------------------------------------------------------------------------------------------------------
def test_a_full_log_drops_nothing_silently():
    n = 20
    w, chk = _bare_world(n), Checker(n, PERIOD)
    pos, _ = _walk(n, 4, 5)
    w.tracks_enable(True, period_ns=PERIOD, tick_ns=PERIOD, next_tick=0, sample_capacity=8)
    w.tracks_update(0, pos[0])
    first = chk.step(0, range(n), pos[0])
    got, in_log, dropped, _ = w.tracks_take(capacity=4)         # too little room: nothing is taken, the size comes back
    assert (len(got), in_log, dropped) == (0, 8, n - 8)
    got, in_log, dropped, _ = w.tracks_take()
    kept = _device_samples(got)
    assert (len(got), in_log, dropped) == (8, 8, n - 8)
    assert set(kept) <= set(first) and len(set(kept)) == 8 and kept == sorted(kept)
    # stored again, and the velocities are measured from the samples that were dropped too
    some = [0, 3, 7, 12, 19]
    mv = np.zeros(n, np.uint8)
    mv[some] = 1
    w.tracks_update(1, pos[1], mv)
    second = chk.step(1, some, pos[1])
    got, in_log, dropped, _ = w.tracks_take()
    assert (in_log, dropped) == (5, n - 8) and _device_samples(got) == second and all(s[4] == 1 for s in second)
    w.tracks_update(2, pos[2])                                  # ... and full again: the count of dropped samples goes on
    third = chk.step(2, range(n), pos[2])
    got, in_log, dropped, _ = w.tracks_take()
    assert (in_log, dropped) == (8, 2 * (n - 8)) and set(_device_samples(got)) <= set(third)


# ---- inside the mission chain -----------------------------------------------------------------------------------------------------
def _scenario(name):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


def _blind_circle():
    sc = _scenario("Circle Experiment")
    f = sc["formation"]["formations"][0]
    f["robots"] = 10
    f["initial-position"]["shape"]["radius"] = 14.0
    f["waypoints"][0]["shape"]["radius"] = 14.0
    sc["config"]["gbp"]["factors-enabled"]["interrobot"] = False
    return sc


def _engine(sc, device_trackers, fma=None, reserve=True):
    w = World(config.world_params(sc["config"]), fma=fma)
    if not reserve:  # (no head-room: robots that spawn later make the world lay its arrays out again)
        w.reserve = lambda robots: None
    return sim.Simulation(sc, w, device_trackers=device_trackers)


class Tap:
    """a Simulation with the trackers on the device: every sample it takes from the log, as the device made it"""

    def __init__(self, s):
        assert s._dev_trk
        self.s, self.samples, take = s, [], s.w.tracks_take

        def tracks_take(*a, **kw):
            out = take(*a, **kw)
            assert out[2] == 0
            self.samples += _device_samples(out[0])
            return out
        s.w.tracks_take = tracks_take

    def end(self):
        self.s._tracks()
        return self.samples, np.array([r["travelled"] for r in self.s.robots])


class Twin:
    """the same run with the trackers on the host: what its _track is handed for every tick — the moving robots and the Transforms
    after the move — feeds the Checker, and the means it reads in front of a tick give the distances by Driver.tick's expression"""

    def __init__(self, s):
        assert not s._dev_trk and s.dev
        self.s, self.chk, self.means, self.dist = s, Checker(0, s.dt_ns), {}, np.zeros(0)
        s._track = self._noted

    def _noted(self, moving, tr, now):
        s = self.s
        k = int(round(now * 1e9 / s.dt_ns)) - 1
        ids = np.array([r["id"] for r in moving], dtype=np.int64)
        self.chk.grow(len(s.robots))
        self.dist = np.concatenate([self.dist, np.zeros(len(s.robots) - len(self.dist))])
        self.chk.step(k, ids, tr)
        if len(ids):
            m0, m1 = self.means.pop(k)
            ts = np.array([r["time_scale"] for r in moving])
            change = ts[:, None] * (m1[ids] - m0[ids])
            self.dist[ids] += np.sqrt(change[:, 0] * change[:, 0] + change[:, 1] * change[:, 1])   # (driver.py, Driver.tick)

    def tick(self):  # Simulation.tick, with a look at the means between the spawns and the FixedUpdate
        s = self.s
        s._apply_plans()
        s._spawn()
        s._plan()
        if s.robots:
            self.means[s.tick_no] = (s.w.read_variable_means(0), s.w.read_variable_means(1))
            s._tick_device()
        s.tick_no += 1

    def end(self):
        self.s._flush_trackers(synchronise=True)
        self.dist = np.concatenate([self.dist, np.zeros(len(self.s.robots) - len(self.dist))])
        return self.chk.samples, self.dist


def _set_idle(sims, rid, idle):
    for s in sims:
        s.w.set_idle(rid, idle)
        s.robots[rid]["idle"] = idle


@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
def test_blinded_circle_inside_the_mission_chain(fma):
    """ten robots cross a circle through each other, 60 ticks of which the first ten have no robot yet; robot 3 is Idle from tick
    22 to tick 31 (its timer and its distance rest), and everybody arrives and despawns before the end"""
    sc, ticks, idle_from, idle_to = _blind_circle(), 60, 22, 32
    dev, chunked, twin = Tap(_engine(sc, True, fma)), Tap(_engine(sc, True, fma)), Twin(_engine(sc, False, fma))
    for t in range(ticks):
        if t in (idle_from, idle_to):
            _set_idle((dev.s, twin.s), 3, t == idle_from)
        dev.s.tick()
        twin.tick()
    for upto, idle in ((idle_from, True), (idle_to, False), (ticks, None)):
        chunked.s.run(max_ticks=upto, chunk=256)
        assert chunked.s.tick_no == upto
        if idle is not None:
            _set_idle((chunked.s,), 3, idle)
    want, want_dist = twin.end()
    assert len(dev.s.robots) == 10 and sum(r["completed"] and not r["alive"] for r in dev.s.robots) >= 1
    assert min(s[0] for s in want) > 0 and len(want) > 100                    # (the first ticks have no robot: only the host counts them)
    assert not [s for s in want if s[1] == 3 and idle_from <= s[0] < idle_to]
    assert any(s[1] == 3 and s[4] > 1 for s in want)                         # measured over the ticks it sat idle
    for tap in (dev, chunked):
        got, dist = tap.end()
        assert got == want
        assert np.array_equal(dist, want_dist) and (dist > 0).all()
    assert json.dumps(dev.s.export(), sort_keys=True) == json.dumps(chunked.s.export(), sort_keys=True)


# ---- 4. distance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
def test_device_driver_distance_travelled(fma):
    """the circle workload of tests/test_gpu_driver.py on a smaller circle: the device's distances are Driver.tick's sums to the
    bit — against the oracle's Driver (libmgx.so; the other library's beliefs are its own), and in both libraries against the
    same expression over the means the engine itself holds in front of every tick"""
    n, K, ticks = 8, 10, 60
    sc = scenarios.circle_scenario(n, K, circle_radius=6.0, n_internal=10, n_external=10)
    sc["ir"] = []
    eng, ref = World(sc["params"], fma=fma), oracle.OracleWorld(sc["params"])
    assert scenarios.populate(eng, sc) == scenarios.populate(ref, sc)
    kw = dict(waypoints=[[tuple(rb["goal"])] for rb in sc["robots"]], radii=[rb["radius"] for rb in sc["robots"]],
              t0=[rb["t0"] for rb in sc["robots"]], steps=sc["steps"], comms_radius=12.0, target_speed=sc["target_speed"])
    de, dr = DeviceDriver(eng, n, K, tracks=True, **kw), Driver(ref, n, K, **kw)
    own, ts = np.zeros(n), dr.time_scale
    for _ in range(ticks):
        m0, m1 = eng.read_variable_means(0), eng.read_variable_means(1)
        before = de.finished_at < 0
        de.tick()
        dr.tick()
        moving = np.nonzero(before & (de.finished_at < 0))[0]                # (a robot that arrives in a tick does not move in it)
        change = ts[moving, None] * (m1[moving] - m0[moving])
        own[moving] += np.sqrt(change[:, 0] * change[:, 0] + change[:, 1] * change[:, 1])
    se, sr = de.summary(), dr.summary()
    assert se["finished"] >= 1 and min(se["distance_travelled"]) > 1.0
    assert se["distance_travelled"] == own.tolist()
    if not fma:
        assert se["finished_at_tick"] == sr["finished_at_tick"] and se["distance_travelled"] == sr["distance_travelled"]
    samples = np.concatenate(de.track_samples)
    assert len(samples) > n and not de.w.tracks_take()[2]                    # hz = 10: a sample per moving robot and tick


# ---- 5. joiners -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [True, False], ids=["appended", "relayout"])
def test_robots_that_join_keep_the_others_state(reserve):
    """Junction Twoway at 30 Hz (three or four ticks to a sample, a remainder carried along): the second wave spawns after two
    seconds, into head-room the world reserved or through a relayout — the first wave's timers, previous samples and distances
    go on as if nothing had happened, the newcomers start from zero"""
    sc, ticks = _scenario("Junction Twoway"), 75
    sc["config"]["simulation"]["hz"] = 30.0
    dev, twin = Tap(_engine(sc, True, reserve=reserve)), Twin(_engine(sc, False, reserve=reserve))
    assert dev.s.dt_ns == 33_333_333
    first_wave = None
    for t in range(ticks):
        dev.s.tick()
        twin.tick()
        first_wave = first_wave or len(dev.s.robots)
    appends = dev.s.w.append_stats()
    assert (appends[0] >= 1 and appends[1] >= len(dev.s.robots) - first_wave) if reserve else appends[:2] == (0, 0), appends
    assert len(dev.s.robots) > first_wave >= 1
    want, want_dist = twin.end()
    got, dist = dev.end()
    assert got == want and np.array_equal(dist, want_dist)
    late = [s for s in want if s[1] >= first_wave]
    assert late and min(late)[4] == 0 and min(s[0] for s in late) >= 55      # a newcomer's first sample has no velocity
    old = [s for s in want if s[1] < first_wave and s[0] >= 62]
    assert old and all(s[4] in (3, 4) for s in old)                          # the others' timers did not start again
    assert (dist[:first_wave] > dist[first_wave:].max()).all() and (dist > 0).all()


# ---- 6. off means off, and clear --------------------------------------------------------------------------------------------------
def test_off_means_off_and_clear():
    L = hostlib.lib()
    sc = _scenario("Circle Experiment")
    sc["formation"]["formations"][0]["robots"] = 12
    on, off = _engine(sc, True), _engine(sc, False)
    n = ctypes.c_uint64()
    assert L.mgx_tracks_take(off.w._w, None, 0, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n), None) == -4   # MGX_ERR_STATE
    assert L.mgx_tracks_update(off.w._w, None, None, 0) == -4 and L.mgx_tracks_clear(off.w._w) == -4
    assert L.mgx_tracks_set_clock(off.w._w, 0) == -4
    first = None
    for t in range(20):
        on.tick()
        off.tick()
        first = t if first is None and on.robots else first
        assert on.w.last_sweep() == off.w.last_sweep(), t
        assert on.w.last_launch_count() == off.w.last_launch_count(), t
    assert len(on.robots) == 12
    for x, y in zip(on.w.read_beliefs(), off.w.read_beliefs()):
        assert np.array_equal(x, y)
    assert np.array_equal(on.translation, off.translation)
    got, in_log, dropped, dist = on.w.tracks_take()
    assert 0 < first < 15 and in_log == len(got) == 12 * (20 - first) and dropped == 0 and (dist > 0).all()   # a sample per robot and tick
    on.tick()
    on.w.tracks_clear()
    got, in_log, dropped, dist = on.w.tracks_take()
    assert (len(got), in_log, dropped) == (0, 0, 0) and not dist.any()
    on.tick()
    got, in_log, dropped, dist = on.w.tracks_take()
    assert len(got) == 12 and all(int(e["span_ticks"]) == 0 and not e["velocity"].any() for e in got) and (dist > 0).all()
    on.w.tracks_enable(False)
    assert L.mgx_tracks_clear(on.w._w) == -4
