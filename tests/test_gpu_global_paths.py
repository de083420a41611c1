"""Global paths on the device: mgx_apply_global_paths — the reference's path-finding completion handler (robot.rs:643-799:
set_tracking_path, reset_variables, reset_tracking_factors, Route::update_waypoints, mission.state = Active) for a batch of
robots in one call, applied in place on a laid-out world — against the CPU oracle driven through the handler's own sequence and
against the engine's per-robot calls; device missions that wait for a path (MissionState::Idle) and then follow it.  Every
comparison is bit for bit."""
import numpy as np
import pytest

from magics_amd import World, scenarios as S
from magics_amd.driver import DeviceDriver, Driver
from magics_amd.hostlib import MgxError
from oracle_ext import ExtOracleWorld, make_pair
from parity import assert_identical
from global_paths_common import mission_kwargs, mission_scenario, replanned_path

pytestmark = pytest.mark.gpu

F32 = np.float32


def _lanes(K, n=4):
    """n robots on parallel lanes along +x, 10 m apart, tracking factors and no inter-robot ones; each follows a 3-point path
    whose corner lies half a metre beyond its variable K-2"""
    ts = S.timesteps_for_K(K)
    speed = 5.0
    robots = []
    for r in range(n):
        y = 10.0 * r
        mean0, prior, dt = S.robot_initial_state((0.0, y, speed, 0.0), (1000.0, y, speed, 0.0), ts, 1.0, speed, S.HORIZON_FOR_K[K] / speed)
        corner = float(mean0[K - 2, 0]) + 0.5
        path = np.array([(0.0, y), (corner, y), (corner, y + 20.0)], dtype=F32)
        robots.append(dict(mean0=mean0, prior_diag=prior, dt=dt, radius=1.0, path=path, order_key=r))
    params = dict(S.JUNCTION_PARAMS, enable_mask=S.EN_DYN | S.EN_OBS | S.EN_TRK)
    sdf = dict(rgb=np.full((16, 16, 3), 255, dtype=np.uint8), world_w=4000.0, world_h=4000.0)
    return dict(params=params, sdf=sdf, robots=robots, ir=[], steps=[1] * 6, K=K)


def _tracking_present(ref, robot, K):
    """per variable 1 .. K-2 of the oracle's graph: is the message of its tracking factor a message (not the empty one)?"""
    first = K + (K - 1) + (K - 2)
    out = []
    for i in range(1, K - 1):
        mine = [b for b in ref.variable_inbox(robot, i) if b[0] == robot and b[1] == first + i - 1]
        assert len(mine) == 1
        out.append(mine[0][2])
    return out


def _handler_on_the_oracle(ref, robots, paths, means, reset_tracking=True):
    """robot.rs:674-769, robot by robot"""
    for r, p, m in zip(robots, paths, means):
        ref.set_tracking_path(r, p)
        ref.reset_variables(r, m)
        if reset_tracking:
            ref.reset_tracking_factors(r)


def _lane_paths_and_means(sc):
    K = sc["K"]
    paths = [np.array([(2.0, 21.0), (12.0, 23.0), (24.0, 23.0), (24.0, 50.0)], dtype=F32), np.array([(1.0, 0.5), (400.0, 2.0)], dtype=F32)]
    means = []
    for r, dy in ((2, 1.0), (0, 0.5)):
        m = sc["robots"][r]["mean0"].copy()
        m[:, 0] += 2.0
        m[:, 1] += dy + 0.1 * np.arange(K)
        means.append(m)
    return [2, 0], paths, np.array(means)


# ---- 1. against the oracle, without inter-robot factors ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 16, 35])  # (35: the tracking state lives in HBM inside the sweeps)
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "segments"])
def test_two_robots_in_one_call(K, resident):
    sc = _lanes(K)
    eng, ref = make_pair(sc)
    if not resident:
        eng.set_resident_launches(False)
    for t in range(3):
        for w in (eng, ref):
            w.iterate(sc["steps"])
        assert_identical(eng, ref, what=f"before the paths, tick {t}")
    robots, paths, means = _lane_paths_and_means(sc)
    before = eng.layout_stats()
    eng.apply_global_paths(robots, paths, means)
    assert eng.layout_stats() == before
    _handler_on_the_oracle(ref, robots, paths, means)
    assert_identical(eng, ref, what="right after the paths")
    silent = []
    for it in range(12):
        for w in (eng, ref):
            w.iterate([1])
        assert_identical(eng, ref, what=f"after the paths, iteration {it}")
        silent.append((not any(_tracking_present(ref, 2, K)), not any(_tracking_present(ref, 0, K))))
        assert any(_tracking_present(ref, 1, K))  # (the others go on)
    assert silent == [(True, True)] * 10 + [(False, False)] * 2, silent
    assert eng.layout_stats() == before
    assert [eng.message_counts(r) for r in range(4)] == [ref.message_counts(r) for r in range(4)]


# ---- 2. against the oracle, with inter-robot factors -------------------------------------------------------------------------
def _grid():
    sc = S.grid_scenario(16, 10, interrobot=True, tracking=True, pitch=2.0, comm_radius=5.0)
    K = sc["K"]
    rng = np.random.default_rng(11)
    robots = [3, 8]
    means = np.array([sc["robots"][r]["mean0"] + rng.normal(0, 0.3, size=(K, 4)) for r in robots])
    paths = [np.ascontiguousarray(m[[0, K // 2, K - 1], :2], dtype=F32) for m in means]
    return sc, robots, paths, means


def _finite_but_for_the_reset(beliefs, what):
    eta, lam, mu = beliefs
    assert np.isfinite(eta).all() and np.isfinite(mu).all(), what
    assert (np.isfinite(lam) | (lam == np.inf)).all(), what


def test_with_interrobot_factors_against_the_oracle():
    sc, robots, paths, means = _grid()
    eng, ref = make_pair(sc)
    tick = S.tick_inputs(sc)
    for _ in range(2):
        for w in (eng, ref):
            w.tick(steps=sc["steps"], **tick)
    before = eng.layout_stats()
    eng.apply_global_paths(robots, paths, means)
    _handler_on_the_oracle(ref, robots, paths, means)
    assert_identical(eng, ref, what="grid, right after the paths")
    _finite_but_for_the_reset(ref.read_beliefs(), "after the paths")
    K = sc["K"]
    _, lam, mu = eng.read_beliefs()
    assert np.array_equal(mu[3 * K:4 * K], means[0]) and np.array_equal(mu[8 * K:9 * K], means[1])
    assert lam[3 * K, 0, 0] == 1e30 and np.isinf(lam[3 * K + 1, 2, 2]) and lam[3 * K + 1, 0, 1] == 0.0
    for t in range(3):
        for w in (eng, ref):
            w.tick(steps=sc["steps"], **tick)
        assert_identical(eng, ref, what=f"grid, tick {t} after the paths")
        _finite_but_for_the_reset(ref.read_beliefs(), f"tick {t} after the paths")
    assert eng.layout_stats() == before
    assert [eng.message_counts(r) for r in range(16)] == [ref.message_counts(r) for r in range(16)]


# ---- 3. against the per-robot calls --------------------------------------------------------------------------------------------
def _same(a, b, n, what):
    for name, x, y in zip(("eta", "lam", "mean"), a.read_beliefs(), b.read_beliefs()):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {name} differs"
    assert [a.message_counts(r) for r in range(n)] == [b.message_counts(r) for r in range(n)], what


def test_one_call_equals_the_three_calls():
    sc, robots, paths, means = _grid()
    new, old = World(sc["params"]), World(sc["params"])
    assert S.populate(new, sc) == S.populate(old, sc)
    tick = S.tick_inputs(sc)
    for _ in range(2):
        for w in (new, old):
            w.tick(steps=sc["steps"], **tick)
    new.apply_global_paths(robots, paths, means)
    for r, p, m in zip(robots, paths, means):
        old.set_tracking_path(r, p)
        old.reset_variables(r, m)
        old.reset_tracking_factors(r)
    _same(new, old, 16, "after the call")
    for t in range(3):
        for w in (new, old):
            w.tick(steps=sc["steps"], **tick)
    _same(new, old, 16, "three ticks later")
    # a topology pass with a larger radius: robot 3 keeps its connections (their creation epochs come from the device records,
    # where the call rewound them) and gets new ones
    pos = np.stack([sc["positions"][:, 0], np.full(16, 0.5), sc["positions"][:, 1]], axis=1).astype(F32)
    nxt = max(n0 for _, _, n0 in sc["ir"]) + sc["K"] - 1
    had = set(new.connections(3))
    out = [w.update_topology(pos, 7.0, nxt) for w in (new, old)]
    assert out[0] == out[1] and out[0][1] > 0
    assert had < set(new.connections(3)) and new.connections(3) == old.connections(3)
    for w in (new, old):
        w.tick(steps=sc["steps"], **tick)
    _same(new, old, 16, "after the topology pass")
    # one more robot: the device state is pulled into the host mirror and laid out again
    rb = sc["robots"][0]
    mean0 = rb["mean0"].copy()
    mean0[:, 0] += 40.0
    stats = new.layout_stats()
    for w in (new, old):
        assert w.add_robot(mean0, rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=16) == 16
    for t in range(2):
        for w in (new, old):
            w.tick(steps=sc["steps"], **tick)
    after = new.layout_stats()
    assert after[0] == stats[0] + 1 and after[1] == stats[1] + 1
    _same(new, old, 17, "after a robot joined")


# ---- 4. it ran on the device -----------------------------------------------------------------------------------------------------
def test_no_pull_and_no_relayout_on_a_laid_out_world():
    sc = _lanes(10)
    robots, paths, means = _lane_paths_and_means(sc)
    eng, ref = make_pair(sc)
    twin = World(sc["params"])
    S.populate(twin, sc)
    for w in (eng, ref, twin):
        w.iterate(sc["steps"])
    before, before_twin = eng.layout_stats(), twin.layout_stats()
    assert before == (1, 0) and before_twin == (1, 0)
    eng.apply_global_paths(robots, paths, means)
    eng.iterate([1])
    assert eng.layout_stats() == before
    twin.reset_variables(2, means[0])
    twin.iterate([1])
    assert twin.layout_stats() == (2, 1)
    _handler_on_the_oracle(ref, robots, paths, means)
    ref.iterate([1])
    assert_identical(eng, ref, what="in place")
    # a world that has switched a factor kind at run time keeps frozen inboxes: the call falls back to the per-robot calls —
    # the same result, one re-layout
    mask = sc["params"]["enable_mask"]
    for w in (eng, ref):
        w.set_enabled(mask & ~S.EN_OBS)
        w.iterate([1])
        w.set_enabled(mask)
        w.iterate([1] * 3)
    assert_identical(eng, ref, what="obstacle factors off and on")
    stats = eng.layout_stats()
    paths2 = [paths[1] + F32(1.0), paths[0] + F32(1.0)]
    eng.apply_global_paths([1, 3], paths2, means + 0.25)
    _handler_on_the_oracle(ref, [1, 3], paths2, means + 0.25)
    assert_identical(eng, ref, what="fallback, right after the paths")
    for it in range(12):
        for w in (eng, ref):
            w.iterate([1])
        assert_identical(eng, ref, what=f"fallback, iteration {it}")
    after = eng.layout_stats()
    assert after[0] > stats[0] and after[1] > stats[1]


# ---- 5. missions ---------------------------------------------------------------------------------------------------------------
def _mission_pair():
    sc, n, K = mission_scenario()
    eng, ref = make_pair(sc)
    idle = (1, 4)
    kw = mission_kwargs(sc, idle)
    return sc, n, K, idle, eng, ref, DeviceDriver(eng, n, K, **kw), Driver(ref, n, K, **kw)


def _compare_missions(de, dr, eng, ref, what):
    tr, left, fin = de.state()
    assert np.array_equal(tr, dr.translation), what
    assert left.tolist() == [len(wl) for wl in dr.way], what
    assert np.array_equal(fin, dr.finished_at), what
    assert_identical(eng, ref, what=what)
    assert not np.isnan(ref.read_beliefs()[2]).any() and not np.isnan(eng.read_beliefs()[2]).any(), what


def _first_six_ticks(sc, idle, eng, ref, de, dr):
    """ticks 0 .. 5 with robots `idle` waiting where they spawned, then their global paths arrive"""
    spawn = dr.translation.copy()
    for tick in range(6):
        assert de.tick() == dr.tick(), tick
        tr = de.state()[0]
        assert np.array_equal(tr, dr.translation), tick
        for r in idle:
            assert np.array_equal(tr[r], spawn[r]), (tick, r)
        assert not np.array_equal(tr[0], spawn[0])
    _compare_missions(de, dr, eng, ref, "before the paths")
    stats = eng.layout_stats()
    for r in idle:
        path = replanned_path(sc["robots"][r])
        de.global_path(r, path, 5.0)
        dr.global_path(r, path, 5.0)
    assert eng.layout_stats() == stats  # (in place: nothing pulled, nothing laid out again)
    _compare_missions(de, dr, eng, ref, "right after the paths")


def test_missions_wait_for_a_path_and_follow_it():
    sc, n, K, idle, eng, ref, de, dr = _mission_pair()
    _first_six_ticks(sc, idle, eng, ref, de, dr)
    for tick in range(6, 60):
        assert de.tick() == dr.tick(), tick
        if tick % 10 == 9:
            _compare_missions(de, dr, eng, ref, f"tick {tick + 1}")
    se, sr = de.summary(), dr.summary()
    assert se["finished_at_tick"] == sr["finished_at_tick"] and se["messages"] == sr["messages"] and se["ticks"] == sr["ticks"] == 60
    assert all(6 < sr["finished_at_tick"][r] < 60 for r in idle), sr["finished_at_tick"]


def test_missions_follow_a_path_through_mission_run():
    sc, n, K, idle, eng, ref, de, dr = _mission_pair()
    _first_six_ticks(sc, idle, eng, ref, de, dr)
    for chunk in range(6):
        out = eng.mission_run(9, de.comms_radius, de.next_number, de.steps, de.max_speed, de.delta_t, despawn_finished=True)
        assert out["ticks"] == 9
        de.next_number = out["next_number"]
        de.tick_no += 9
        events = [dr.tick() for _ in range(9)]
        assert [(int(c), int(d)) for c, d in zip(out["created"], out["deleted"])] == [(int(c), int(d)) for c, d in events], chunk
        _compare_missions(de, dr, eng, ref, f"chunk {chunk}")
    se, sr = de.summary(), dr.summary()
    assert se["finished_at_tick"] == sr["finished_at_tick"] and se["messages"] == sr["messages"]
    assert all(6 < sr["finished_at_tick"][r] < 60 for r in idle), sr["finished_at_tick"]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_batches_change_nothing():
    sc = _lanes(10)
    eng, ref = make_pair(sc)
    rb = sc["robots"][0]
    ghost = eng.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], 1.0, order_key=7, ghost=True)  # (another rank's: the engine only)
    for w in (eng, ref):
        w.iterate([1] * 12)
        w.remove_robot(3)
        w.iterate([1] * 3)
    K = sc["K"]
    p, m = np.array([(0.0, 0.0), (5.0, 1.0), (9.0, 9.0)], dtype=F32), np.zeros((K, 4))
    for robots, paths, kw, match in (([0, 1, 0], [p, p, p], {}, "listed twice"), ([1, ghost], [p, p], {}, "not a live local robot"),
                                     ([1, 3], [p, p], {}, "not a live local robot"), ([1, 0], [p, p[:1]], {}, "n_path"),
                                     ([7], [p], {}, "bad robot"), ([1], [p], dict(route=True), "no mission")):
        with pytest.raises(MgxError, match=match):
            eng.apply_global_paths(robots, paths, np.array([m] * len(robots)), **kw)
    for w in (eng, ref):
        w.iterate([1] * 3)
    assert_identical(eng, ref, what="after the refused batches")


def test_route_on_a_completed_mission_is_refused():
    sc, n, K = mission_scenario()
    eng, ref = make_pair(sc)
    kw = mission_kwargs(sc, ())
    kw["waypoints"][2] = [tuple(sc["robots"][2]["pos"])]  # robot 2 is where it wants to be: complete at the first tick
    de, dr = DeviceDriver(eng, n, K, despawn_when_finished=False, **kw), Driver(ref, n, K, despawn_when_finished=False, **kw)
    for tick in range(2):
        assert de.tick() == dr.tick()
    assert de.state()[2][2] == 0 and dr.finished_at[2] == 0
    with pytest.raises(MgxError, match="completed its mission"):
        de.global_path(2, replanned_path(sc["robots"][2]), 5.0)
    for tick in range(3):
        assert de.tick() == dr.tick()
    _compare_missions(de, dr, eng, ref, "after the refused route")


# ---- 7. the handler where the engine keeps no laid-out, unfrozen world (found by tests/test_gpu_script_fuzz.py) -----------------
def _handler_both(eng, ref, robots, paths, means):
    eng.apply_global_paths(robots, paths, means)
    _handler_on_the_oracle(ref, robots, paths, means)


def test_handler_before_the_first_iteration():
    sc = S.grid_scenario(6, 10, interrobot=True, tracking=True, seed=24, pitch=2.5, comm_radius=4.5)
    eng, ref = make_pair(sc)
    K = sc["K"]
    rng = np.random.default_rng(5)
    robots = [2, 3]
    means = np.array([sc["robots"][r]["mean0"] + rng.normal(0, 0.3, size=(K, 4)) for r in robots])
    paths = [np.ascontiguousarray(m[[0, K // 2, K - 1], :2], dtype=F32) for m in means]
    _handler_both(eng, ref, robots, paths, means)
    assert_identical(eng, ref, what="right after the handler")
    for k, steps in enumerate(([1], [2], [3])):
        for w in (eng, ref):
            w.iterate(steps)
        assert_identical(eng, ref, what=f"handler before the first iteration, schedule {k}")
    assert np.isfinite(ref.read_beliefs()[2]).all()


def test_handler_while_dynamics_factors_are_off():
    sc = S.grid_scenario(6, 10, interrobot=False, tracking=True, seed=3, pitch=2.5, comm_radius=4.5)
    eng, ref = make_pair(sc)
    K, mask = sc["K"], sc["params"]["enable_mask"]
    rng = np.random.default_rng(5)
    robots = [1, 4]
    means = np.array([sc["robots"][r]["mean0"] + rng.normal(0, 0.3, size=(K, 4)) for r in robots])
    paths = [np.ascontiguousarray(m[[0, K // 2, K - 1], :2], dtype=F32) for m in means]
    for w in (eng, ref):
        w.iterate([3, 3])
        w.set_enabled(mask & ~S.EN_DYN)
        w.iterate([3])
    _handler_both(eng, ref, robots, paths, means)
    for k in range(3):
        for w in (eng, ref):
            w.iterate([3])
        assert_identical(eng, ref, what=f"dynamics off, iteration {k} after the handler")
    for w in (eng, ref):
        w.set_enabled(mask)
        w.iterate([1])
    assert_identical(eng, ref, what="dynamics on again")
