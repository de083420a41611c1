"""Robots that join a laid-out world with head-room (mgx_world_reserve) are appended on the device: one staged block, one
kernel (k_append_robots), nothing pulled and nothing laid out again — mgx_layout_stats does not move and mgx_append_stats counts
the append.  Every comparison is bit for bit against the CPU oracle, which knows no head-room: a robot is a robot.  A world that
never reserves keeps today's path (one layout and one pull per commit with new robots)."""
import json
import os

import numpy as np
import pytest

import oracle
from magics_amd import World, config, hostlib, scenarios as S, sim
from parity import assert_identical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _lanes(K, n):
    """n robots on parallel lanes along +x, 10 m apart: dynamics, obstacle and tracking factors, a 3-point path each"""
    horizon = {5: 5, 16: S.HORIZON_FOR_K[16]}[K]  # (timesteps: 5 variables at horizon 5, 16 at the table's 45)
    ts = hostlib.variable_timesteps(horizon, 3)
    assert len(ts) == K
    speed = 5.0
    robots = []
    for r in range(n):
        y = 10.0 * r
        mean0, prior, dt = S.robot_initial_state((0.0, y, speed, 0.0), (1000.0, y, speed, 0.0), ts, 1.0, speed, horizon / speed)
        corner = float(mean0[K - 2, 0]) + 0.5
        path = np.array([(0.0, y), (corner, y), (corner, y + 20.0)], dtype=F32)
        robots.append(dict(mean0=mean0, prior_diag=prior, dt=dt, radius=1.0 + 0.125 * r, path=path, order_key=r))
    params = dict(S.JUNCTION_PARAMS, enable_mask=S.EN_DYN | S.EN_OBS | S.EN_TRK)
    sdf = dict(rgb=np.full((16, 16, 3), 255, dtype=np.uint8), world_w=4000.0, world_h=4000.0)
    return dict(params=params, sdf=sdf, robots=robots, ir=[], steps=[1] * 6, K=K)


def _first(sc, n):
    """the scenario with its first n robots only (the others join later)"""
    return dict(sc, robots=sc["robots"][:n], ir=[e for e in sc["ir"] if e[0] < n and e[1] < n])


def _add(worlds, rb):
    ids = [w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=rb["order_key"]) for w in worlds]
    assert len(set(ids)) == 1
    return ids[0]


def _reserved_pair(sc, n, reserve):
    """engine (head-room asked for before the first layout) and oracle, populated with the first n robots"""
    eng, ref = World(sc["params"]), oracle.OracleWorld(sc["params"])
    if reserve:
        eng.reserve(reserve)
    assert S.populate(eng, _first(sc, n)) == S.populate(ref, _first(sc, n))
    return eng, ref


def _counts(w, n):
    return [w.message_counts(r) for r in range(n)]


# ---- 1. it ran on the device ---------------------------------------------------------------------------------------------------
def test_a_robot_joins_without_pull_or_layout():
    sc = _lanes(16, 4)
    eng, ref = _reserved_pair(sc, 3, 8)
    twin = World(sc["params"])
    S.populate(twin, _first(sc, 3))
    for w in (eng, ref, twin):
        w.iterate(sc["steps"])
    assert eng.layout_stats() == (1, 0) and eng.append_stats() == (0, 0, 0)
    assert _add((eng, ref, twin), sc["robots"][3]) == 3
    for w in (eng, ref, twin):
        w.iterate([1])
    assert eng.layout_stats() == (1, 0)
    assert eng.append_stats() == (1, 1, 0)
    assert_identical(eng, ref, what="first iteration with the appended robot")
    for it in range(5):
        for w in (eng, ref, twin):
            w.iterate([1])
        assert_identical(eng, ref, what=f"appended, iteration {it + 1}")
    assert eng.layout_stats() == (1, 0) and eng.append_stats() == (1, 1, 0)
    # the world that never asked for head-room: one more layout, one pull, no append — and the same numbers
    assert twin.layout_stats() == (2, 1) and twin.append_stats() == (0, 0, 0)
    assert_identical(twin, ref, what="the unreserved twin")
    assert _counts(eng, 4) == _counts(ref, 4)


# ---- 2. both snapshot parities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [3, 4], ids=["odd", "even"])
def test_both_snapshot_parities(sweeps):
    sc = _lanes(16, 4)
    eng, ref = _reserved_pair(sc, 3, 8)
    eng.set_resident_launches(False)  # (one launch per sweep: the buffer the device reads next is the sweeps' parity)
    for w in (eng, ref):
        for _ in range(sweeps):
            w.iterate([1])
    _add((eng, ref), sc["robots"][3])
    for it in range(6):
        for w in (eng, ref):
            w.iterate([1])
        assert_identical(eng, ref, what=f"{sweeps} sweeps before the append, iteration {it}")
    assert eng.layout_stats() == (1, 0) and eng.append_stats() == (1, 1, 0)


# ---- 3. strides ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 16])
def test_two_robots_in_one_commit_at_odd_strides(K):
    sc = _lanes(K, 5)
    eng, ref = _reserved_pair(sc, 3, 7)
    for w in (eng, ref):
        w.iterate([1] * 3)
    for rb in sc["robots"][3:]:
        _add((eng, ref), rb)
    for it in range(6):  # (dynamics and tracking state of old and new robots: a wrong ND / NT shows in the first)
        for w in (eng, ref):
            w.iterate([1])
        assert_identical(eng, ref, what=f"K = {K}, two appended, iteration {it}")
    assert eng.layout_stats() == (1, 0) and eng.append_stats() == (1, 2, 0)
    assert _counts(eng, 5) == _counts(ref, 5)
    # ... and what a later pull reads of all five
    eng.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    ref.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    for w in (eng, ref):
        w.iterate([1] * 3)
    assert_identical(eng, ref, what=f"K = {K}, laid out again from the pulled mirror")
    assert eng.layout_stats() == (2, 1)


# ---- 4. the new robot meets old ones in the same tick -------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "segments"])
def test_new_robot_connects_in_the_tick_it_joins(resident):
    full = S.grid_scenario(6, 16, interrobot=True, pitch=2.0, comm_radius=5.0)
    sc = _first(full, 5)
    eng, ref = World(sc["params"]), oracle.OracleWorld(sc["params"])
    eng.reserve(9)
    assert S.populate(eng, sc) == S.populate(ref, sc)
    if not resident:
        eng.set_resident_launches(False)
    tick5, tick6 = S.tick_inputs(sc), S.tick_inputs(full)
    for w in (eng, ref):
        w.tick(steps=sc["steps"], **tick5)
    assert_identical(eng, ref, what="five robots")
    pos = np.stack([full["positions"][:, 0], np.full(6, 0.5), full["positions"][:, 1]], axis=1).astype(F32)
    nxt = max(n0 for _, _, n0 in sc["ir"]) + sc["K"] - 1
    _add((eng, ref), full["robots"][5])
    for t in range(3):
        out = [w.update_topology(pos, 5.0, nxt) for w in (eng, ref)]
        assert out[0] == out[1]
        nxt = out[0][0]
        if t == 0:
            assert out[0][1] > 0  # (the new robot is within range of old ones)
        for w in (eng, ref):
            w.tick(steps=full["steps"], **tick6)
        assert [eng.connections(r) for r in range(6)] == [ref.connections(r) for r in range(6)], t
        assert eng.connections(5)
        assert_identical(eng, ref, what=f"tick {t} with the robot that joined")
        form = eng.last_sweep()[2]
        assert form in ((1, 2) if resident else (0,)), (t, eng.last_sweep())
    assert eng.layout_stats() == (1, 0) and eng.append_stats() == (1, 1, 0)
    assert _counts(eng, 6) == _counts(ref, 6)


# ---- 5. capacity ---------------------------------------------------------------------------------------------------------------
def test_head_room_runs_out_and_doubles():
    sc = _lanes(5, 6)
    eng, ref = _reserved_pair(sc, 3, 4)
    for w in (eng, ref):
        w.iterate([1] * 2)
    expected = [((1, 0), (1, 1, 0)),   # fits
                ((2, 1), (1, 1, 1)),   # the fifth robot does not: laid out in full, with room for ten
                ((2, 1), (2, 2, 1))]   # in place again
    for rb, (layouts, appends) in zip(sc["robots"][3:], expected):
        n = _add((eng, ref), rb) + 1
        for it in range(2):
            for w in (eng, ref):
                w.iterate([1])
            assert_identical(eng, ref, what=f"{n} robots, iteration {it}")
        assert eng.layout_stats() == layouts and eng.append_stats() == appends, (n, eng.layout_stats(), eng.append_stats())
    assert _counts(eng, 6) == _counts(ref, 6)


# ---- 6. fallback conditions keep today's results --------------------------------------------------------------------------------
def test_a_switched_kind_falls_back():
    sc = _lanes(5, 4)
    eng, ref = _reserved_pair(sc, 3, 8)
    mask = sc["params"]["enable_mask"]
    for w in (eng, ref):
        w.iterate([1] * 2)
        w.set_enabled(mask & ~S.EN_OBS)
        w.iterate([1])
        w.set_enabled(mask)
        w.iterate([1] * 3)
    stats = eng.layout_stats()
    _add((eng, ref), sc["robots"][3])
    for it in range(4):
        for w in (eng, ref):
            w.iterate([1])
        assert_identical(eng, ref, what=f"frozen inboxes: full layout, iteration {it}")
    assert eng.layout_stats() == (stats[0] + 1, stats[1] + 1) and eng.append_stats() == (0, 0, 1)


def test_a_new_image_with_a_new_robot_is_one_full_layout():
    sc = _lanes(5, 4)
    eng, ref = _reserved_pair(sc, 3, 8)
    for w in (eng, ref):
        w.iterate([1] * 2)
    _add((eng, ref), sc["robots"][3])
    for w in (eng, ref):
        w.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
        w.iterate([1] * 3)
    assert_identical(eng, ref, what="image and robot together")
    assert eng.layout_stats() == (2, 1) and eng.append_stats() == (0, 0, 1)


def test_a_ghost_is_laid_out_in_full():
    sc = _lanes(5, 4)
    eng, ref = _reserved_pair(sc, 3, 8)
    for w in (eng, ref):
        w.iterate([1] * 2)
    rb = sc["robots"][3]
    assert eng.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], 1.0, order_key=3, ghost=True) == 3  # (another rank's: the engine only)
    for w in (eng, ref):
        w.iterate([1] * 3)
    for name, a, b in zip(("eta", "lam", "mean"), eng.read_beliefs(), ref.read_beliefs()):
        assert np.array_equal(a[:3 * 5], b), name  # (the oracle holds the three local robots)
    assert eng.layout_stats() == (2, 1) and eng.append_stats() == (0, 0, 1)


def test_reserve_on_a_laid_out_world_costs_one_layout():
    sc = _lanes(5, 5)
    eng, ref = _reserved_pair(sc, 3, 0)
    for w in (eng, ref):
        w.iterate([1] * 2)
    assert eng.layout_stats() == (1, 0)
    eng.reserve(3)  # (at the robot count: nothing)
    for w in (eng, ref):
        w.iterate([1])
    assert eng.layout_stats() == (1, 0)
    eng.reserve(8)
    for w in (eng, ref):
        w.iterate([1])
    assert eng.layout_stats() == (2, 1) and eng.append_stats() == (0, 0, 0)
    assert_identical(eng, ref, what="laid out again with head-room")
    for rb in sc["robots"][3:]:
        _add((eng, ref), rb)
        for w in (eng, ref):
            w.iterate([1] * 2)
        assert_identical(eng, ref, what="appended after a late reserve")
    assert eng.layout_stats() == (2, 1) and eng.append_stats() == (2, 2, 0)


# ---- 7. mirror coherence ---------------------------------------------------------------------------------------------------------
def test_reads_and_a_later_full_layout_see_the_appended_robots():
    sc = _lanes(16, 5)
    eng, ref = _reserved_pair(sc, 3, 8)
    for w in (eng, ref):
        w.iterate([1] * 3)
    _add((eng, ref), sc["robots"][3])
    assert_identical(eng, ref, what="right after add_robot")
    assert _counts(eng, 4) == _counts(ref, 4)
    for w in (eng, ref):
        w.iterate([1])
    assert_identical(eng, ref, what="one sweep later")
    assert _counts(eng, 4) == _counts(ref, 4)
    for w in (eng, ref):
        w.remove_robot(1)
    _add((eng, ref), sc["robots"][4])
    for w in (eng, ref):
        w.iterate([1] * 2)
    assert_identical(eng, ref, what="an old robot removed, another appended")
    assert eng.layout_stats() == (1, 0) and eng.append_stats() == (2, 2, 0)
    for w in (eng, ref):
        w.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
        w.iterate([1] * 2)
    assert_identical(eng, ref, what="laid out in full from the pulled mirror")
    assert eng.layout_stats() == (2, 1)
    assert _counts(eng, 5) == _counts(ref, 5)


# ---- 8. lingering ------------------------------------------------------------------------------------------------------------------
def test_append_between_two_lingering_ticks():
    full = S.grid_scenario(6, 16, interrobot=True, pitch=2.0, comm_radius=5.0)
    sc = _first(full, 5)
    eng, ref = World(sc["params"]), oracle.OracleWorld(sc["params"])
    eng.reserve(8)
    assert S.populate(eng, sc) == S.populate(ref, sc)
    eng.set_linger(20000)  # (a bound no host jitter reaches)
    tick5, tick6 = S.tick_inputs(sc), S.tick_inputs(full)
    for _ in range(3):
        eng.tick(steps=sc["steps"], **tick5)
    for _ in range(3):
        ref.tick(steps=sc["steps"], **tick5)
    launches, posts, reruns, _ = eng.linger_stats()
    assert launches == 1 and posts + reruns == 2
    _add((eng, ref), full["robots"][5])  # (ends the launch)
    for _ in range(3):
        eng.tick(steps=full["steps"], **tick6)
    for _ in range(3):
        ref.tick(steps=full["steps"], **tick6)
    launches2, posts2, reruns2, _ = eng.linger_stats()
    assert launches2 == 2 and posts2 + reruns2 == 4 and posts2 > posts, (launches2, posts2, reruns2)
    assert eng.last_sweep()[2] in (1, 2)
    assert_identical(eng, ref, what="three ticks, a robot, three ticks")
    assert eng.layout_stats() == (1, 0) and eng.append_stats() == (1, 1, 0)
    assert _counts(eng, 6) == _counts(ref, 6)


# ---- 9. device missions with spawns --------------------------------------------------------------------------------------------
def test_junction_twoway_spawns_in_place():
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)["Junction Twoway"]
    p = config.world_params(sc["config"])
    a, b = sim.Simulation(sc, World(p)), sim.Simulation(sc, oracle.OracleWorld(p))
    assert a.dev
    spawn_ticks, pulls_at = [], []
    for t in range(90):
        before = len(a.robots)
        a.tick()
        b.tick()
        if len(a.robots) > before:
            spawn_ticks.append(t)
        pulls_at.append(a.w.layout_stats()[1])
    assert len(spawn_ticks) >= 3, spawn_ticks
    assert len(a.robots) == len(b.robots)
    assert np.array_equal(a.translation, b.translation)
    for x, y in zip(a.w.read_beliefs(), b.w.read_beliefs()):
        assert np.array_equal(x, y)
    assert a.events == b.events
    assert json.dumps(a.export(), sort_keys=True) == json.dumps(b.export(), sort_keys=True)
    assert a.w.layout_stats()[1] == pulls_at[spawn_ticks[1]], (pulls_at[spawn_ticks[1]], a.w.layout_stats(), spawn_ticks)
    assert a.w.append_stats()[0] >= 2 and a.w.append_stats()[2] == 0, a.w.append_stats()


# ---- 10. robots that join while a factor kind is switched off (found by tests/test_gpu_script_fuzz.py) ---------------------------
def _joins_while_off(kind):
    """five robots iterate, `kind` goes off, a sixth joins (its factors of that kind are created switched off: they take no
    message, not even the one that fills their inbox with keys — factorgraph.rs:304-330, factor/mod.rs:307-310), the kind
    comes back: beliefs and message counts after every step"""
    full = S.grid_scenario(6, 10, interrobot=True, seed=3, pitch=2.5, comm_radius=4.5)
    sc = _first(full, 5)
    eng, ref = World(sc["params"]), oracle.OracleWorld(sc["params"])
    assert S.populate(eng, sc) == S.populate(ref, sc)
    mask = sc["params"]["enable_mask"]
    for w in (eng, ref):
        w.iterate([3, 3])
        w.set_enabled(mask & ~kind)
        w.iterate([3])
    assert_identical(eng, ref, what="kind off")
    _add((eng, ref), full["robots"][5])
    for w in (eng, ref):
        w.iterate([3])
    assert_identical(eng, ref, what="joined while the kind is off")
    assert _counts(eng, 6) == _counts(ref, 6)
    for w in (eng, ref):
        w.set_enabled(mask)
        w.iterate([1])
    assert_identical(eng, ref, what="kind on again, one internal iteration")
    assert _counts(eng, 6) == _counts(ref, 6)
    for w in (eng, ref):
        w.iterate([3, 3])
    assert_identical(eng, ref, what="two more")
    assert _counts(eng, 6) == _counts(ref, 6)


def test_a_robot_joins_while_dynamics_factors_are_off():
    _joins_while_off(S.EN_DYN)


def test_a_robot_joins_while_obstacle_factors_are_off():
    _joins_while_off(S.EN_OBS)


def test_a_robot_joins_while_interrobot_factors_are_off():
    _joins_while_off(S.EN_IR)
