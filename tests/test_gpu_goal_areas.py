"""Goal areas on the device (mgx_goal_areas_*, magics_amd/csrc/mgx_goal_areas.hip) against the answers written out by hand in
tests/test_goal_areas.py and the numpy restatement `sim.goal_area_contacts`: the table of first arrivals cell for cell in both
libraries, first arrivals that stick, robots that join (appended in place and through a relayout), the mission chain tick by
tick, many ticks per call and against the host pass, and switched off."""
import ctypes
import json
import os

import numpy as np
import pytest

from magics_amd import World, config, hostlib, scenarios as S, sim

from test_goal_areas import JUNCTION, JUNCTION_TICKS, KNOWN
from test_gpu_spawn_in_place import _first, _lanes

pytestmark = pytest.mark.gpu
F = np.float32
STATE = -4  # MGX_ERR_STATE
BOX_A, BOX_JUNCTION, BOX_POINT, BOX_BOTH = ((-8, -4), (8, 4)), ((-8, -48), (8, -52)), ((2, 3), (2, 3)), ((8, -48), (-8, -52))


def _add(w, radius, ghost=False):
    mean0, prior, dt = S.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), S.timesteps_for_K(10), 1.0, 5.0, 5.0)
    return w.add_robot(mean0, prior, dt, float(radius), ghost=ghost)


def _xyz(points):
    pos = np.zeros((len(points), 3), F)
    pos[:, 0], pos[:, 1], pos[:, 2] = [p[0] for p in points], -1.5, [p[1] for p in points]
    return pos


def _table(w, n_areas, n_robots):
    """the device's table as [robots, areas] ticks (-1: never), checked against what else the read says"""
    arrivals, per_area = w.goal_areas_read()
    t = np.full((n_robots, n_areas), -1, np.int64)
    for e in arrivals:
        assert t[int(e["robot"]), int(e["area"])] == -1
        t[int(e["robot"]), int(e["area"])] = int(e["tick"])
    keys = [(int(e["tick"]), int(e["robot"]), int(e["area"])) for e in arrivals]
    assert keys == sorted(keys) and int(per_area.sum()) == len(arrivals)
    assert per_area.tolist() == [(t[:, a] >= 0).sum() for a in range(n_areas)]
    return t


def _many_areas():
    """the four boxes of the known answers and sixty more, small and large, some of them around the known positions"""
    rng = np.random.default_rng(64)
    boxes = [BOX_A, BOX_JUNCTION, BOX_POINT, BOX_BOTH]
    while len(boxes) < hostlib.GOAL_AREAS_MAX:
        c, h = rng.uniform(-14, 14, 2) + (0, -25 if len(boxes) % 3 == 0 else 0), rng.uniform(0, 6, 2)
        boxes.append(((float(F(c[0] - h[0])), float(F(c[1] + h[1]))), (float(F(c[0] + h[0])), float(F(c[1] - h[1])))))
    return boxes


# ---- 1. the pass over handed-in positions against the known answers ---------------------------------------------------------------
@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
@pytest.mark.parametrize("n_areas", [3, 64])
def test_update_against_the_known_answers(fma, n_areas):
    # mgx_robot_add refuses a radius that is not positive: the known answers with r = 0 and r = NaN are the host's alone
    cases = [k for k in KNOWN if k[3] > 0]
    assert len(cases) == len(KNOWN) - 3 and sum(1 for k in cases if np.isnan(k[2]).any()) == 2
    n, gone = 70, (1, 33, 64)
    pos, rad = [(10000.0 + 3 * i, -10000.0) for i in range(n)], [1.0] * n
    where = list(range(0, 26, 2)) + list(range(70 - (len(cases) - 13), 70))      # the first wave, and the ragged tail of the second
    for i, k in zip(where, cases):
        pos[i], rad[i] = k[2], float(k[3])
    for i in gone:                                                               # removed robots that would touch
        assert i not in where
        pos[i], rad[i] = (1.5, -2.0), 1.0
    w = World(S.JUNCTION_PARAMS, fma=fma)
    with pytest.raises(hostlib.MgxError, match="radius must be positive"):
        _add(w, float("nan"))
    for r in rad:
        _add(w, r)
    for i in gone:
        w.remove_robot(i)
    areas = [BOX_A, BOX_JUNCTION, BOX_POINT] if n_areas == 3 else _many_areas()
    w.goal_areas_enable(areas, next_tick=0)
    w.goal_areas_update(5, _xyz(pos))
    got = _table(w, n_areas, n)
    want = sim.goal_area_contacts(areas, np.array(pos, dtype=F), np.array(rad, dtype=F))
    # the known answers themselves, on the device: every case against its own box
    checked = 0
    for i, k in zip(where, cases):
        if k[1] in areas:
            assert bool(got[i, areas.index(k[1])] == 5) == k[4], k[0]
            checked += 1
    assert checked == (len(cases) if n_areas == 64 else len(cases) - 1)
    want[list(gone)] = False
    assert want[:, 0].sum() >= 6 and (n_areas == 3 or want[:, 4:].sum() >= 20)
    assert np.array_equal(got >= 0, want) and set(np.unique(got)) == {-1, 5}
    assert not (got[list(gone)] >= 0).any() and not (got[[i for i, k in zip(where, cases) if np.isnan(k[2]).any()]] >= 0).any()


# ---- 2. the first arrival sticks ----------------------------------------------------------------------------------------------------
def test_first_arrival_sticks_and_clear_forgets():
    w = World(S.JUNCTION_PARAMS)
    for _ in range(3):
        _add(w, 1.0)
    w.goal_areas_enable([BOX_A, ((-8, -4), (100, 4))], next_tick=0)
    inside, away, second = (0.0, 0.0), (0.0, 50.0), (50.0, 0.0)
    for tick in range(12):
        p0 = inside if tick in (3, 7, 9) else away
        p1 = second if tick >= 2 else away                  # robot 1: area 1 only, from tick 2 on
        p2 = inside if tick == 3 else away                  # robot 2: both areas in the pass of tick 3, like robot 0
        w.goal_areas_update(tick, _xyz([p0, p1, p2]))
        if tick == 8:
            arrivals, per_area = w.goal_areas_read()
            assert [(int(e["tick"]), int(e["robot"]), int(e["area"])) for e in arrivals] == [(2, 1, 1), (3, 0, 0), (3, 0, 1), (3, 2, 0), (3, 2, 1)]
            assert per_area.tolist() == [2, 3]
            w.goal_areas_clear()
            assert len(w.goal_areas_read()[0]) == 0
    arrivals, per_area = w.goal_areas_read()
    assert [(int(e["tick"]), int(e["robot"]), int(e["area"])) for e in arrivals] == [(9, 0, 0), (9, 0, 1), (9, 1, 1)]
    assert per_area.tolist() == [1, 2]
    # the size first; too little room is an error that still says how much there is
    L, tot = hostlib.lib(), ctypes.c_uint64()
    buf = np.zeros(2, hostlib.goal_arrival_dtype())
    assert L.mgx_goal_areas_read(w._w, buf.ctypes.data, 2, ctypes.byref(tot), None) == -1 and tot.value == 3
    assert L.mgx_goal_areas_update(w._w, None, 2**32 - 1) == -1 and L.mgx_goal_areas_set_clock(w._w, 2**32 - 1) == -1
    with pytest.raises(hostlib.MgxError, match="the goal areas are on"):
        w.goal_areas_enable([BOX_A])
    w.goal_areas_enable(None)
    assert L.mgx_goal_areas_clear(w._w) == STATE


# ---- 3. head-room and append -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [8, 0], ids=["appended", "relayout"])
def test_robots_that_join_keep_the_others_arrivals(reserve):
    sc = _lanes(5, 5)
    w = World(sc["params"])
    if reserve:
        w.reserve(reserve)
    S.populate(w, _first(sc, 3))
    w.iterate(sc["steps"])
    w.goal_areas_enable([BOX_A, BOX_JUNCTION], next_tick=0)
    away = (500.0, 500.0)
    w.goal_areas_update(4, _xyz([(0.0, 0.0), away, (0.0, -50.0)]))
    before = _table(w, 2, 3)
    assert before.tolist() == [[4, -1], [-1, -1], [-1, 4]]
    stats = w.layout_stats(), w.append_stats()
    for rb in sc["robots"][3:]:
        w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=rb["order_key"])
    w.iterate([1])
    if reserve:
        assert w.layout_stats() == stats[0] and w.append_stats() == (stats[1][0] + 1, stats[1][1] + 2, 0)
    else:
        assert w.layout_stats() == (stats[0][0] + 1, stats[0][1] + 1) and w.append_stats()[:2] == (0, 0)
    assert _table(w, 2, 5)[:3].tolist() == before.tolist() and (_table(w, 2, 5)[3:] == -1).all()
    w.goal_areas_update(6, _xyz([(0.0, -50.0), (0.0, 0.0), (0.0, -50.0), (0.0, -50.0), away]))
    assert _table(w, 2, 5).tolist() == [[4, 6], [6, -1], [-1, 4], [-1, 6], [-1, -1]]


def test_more_robots_than_the_rows_hold():
    """robots beyond the table's head-room: longer rows, the arrivals so far copied row by row"""
    w = World(S.JUNCTION_PARAMS)
    for _ in range(100):
        _add(w, 1.0)
    w.goal_areas_enable([BOX_A, BOX_JUNCTION, BOX_POINT], next_tick=0)
    away = (500.0, 500.0)
    w.goal_areas_update(1, _xyz([(0.0, 0.0) if i % 7 == 0 else (0.0, -50.0) if i % 7 == 3 else away for i in range(100)]))
    before = _table(w, 3, 100)
    assert (before[:, 0] >= 0).sum() == 15 and (before[:, 1] >= 0).sum() == 14 and (before[:, 2] >= 0).sum() == 0
    for _ in range(150):
        _add(w, 1.0)
    assert np.array_equal(_table(w, 3, 250)[:100], before)
    w.goal_areas_update(2, _xyz([(2.0, 3.0) if i in (5, 99, 100, 249) else away for i in range(250)]))
    after = _table(w, 3, 250)
    assert np.array_equal(after[:100, 1], before[:, 1]) and (after[100:, 1] == -1).all()
    assert np.array_equal(np.delete(after[:100, 0], [5, 99]), np.delete(before[:, 0], [5, 99])) and (before[[5, 99], 0] == -1).all()
    assert np.nonzero(after[:, 0] == 2)[0].tolist() == [5, 99, 100, 249] == np.nonzero(after[:, 2] == 2)[0].tolist()


# ---- 4. the mission chain ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def junction_runs():
    sc = config.load_scenario(JUNCTION)

    def run(chunk, **kw):
        s = sim.Simulation(sc, World(config.world_params(sc["config"])), **kw)
        s.run(max_ticks=JUNCTION_TICKS, chunk=chunk)
        assert s.tick_no == JUNCTION_TICKS and s.dev
        return s, s.export()
    return {"ticks": run(1, goal_areas="junction"), "chunks": run(256, goal_areas="junction"),
            "host": run(1, goal_areas="junction", device_goal_areas=False), "none": run(1)}


def test_the_mission_chain_three_ways(junction_runs):
    (s, exp), (s_c, exp_c), (s_h, exp_h), (s_n, exp_n) = (junction_runs[k] for k in ("ticks", "chunks", "host", "none"))
    assert s._dev_goals and s_c._dev_goals and not s_h._dev_goals and s_h._host_needs_transforms() and not s._host_needs_transforms()
    ga = exp["goal_areas"]
    assert json.dumps(ga, sort_keys=True) == json.dumps(exp_c["goal_areas"], sort_keys=True) == json.dumps(exp_h["goal_areas"], sort_keys=True)
    n = [len(a["history"]) for a in ga.values()]
    assert list(ga) == ["0", "1"] and sum(n) >= 4 and min(n) >= 1, n
    assert all(rid in exp["robots"] and t >= exp["robots"][rid]["mission"]["started_at"] for a in ga.values() for rid, t in a["history"].items())
    # robots that were despawned after arriving keep their entries
    assert any(not s.robots[int(rid)]["alive"] for a in ga.values() for rid in a["history"])
    # the trajectories are untouched
    assert exp_n["goal_areas"] == {} and "goal_areas" not in s_n.metrics()
    for other in (exp, exp_c, exp_h):
        assert {k: v["positions"] for k, v in other["robots"].items()} == {k: v["positions"] for k, v in exp_n["robots"].items()}
    m = s.metrics()["goal_areas"]
    assert m == s_c.metrics()["goal_areas"] == s_h.metrics()["goal_areas"] and m["arrivals"] == n and m["flow"] == sim.goal_flow(exp)


# ---- 5. off means off --------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    L = hostlib.lib()
    sc = config.load_scenario(JUNCTION)
    on = sim.Simulation(sc, World(config.world_params(sc["config"])), goal_areas="junction")
    off = sim.Simulation(sc, World(config.world_params(sc["config"])))
    n = ctypes.c_uint64()
    assert L.mgx_goal_areas_read(off.w._w, None, 0, ctypes.byref(n), None) == STATE
    assert L.mgx_goal_areas_update(off.w._w, None, 0) == STATE and L.mgx_goal_areas_clear(off.w._w) == STATE
    assert L.mgx_goal_areas_set_clock(off.w._w, 0) == STATE
    for t in range(12):
        on.tick()
        off.tick()
        assert on.w.last_sweep() == off.w.last_sweep(), t
        assert on.w.last_launch_count() == off.w.last_launch_count(), t
    assert len(on.robots) >= 2
    for x, y in zip(on.w.read_beliefs(), off.w.read_beliefs()):
        assert np.array_equal(x, y)
    assert np.array_equal(on.translation, off.translation)
    # a world with ghosts refuses
    w = World(S.JUNCTION_PARAMS)
    _add(w, 1.0)
    _add(w, 1.0, ghost=True)
    with pytest.raises(hostlib.MgxError, match="unsharded"):
        w.goal_areas_enable([BOX_A])
    assert L.mgx_goal_areas_clear(w._w) == STATE
