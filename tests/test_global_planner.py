"""The global planner's specification (include/mgx.h, "global planner") as magics_amd/global_planner.py restates it on the host:
the properties a plan has by construction, the failures, and the binding of the new entry points.  The device planner is checked
against this restatement bit for bit in tests/test_gpu_planner.py."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

from magics_amd import config, hostlib
from magics_amd import global_planner as gp
from magics_amd.prng import WyRand
from magics_amd.sim import environment_contacts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLO_GP = os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP")
# the scenario's own request (formation.yaml on the 250 x 175 map) and a sampler about as wide as the map
START, END = (-87.5, -70.0), (106.25, 49.875)


@pytest.fixture(scope="module")
def solo():
    sc = config.load_scenario(SOLO_GP)
    p = gp.params_from_config(sc["config"], sample_half_extent=125.0, max_iterations=20000, smoothing_max_iterations=60)
    return sc["environment"], p


@pytest.fixture(scope="module")
def plans(solo):
    """(planner, smoothed plan, the same request without smoothing) on the Solo GP map, on a map without colliders, and on Solo GP
    with a neighbourhood no wider than a step ("tight")"""
    env, p = solo
    out = {}
    for name, e, q in (("solo", env, p), ("free", None, p), ("tight", env, dict(p, neighbourhood_radius=p["step_size"]))):
        pl = gp.Planner(e, q)
        raw = gp.Planner(e, dict(q, smoothing_enabled=False))
        out[name] = (pl, pl.plan(START, END, 7), raw.plan(START, END, 7))
    return out


def test_uniform_bit_patterns():
    h = 2000.0
    assert gp.uniform_from_u64(0, h) == -h
    top = struct.unpack("<d", struct.pack("<Q", 0x3FFFFFFFFFFFFFFF))[0] - 1.0
    assert top == 1.0 - 2.0 ** -52
    assert gp.uniform_from_u64(2 ** 64 - 1, h) == top * (2.0 * h) - h

    class Fixed(WyRand):
        def next_u64(self):
            return 2 ** 64 - 1
    assert gp.uniform(Fixed(0), 125.0) == (1.0 - 2.0 ** -52) * 250.0 - 125.0


@pytest.mark.parametrize("name", ["solo", "free", "tight"])
def test_plan_properties(plans, solo, name):
    pl, res, raw = plans[name]
    step, radius = pl.p["step_size"], pl.p["neighbourhood_radius"]
    assert res["status"] == gp.PLAN_OK and raw["status"] == gp.PLAN_OK
    path = res["path"]
    assert path.dtype == np.float32 and len(path) >= 2
    assert tuple(path[0]) == tuple(np.float32(START)) and tuple(path[-1]) == tuple(np.float32(END))
    # the tree: every vertex but the root is feasible under environment_contacts
    xy, parent, cost = res["tree"]
    assert len(xy) == res["n_nodes"] > 1 and parent[0] == -1 and cost[0] == 0.0
    if len(pl.colliders):
        rad = np.full(len(xy) - 1, solo[1]["collision_radius"], np.float32)
        assert not environment_contacts(pl.colliders, pl.vertices, xy[1:].astype(np.float32), rad).any()
    # stored costs strictly decrease along every parent chain: extraction ends within n_nodes steps
    kids = np.arange(1, len(xy))
    assert (parent[kids] >= 0).all() and (parent[kids] < len(xy)).all()
    assert (cost[parent[kids]] < cost[kids]).all()
    # growth is the same with and without smoothing.  A node is created within one step of its nearest node, and the goal test
    # keeps the last hop within one step; its PARENT is the cheapest node of the neighbourhood, so a hop is at most
    # max(step, neighbourhood_radius): one step where the neighbourhood is no wider than that ("tight").  In f64 the steered
    # point misses the step by a few ulps of the coordinates (~1e-14 relative): 1e-12 covers it
    assert raw["n_nodes"] == res["n_nodes"] and raw["iterations"] == res["iterations"] and raw["cost"] == res["cost"]
    un = res["unsmoothed"]
    assert np.array_equal(un, raw["path64"]) and np.array_equal(un.astype(np.float32), raw["path"])
    hops = np.hypot(*(un[1:] - un[:-1]).T)
    assert (hops <= max(step, radius) * (1 + 1e-12)).all() and hops[-1] <= step
    if name == "tight":
        assert radius == step and (hops <= step * (1 + 1e-12)).all()
    # the smoothed path is a subsequence of the unsmoothed one, and every chord it took is free
    sm = res["path64"]
    at, j = [], 0
    for pt in sm:
        while not np.array_equal(un[j], pt):
            j += 1
        at.append(j)
        j += 1
    assert at[0] == 0 and at[-1] == len(un) - 1 and len(sm) <= len(un)
    for a, b in zip(sm[:-1], sm[1:]):
        assert pl.feasible(pl.chord_points(tuple(a), tuple(b))).all()
    if name == "free":
        assert len(sm) < len(un)


@pytest.mark.parametrize("name", ["solo", "free"])
def test_stream_state_is_the_draws_made(plans, name):
    _, res, raw = plans[name]
    for r in (res, raw):
        rng = WyRand(7)
        for _ in range(r["draws"]):
            rng.next_u64()
        assert r["wyrand_state"] == rng.state
    assert raw["draws"] == 2 * raw["iterations"] and res["draws"] > raw["draws"]


def test_same_seed_same_plan_other_seed_other_plan(plans, solo):
    pl, res, _ = plans["solo"]
    again, other = pl.plan(START, END, 7), pl.plan(START, END, 8)
    assert again["wyrand_state"] == res["wyrand_state"] and np.array_equal(again["path"], res["path"])
    assert np.array_equal(again["tree"][0], res["tree"][0]) and again["cost"] == res["cost"]
    assert other["status"] == gp.PLAN_OK
    assert other["wyrand_state"] != res["wyrand_state"] and not np.array_equal(other["tree"][0][:8], res["tree"][0][:8])


def test_failures(solo):
    env, p = solo
    r = gp.Planner(env, dict(p, max_iterations=50)).plan(START, END, 7)
    assert r["status"] == gp.PLAN_MAX_ITERATIONS and len(r["path"]) == 0 and r["iterations"] == 50 and r["draws"] == 100
    r = gp.Planner(env, dict(p, max_nodes=16)).plan(START, END, 7)
    assert r["status"] == gp.PLAN_TREE_FULL and len(r["path"]) == 0 and r["n_nodes"] == 16
    with pytest.raises(ValueError):
        gp.Planner(env, dict(p, step_size=0.0))
    with pytest.raises(ValueError):
        gp.Planner(env, dict(p, collision_radius=math.nan))


def test_params_come_from_the_scenario(solo):
    sc = config.load_scenario(SOLO_GP)
    p = gp.params_from_config(sc["config"])
    assert (p["step_size"], p["neighbourhood_radius"], p["collision_radius"], p["max_iterations"]) == (5.0, 8.0, 3.0, 5000000)
    assert p["smoothing_enabled"] and p["smoothing_max_iterations"] == 500
    assert p["smoothing_step"] == p["step_size"]  # rrtstar.rs:60 hands the step size to the smoothing pass


def test_the_scenario_runner_needs_an_engine_world():
    """without the option the strategy is rejected as before; with it, a world without device missions still is"""
    import oracle
    from magics_amd import sim
    sc = config.load_scenario(SOLO_GP)
    with pytest.raises(ValueError):
        sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"])), global_planner="device")
    for mode, what in ((None, "outside the hot path"), (True, "engine world"), ("host", "engine world")):
        s = sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"])), global_planner=mode)
        with pytest.raises(NotImplementedError, match=what):
            s.run(max_ticks=3)


def test_new_symbols_are_exported_and_bound():
    L = ctypes.CDLL(hostlib.LIB_PATH)
    for name in ("mgx_planner_enable", "mgx_plan_paths", "mgx_plan_tree"):
        assert name in hostlib.SYMBOLS and hasattr(L, name), name
    assert ctypes.sizeof(hostlib.PlanParams) == 40
    assert hostlib.plan_request_dtype().itemsize == 24 and hostlib.plan_result_dtype().itemsize == 40
    B = hostlib.lib()
    assert B.mgx_planner_enable(None, None, None) == -1 and b"null" in B.mgx_last_error()
    assert B.mgx_plan_paths(None, 0, None, None, None, 0, None) == -1
    assert B.mgx_plan_tree(None, 0, 0, None, None, None, None) == -1
