"""The global planner on the device (mgx_planner.hip, mgx_plan_paths) against the host restatement of its specification
(magics_amd/global_planner.py), bit for bit: status, node count, iterations, cost, stream state, every path point and the whole
tree — in both libraries, for the reference's far sampler and for a dense one, wherever the launches' slices fall."""
import ctypes
import os
import struct

import numpy as np
import pytest

from magics_amd import World, config, hostlib, scenarios
from magics_amd import global_planner as gp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLO_GP = os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP")
F = np.float32

# sample_half_extent = 2000, the reference's sampler: the tree grows by full steps towards far samples, as spikes from its hull, so
# a goal is only met where a spike happens to pass.  These goals lie 4 m beyond a node that the seed's own tree grows after more
# than 256 others (found with the restatement); the starts stand beside the map's outer walls, which turn part of the growth away.
FAR = [((-140.0, 0.0), (-41.1, -352.69), 11), ((-87.5, -95.0), (-93.15, -426.55), 12), ((140.0, 30.0), (512.92, 394.86), 13)]
# sample_half_extent = 125, about the map's half width: samples fall inside the tree's reach, neighbourhoods are dense
# (the first is the scenario's own request)
DENSE = [((-87.5, -70.0), (106.25, 49.875), 7), ((106.25, 49.875), (-87.5, -70.0), 8), ((-87.5, 50.0), (106.25, 49.875), 15),
         ((85.0, 25.0), (-87.5, -50.0), 16)]


def _bits(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def solo():
    sc = config.load_scenario(SOLO_GP)
    return sc["environment"], gp.params_from_config(sc["config"], max_iterations=20000, smoothing_max_iterations=60)


@pytest.fixture(scope="module")
def expected(solo):
    """the restatement's results, computed once: name -> (params, requests, results)"""
    env, p = solo
    out = {}
    for name, reqs, h in (("far", FAR, 2000.0), ("dense", DENSE, 125.0)):
        q = dict(p, sample_half_extent=h)
        out[name] = (q, reqs, gp.plan_paths(env, reqs, q))
    return out


def _world(fma=None):
    return World(scenarios.JUNCTION_PARAMS, fma=fma)


def _same(dev, tree, ref):
    assert dev["status"] == ref["status"]
    assert (dev["n_nodes"], dev["iterations"]) == (ref["n_nodes"], ref["iterations"])
    assert _bits(dev["cost"]) == _bits(ref["cost"])
    assert dev["wyrand_state"] == ref["wyrand_state"]
    assert dev["path"].dtype == F and dev["path"].tobytes() == ref["path"].tobytes()
    if tree is not None:
        xy, parent, cost = tree
        assert xy.tobytes() == ref["tree"][0].tobytes()
        assert np.array_equal(parent, ref["tree"][1])
        assert cost.tobytes() == ref["tree"][2].tobytes()


def _plan(w, env, p, reqs):
    w.planner_enable(env, p)
    res = w.plan_paths(reqs)
    return res, [w.plan_tree(i) for i in range(len(reqs))]


def test_the_far_cases_grow_large_trees(expected):
    """the reference's sampler: growth by full steps, rewires rare; more than 256 nodes, so that the strided loops run more than
    once and the reduction crosses the waves"""
    for r in expected["far"][2]:
        assert r["status"] == gp.PLAN_OK and r["n_nodes"] > 256 and len(r["path"]) >= 2
        assert r["rewires"] * 10 < r["n_nodes"]
        assert r["iterations"] > r["n_nodes"] - 1  # (some steered points met the walls)


def test_the_dense_cases_rewire(expected):
    assert max(r["n_nodes"] for r in expected["dense"][2]) > 256
    for r in expected["dense"][2]:
        assert r["status"] == gp.PLAN_OK
        assert r["rewires"] * 10 >= r["n_nodes"]
        assert len(r["path"]) < len(r["unsmoothed"])  # (the smoothing pass took a chord)


@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
@pytest.mark.parametrize("which", ["far", "dense"])
def test_device_equals_the_restatement(solo, expected, which, fma):
    p, reqs, ref = expected[which]
    res, trees = _plan(_world(fma), solo[0], p, reqs)
    assert len(res) == len(reqs) >= 3
    for d, t, r in zip(res, trees, ref):
        _same(d, t, r)


@pytest.mark.parametrize("slice_", [1, 7, 1024])
def test_slices_do_not_show(solo, expected, slice_):
    p, reqs, ref = expected["dense"]
    res, trees = _plan(_world(), solo[0], dict(p, iterations_per_launch=slice_), reqs)
    for d, t, r in zip(res, trees, ref):
        _same(d, t, r)


def test_failures_match_the_restatement(solo, expected):
    env = solo[0]
    p, reqs, _ = expected["dense"]
    w = _world()
    for q, status in ((dict(p, max_iterations=50), gp.PLAN_MAX_ITERATIONS), (dict(p, max_nodes=16), gp.PLAN_TREE_FULL)):
        ref = gp.plan_paths(env, reqs, q)
        assert all(r["status"] == status and len(r["path"]) == 0 for r in ref)
        res, trees = _plan(w, env, q, reqs)
        for d, t, r in zip(res, trees, ref):
            _same(d, t, r)
    # one request that fails among requests that do not
    q = dict(p, max_iterations=2400)
    ref = gp.plan_paths(env, reqs, q)
    assert sorted({r["status"] for r in ref}) == [gp.PLAN_OK, gp.PLAN_MAX_ITERATIONS]
    res, trees = _plan(w, env, q, reqs)
    for d, t, r in zip(res, trees, ref):
        _same(d, t, r)


def test_a_refused_call_changes_nothing(solo, expected):
    p, reqs, ref = expected["dense"]
    w = _world()
    with pytest.raises(hostlib.MgxError, match="planner is off"):
        w.plan_paths(reqs)
    w.planner_enable(solo[0], p)
    req = np.zeros(len(reqs), hostlib.plan_request_dtype())
    for i, (s, e, seed) in enumerate(reqs):
        req["start"][i], req["end"][i], req["wyrand_state"][i] = s, e, seed
    total = sum(len(r["path"]) for r in ref)
    # room for one point less than the paths have: the counts come back, no point does
    rc, res, xy, n = w.plan_paths_raw(req, total - 1)
    assert rc == -1 and n == total and np.isnan(xy).all()
    assert [int(x) for x in res["n_points"]] == [len(r["path"]) for r in ref]
    assert [int(x) for x in res["first_point"]] == [int(x) for x in np.cumsum([0] + [len(r["path"]) for r in ref[:-1]])]
    assert [int(x) for x in res["status"]] == [r["status"] for r in ref]
    # a start that is not finite: nothing is written, and the trees of the call before are still there
    before = w.plan_tree(1)
    bad = req.copy()
    bad["start"][2][1] = np.inf
    res = np.frombuffer(bytes([0x55]) * (len(req) * hostlib.plan_result_dtype().itemsize), hostlib.plan_result_dtype()).copy()
    xy = np.full((total, 2), np.nan, F)
    cnt = ctypes.c_uint32(12345)
    rc = w._L.mgx_plan_paths(w._w, len(bad), bad.ctypes.data, res.ctypes.data, xy.ctypes.data, total, ctypes.byref(cnt))
    assert rc == -1 and cnt.value == 12345 and np.isnan(xy).all() and (res.view(np.uint8) == 0x55).all()
    assert rc == -1 and b"not finite" in w._L.mgx_last_error()
    after = w.plan_tree(1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    assert w._L.mgx_plan_paths(w._w, len(req), None, res.ctypes.data, xy.ctypes.data, total, ctypes.byref(cnt)) == -1
    assert w._L.mgx_plan_paths(w._w, len(req), req.ctypes.data, res.ctypes.data, None, total, ctypes.byref(cnt)) == -1
    # and with room the same call goes through
    rc, res, xy, n = w.plan_paths_raw(req, total)
    assert rc == 0 and n == total and xy.tobytes() == np.concatenate([r["path"] for r in ref]).tobytes()
    w.planner_enable(None)
    with pytest.raises(hostlib.MgxError, match="planner is off"):
        w.plan_paths(reqs)


def test_a_world_with_ghosts_is_refused(solo, expected):
    p, reqs, _ = expected["dense"]
    w = _world()
    mean0, prior, dt = scenarios.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), scenarios.timesteps_for_K(10), 1.0, 5.0, 5.0)
    w.add_robot(mean0, prior, dt, 1.0)
    w.planner_enable(solo[0], p)
    w.add_robot(mean0, prior, dt, 1.0, ghost=True)
    with pytest.raises(hostlib.MgxError, match="unsharded"):
        w.plan_paths(reqs[:1])


def test_beside_the_environment_pass_and_the_layout(solo, expected):
    """the planner holds its own copy of the map: the robot-environment pass logs what it logs without it, and a plan neither lays
    the world's arrays out again nor pulls them"""
    env = solo[0]
    p, reqs, ref = expected["dense"]
    sc = scenarios.grid_scenario(4, 10, interrobot=True, comm_radius=8.0)
    rng = np.random.default_rng(3)
    n = len(sc["robots"])
    passes = [np.stack([rng.uniform(-130, 130, n), np.full(n, -1.5), rng.uniform(-95, 95, n)], axis=1).astype(F) for _ in range(4)]
    logs = []
    for planner in (False, True):
        w = World(sc["params"])
        scenarios.populate(w, sc)
        w.iterate(sc["steps"])
        w.env_collisions_enable(env)
        if planner:
            w.planner_enable(env, p)
        stats = w.layout_stats()
        for k, pos in enumerate(passes):
            w.env_collisions_update(pos)
            if planner and k == 1:
                res = w.plan_paths(reqs[:1])
                _same(res[0], w.plan_tree(0), ref[0])
        ev, total, dropped, per = w.env_collisions_read()
        assert total > 0 and dropped == 0
        logs.append((ev.tobytes(), total, per.tobytes()))
        w.iterate(sc["steps"])
        assert w.layout_stats() == stats
        if planner:
            w.env_collisions_enable(None)      # either goes without the other
            _same(w.plan_paths(reqs[:1])[0], None, ref[0])
    assert logs[0] == logs[1]


# ---- the call is the pool driven to the end: one block of as many slots as the largest call so far (Planner::call) ---------------
def test_calls_grow_and_shrink(solo, expected):
    """1, then 4, then 2 requests on one world: the pool of the call is built again for the larger call and keeps its size for the
    smaller one; a request's tree is found through the slot it got, and only the last call's requests have one"""
    p, reqs, ref = expected["dense"]
    w = _world()
    w.planner_enable(solo[0], p)
    for n in (1, 4, 2):
        res = w.plan_paths(reqs[:n])
        assert len(res) == n
        for i in range(n):
            _same(res[i], w.plan_tree(i), ref[i])
    with pytest.raises(hostlib.MgxError, match="request 2: the last mgx_plan_paths had 2"):
        w.plan_tree(2)
    assert w.plan_paths([]) == []
    with pytest.raises(hostlib.MgxError, match="request 0: the last mgx_plan_paths had 0"):
        w.plan_tree(0)


def test_more_requests_than_a_block_of_the_riding_pool(solo, expected):
    """20 requests, more than the 16 slots of a block of the pool that rides the stream: the call's pool is one block of 20"""
    p = dict(expected["dense"][0], max_iterations=300)
    reqs = [(DENSE[i % len(DENSE)][0], DENSE[i % len(DENSE)][1], 100 + i) for i in range(20)]
    ref = gp.plan_paths(solo[0], reqs, p)
    res, trees = _plan(_world(), solo[0], p, reqs)
    assert len(res) == len(ref) == 20
    for d, t, r in zip(res, trees, ref):
        assert d["status"] == r["status"] == gp.PLAN_MAX_ITERATIONS
        _same(d, t, r)


def test_a_call_does_not_disturb_pending_requests(solo, expected):
    """the call has a pool of its own: what rides the stream keeps its tickets and its slice numbers, and is not advanced"""
    p, reqs, ref = expected["dense"]
    w = _world()
    w.planner_enable(solo[0], p)
    assert w.plan_submit(reqs[:2]) == [1, 2]
    for _ in range(2):
        w.plan_advance(7)
    res = w.plan_paths(reqs[2:])  # (iterations_per_launch is the default, 1024)
    assert p["iterations_per_launch"] in (0, 1024) and w.plan_pending() == 2
    for i, d in enumerate(res):
        _same(d, w.plan_tree(i), ref[2 + i])
    want = {1 + i: gp.slices_needed(ref[i], p, 7) for i in range(2)}
    assert min(want.values()) > 2
    got = []
    for _ in range(max(want.values()) - 2):
        w.plan_advance(7)
        got += w.plan_collect(wait=True)
    assert w.plan_pending() == 0 and {d["ticket"]: d["slices"] for d in got} == want
    for d in got:
        _same(d, None, ref[d["ticket"] - 1])
    assert w.plan_submit(reqs[:1]) == [3]


def test_a_call_too_large_to_allocate_leaves_smaller_calls_working(solo, expected):
    """2^20 requests with trees of 8192 nodes ask for 300 GB in one allocation: the call is refused with the runtime's error, the
    pool it tried to build is gone, and the same world plans a small call afterwards (as the caller's retry in batches would)"""
    p, reqs, ref = expected["dense"]
    w = _world()
    w.planner_enable(solo[0], dict(p, max_nodes=8192))
    _same(w.plan_paths(reqs[:1])[0], w.plan_tree(0), ref[0])
    req = np.zeros(1 << 20, hostlib.plan_request_dtype())
    req["wyrand_state"] = 1
    rc, _, _, _ = w.plan_paths_raw(req, 1)
    assert rc < 0 and b"hipMalloc" in w._L.mgx_last_error()
    with pytest.raises(hostlib.MgxError, match="the last mgx_plan_paths had 0"):
        w.plan_tree(0)
    res = w.plan_paths(reqs[:2])
    for i in range(2):
        _same(res[i], w.plan_tree(i), ref[i])
