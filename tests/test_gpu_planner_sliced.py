"""Plans that ride the stream (mgx_plan_submit / _advance / _collect / _cancel / _pending, mgx_planner_set_tick_budget): requests
wait in a pool, a slice is one enqueued launch, the device reports what ended through a completion log.  Every plan is
mgx_plan_paths' and the host restatement's bit for bit whatever the budget, however submits, advances and collects interleave
and whichever slot a request gets; the slice a request ends in is the header's rule; collect hands out in the order of (slice
number, ticket), each request once; a tick with a budget carries exactly one slice and computes what it computes without a
planner; and the Solo GP scenario run with `global_planner="sliced"` is the synchronous run shifted by the slices its plan took."""

import numpy as np
import pytest

from magics_amd import World, config, hostlib, scenarios as S, sim
from magics_amd import global_planner as gp
from magics_amd.driver import DeviceDriver
from global_paths_common import mission_kwargs
from test_gpu_planner import DENSE, SOLO_GP, _same

pytestmark = pytest.mark.gpu

F = np.float32
NOWHERE = ((-87.5, -70.0), (5000.0, 5000.0), 21)  # a goal no tree reaches
FAIL_ITERATIONS = 96


@pytest.fixture(scope="module")
def solo():
    sc = config.load_scenario(SOLO_GP)
    p = gp.params_from_config(sc["config"], max_iterations=20000, smoothing_max_iterations=60, sample_half_extent=125.0, max_nodes=2048)
    return sc["environment"], p


@pytest.fixture(scope="module")
def expected(solo):
    """the restatement's results, computed once: (the DENSE requests', the failing request's under max_iterations = 96)"""
    env, p = solo
    dense = gp.plan_paths(env, DENSE, p)
    assert all(r["status"] == gp.PLAN_OK and r["n_nodes"] < 2048 for r in dense) and max(r["n_nodes"] for r in dense) > 256
    fail = gp.plan_paths(env, [NOWHERE], dict(p, max_iterations=FAIL_ITERATIONS))[0]
    assert fail["status"] == gp.PLAN_MAX_ITERATIONS and fail["iterations"] == FAIL_ITERATIONS
    return dense, fail


def _world(env=None, p=None, fma=None):
    w = World(S.JUNCTION_PARAMS, fma=fma)
    if env is not None:
        w.planner_enable(env, p)
    return w


def _most(p, budget):
    """no request takes more advances than this"""
    return (p["max_iterations"] + p["smoothing_max_iterations"]) // budget + 2


def _drain(w, p, budget, got=None):
    """advance and collect (waiting) until nothing is pending -> what came, in the order it came"""
    got = [] if got is None else got
    for _ in range(_most(p, budget)):
        if not w.plan_pending():
            break
        w.plan_advance(budget)
        got += w.plan_collect(wait=True)
    assert w.plan_pending() == 0
    return got


def _same_plan(d, ref):
    _same(d, None, ref)
    assert d["smoothing_iterations"] == ref["smoothing_iterations"]


_SYNCHRONOUS = {}


def _synchronous(solo, fma):
    """World.plan_paths of the DENSE requests on a world of its own, once per library"""
    if fma not in _SYNCHRONOUS:
        _SYNCHRONOUS[fma] = _world(solo[0], solo[1], fma).plan_paths(DENSE)
    return _SYNCHRONOUS[fma]


# ---- 1. the same bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
@pytest.mark.parametrize("budget", [7, 64, 1000])
def test_same_bits_as_the_synchronous_call_and_the_restatement(solo, expected, budget, fma):
    env, p = solo
    w = _world(env, p, fma)
    tickets = w.plan_submit(DENSE)
    assert tickets == [1, 2, 3, 4] and w.plan_pending() == 4
    got = {d["ticket"]: d for d in _drain(w, p, budget)}
    assert sorted(got) == tickets
    for t, ref, syn in zip(tickets, expected[0], _synchronous(solo, fma)):
        _same_plan(got[t], ref)
        _same_plan(got[t], dict(syn, tree=None))
    # the request that fails, under its own limit
    q = dict(p, max_iterations=FAIL_ITERATIONS)
    w.planner_enable(env, q)
    (t,) = w.plan_submit([NOWHERE])
    assert t == 5  # (tickets are the world's: a new map does not start them again)
    (d,) = _drain(w, q, budget)
    _same_plan(d, expected[1])
    assert d["ticket"] == 5 and len(d["path"]) == 0


# ---- 2. slice numbers, the order of collect ------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [7, 64])
def test_slice_numbers_and_collect_order(solo, expected, budget):
    env, p = solo
    w = _world(env, p)
    tickets = w.plan_submit(DENSE)
    got = _drain(w, p, budget)
    want = {t: gp.slices_needed(r, p, budget) for t, r in zip(tickets, expected[0])}
    assert {d["ticket"]: d["slices"] for d in got} == want
    assert len(got) == len(tickets) == len({d["ticket"] for d in got})  # nothing twice
    order = [(d["slices"], d["ticket"]) for d in got]
    assert order == sorted(order)
    assert w.plan_collect(wait=True) == [] and w.plan_collect() == []
    # several that end before one collect: still (slices, ticket), and room for one hands out one
    tickets = w.plan_submit(DENSE)
    for _ in range(max(want.values())):
        w.plan_advance(budget)
    first = w.plan_collect(wait=True, capacity=1)
    assert len(first) == 1 and w.plan_pending() == 3
    points = sum(len(r["path"]) for r in expected[0])
    second = w.plan_collect(wait=True, point_capacity=points - len(first[0]["path"]) - 1)  # one point short of the other three
    rest = w.plan_collect()  # (everything has been waited for: what the points had no room for)
    got = first + second + rest
    assert len(second) == 2 and len(rest) == 1 and w.plan_pending() == 0
    order = [(d["slices"], d["ticket"]) for d in got]
    assert order == sorted(order)
    assert {d["ticket"]: d["slices"] for d in got} == {t: gp.slices_needed(r, p, budget) for t, r in zip(tickets, expected[0])}
    for d, ref in zip(sorted(got, key=lambda d: d["ticket"]), expected[0]):
        _same_plan(d, ref)
    # the failing request: max_iterations // B + 1
    q = dict(p, max_iterations=FAIL_ITERATIONS)
    w.planner_enable(env, q)
    w.plan_submit([NOWHERE])
    (d,) = _drain(w, q, budget)
    assert d["slices"] == FAIL_ITERATIONS // budget + 1 == gp.slices_needed(expected[1], q, budget)


# ---- 3. staggered: submits between advances, a second block of slots, slots taken again ----------------------------------------
def test_staggered_submits_grow_the_pool_and_reuse_slots(solo, expected):
    env, p = solo
    budget = 7
    w = _world(env, p)
    which = {}  # ticket -> index into DENSE
    got = []

    def submit(idx):
        for t, i in zip(w.plan_submit([DENSE[i] for i in idx]), idx):
            assert t == len(which) + 1
            which[t] = i

    submit([0, 1])
    for _ in range(3):
        w.plan_advance(budget)
    submit([2, 3, 0])
    w.plan_advance(budget)
    got += w.plan_collect(wait=True)
    submit([1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1])  # 18 pending: more than one block of slots holds, while 5 are under way
    assert w.plan_pending() == 18 - len(got)
    shortest = min(gp.slices_needed(r, p, budget) for r in expected[0])
    for _ in range(shortest + 2):
        w.plan_advance(budget)
        got += w.plan_collect(wait=True)
    assert 0 < len(got) < 18  # some have ended and been collected: their slots are free
    submit([3, 2, 1, 0])     # ... and are taken again under the requests still pending
    _drain(w, p, budget, got)
    assert sorted(d["ticket"] for d in got) == list(range(1, 23))
    for d in got:
        ref = expected[0][which[d["ticket"]]]
        _same_plan(d, ref)
        assert d["slices"] == gp.slices_needed(ref, p, budget), d["ticket"]


# ---- 4. collect that does not wait ---------------------------------------------------------------------------------------------
def test_collect_without_waiting_hands_out_what_waiting_would(solo, expected):
    env, p = solo
    budget = 64
    a, b = _world(env, p), _world(env, p)
    for w in (a, b):
        w.plan_submit(DENSE)
        assert w.plan_collect() == [] and w.plan_collect(wait=True) == []  # before any advance: nothing, and no error
    total = 0
    for _ in range(_most(p, budget)):
        if not b.plan_pending():
            break
        a.plan_advance(budget)
        a.synchronize()
        x = a.plan_collect()
        b.plan_advance(budget)
        y = b.plan_collect(wait=True)
        assert [(d["ticket"], d["slices"], d["status"], d["wyrand_state"], d["path"].tobytes()) for d in x] == \
               [(d["ticket"], d["slices"], d["status"], d["wyrand_state"], d["path"].tobytes()) for d in y]
        total += len(x)
    assert total == 4 and a.plan_pending() == b.plan_pending() == 0


# ---- 5. cancel, errors, the layout ---------------------------------------------------------------------------------------------
def test_cancel_and_errors(solo, expected):
    env, p = solo
    budget = 64
    w = _world()
    with pytest.raises(hostlib.MgxError, match="planner is off"):
        w.plan_submit(DENSE[:1])
    assert w.plan_pending() == 0
    w.planner_enable(env, p)
    tickets = w.plan_submit(DENSE)
    with pytest.raises(hostlib.MgxError, match="0 iterations"):
        w.plan_advance(0)
    bad = list(DENSE[1])
    bad[1] = (float("nan"), 0.0)
    with pytest.raises(hostlib.MgxError, match="not finite"):
        w.plan_submit([DENSE[0], tuple(bad)])
    assert w.plan_pending() == 4  # (nothing of the refused call was queued)
    w.plan_advance(budget)
    w.plan_cancel(tickets[1])     # while it is under way
    assert w.plan_pending() == 3
    with pytest.raises(hostlib.MgxError, match="not pending"):
        w.plan_cancel(tickets[1])
    with pytest.raises(hostlib.MgxError, match="not pending"):
        w.plan_cancel(99)
    with pytest.raises(hostlib.MgxError, match="pending"):
        w.planner_enable(env, dict(p, max_iterations=50))  # a new map while requests wait
    # one that has ended and waits to be collected is cancelled too: the first of the others to end
    need = {i: gp.slices_needed(expected[0][i], p, budget) for i in (0, 2, 3)}
    gone = min(need, key=lambda i: (need[i], i))
    for _ in range(need[gone] - 1):  # (one advance has been made)
        w.plan_advance(budget)
    w.synchronize()
    w.plan_cancel(tickets[gone])
    assert w.plan_pending() == 2
    got = _drain(w, p, budget)
    assert sorted(d["ticket"] for d in got) == [tickets[i] for i in (0, 2, 3) if i != gone]
    for d in got:
        i = tickets.index(d["ticket"])
        _same_plan(d, expected[0][i])
        assert d["slices"] == need[i]
    with pytest.raises(hostlib.MgxError, match="not pending"):
        w.plan_cancel(got[0]["ticket"])  # collected
    # the synchronous call and the tree read-back work beside pending requests
    more = w.plan_submit(DENSE[:2])
    w.plan_advance(budget)
    res = w.plan_paths(DENSE[2:3])
    _same(res[0], w.plan_tree(0), expected[0][2])
    assert w.plan_pending() == 2
    # off: they are dropped with everything else
    w.planner_enable(None)
    assert w.plan_pending() == 0
    with pytest.raises(hostlib.MgxError, match="planner is off"):
        w.plan_collect(wait=True)
    w.planner_enable(env, p)
    assert w.plan_collect(wait=True) == []
    again = w.plan_submit(DENSE[:1])
    assert again[0] == more[-1] + 1  # (never used twice)
    (d,) = _drain(w, p, budget)
    _same_plan(d, expected[0][0])


def test_the_layout_does_not_move(solo, expected):
    env, p = solo
    sc = S.grid_scenario(4, 10, interrobot=True, comm_radius=8.0)
    w = World(sc["params"])
    S.populate(w, sc)
    w.iterate(sc["steps"])
    w.planner_enable(env, p)
    stats = w.layout_stats()
    w.plan_submit(DENSE[:2])
    assert w.layout_stats() == stats
    w.plan_advance(64)
    w.iterate(sc["steps"])
    assert w.layout_stats() == stats
    got = _drain(w, p, 64)
    assert w.layout_stats() == stats
    w.iterate(sc["steps"])
    assert w.layout_stats() == stats
    for d, ref in zip(sorted(got, key=lambda d: d["ticket"]), expected[0]):
        _same_plan(d, ref)


# ---- 6. riding the ticks -------------------------------------------------------------------------------------------------------
def _driver():
    """12 robots x 8 variables on a circle, their missions on the device (as tests/test_gpu_global_paths.py makes its driver)"""
    n, K = 12, 8
    had = S.HORIZON_FOR_K.get(K)
    S.HORIZON_FOR_K[K] = next(h for h in range(1, 200) if len(hostlib.variable_timesteps(h, 3)) == K)
    try:
        sc = S.circle_scenario(n, K, circle_radius=10.0, n_internal=10, n_external=10)
    finally:
        if had is None:
            del S.HORIZON_FOR_K[K]
    sc["ir"] = []
    sc["params"] = dict(sc["params"], enable_mask=sc["params"]["enable_mask"] | S.EN_TRK)
    for rb in sc["robots"]:
        rb["path"] = np.array([rb["pos"], rb["goal"]], dtype=F)
    w = World(sc["params"])
    S.populate(w, sc)
    return w, DeviceDriver(w, n, K, **mission_kwargs(sc, ()))


def test_a_tick_carries_one_slice_and_computes_what_it_computes_without(solo, expected):
    env, p = solo
    budget = 32
    ref = expected[0][0]
    need = gp.slices_needed(ref, p, budget)
    assert need >= 3
    (w, de), (plain, dp) = _driver(), _driver()
    w.planner_enable(env, p)
    w.planner_set_tick_budget(budget)
    (ticket,) = w.plan_submit(DENSE[:1])
    for t in range(1, need + 3):
        assert de.tick() == dp.tick()
        got = w.plan_collect(wait=True)
        if t < need:
            assert got == [] and w.plan_pending() == 1, t
        elif t == need:  # t ticks: t slices behind it
            assert len(got) == 1 and got[0]["ticket"] == ticket and got[0]["slices"] == need == t
            _same_plan(got[0], ref)
        else:
            assert got == [] and w.plan_pending() == 0
        for a, b in zip(w.read_beliefs(), plain.read_beliefs()):
            assert np.array_equal(a, b, equal_nan=True), t
        sa, sb = de.state(), dp.state()
        assert all(np.array_equal(x, y) for x, y in zip(sa, sb)), t


def test_without_a_budget_the_ticks_advance_nothing(solo, expected):
    env, p = solo
    q = dict(p, max_iterations=FAIL_ITERATIONS)
    w, de = _driver()
    w.planner_enable(env, q)
    w.plan_submit([NOWHERE])
    for _ in range(3):
        de.tick()
    assert w.plan_collect(wait=True) == [] and w.plan_pending() == 1
    w.planner_set_tick_budget(32)
    de.tick()
    w.planner_set_tick_budget(0)
    for _ in range(2):
        de.tick()
    assert w.plan_collect(wait=True) == []
    for k in range(FAIL_ITERATIONS // 32 + 1 - 1):  # the one tick with a budget was its first slice
        assert w.plan_collect(wait=True) == []
        w.plan_advance(32)
    (d,) = w.plan_collect(wait=True)
    assert d["slices"] == FAIL_ITERATIONS // 32 + 1 == 4
    _same_plan(d, expected[1])


# ---- 7. Solo GP with the plan riding the ticks ----------------------------------------------------------------------------------
OVERRIDES = {"sample_half_extent": 125.0, "max_iterations": 20000}


class _Run:
    def __init__(self, mode):
        sc = config.load_scenario(SOLO_GP)
        self.sc = sc
        self.s = s = sim.Simulation(sc, World(config.world_params(sc["config"])), global_planner=mode, planner_overrides=OVERRIDES, plan_budget=64)
        s.tick()  # the tick the robot spawns in
        assert len(s.robots) == 1 and s.robots[0]["idle"]
        self.request = (tuple(float(v) for v in s.robots[0]["waypoints"][0][:2]), tuple(float(v) for v in s.robots[0]["waypoints"][1][:2]),
                        s.robots[0]["rng"].state)
        self.spawned_at = s.translation[0].copy()
        self.idle_positions = []
        while s.robots[0]["idle"] and s.tick_no < 400:
            s.tick()
            if s.robots[0]["idle"]:
                self.idle_positions.append(s.translation[0].copy())
        self.active_at = s.tick_no - 1  # the tick whose start applied the path
        s.run()
        self.export = s.export()


@pytest.fixture(scope="module")
def runs():
    return {mode: _Run(mode) for mode in (True, "sliced")}


def test_solo_gp_sliced_is_the_synchronous_run_shifted(runs):
    """The synchronous run plans inside the tick the robot spawns in (tick 0) and applies the path when tick 1 starts.  Sliced,
    the request is submitted in tick 0 and every tick from tick 0 on ends with one slice, so a plan of s slices is complete behind
    tick s - 1 and is applied when tick s starts: s = 1 is the synchronous run, and each further slice is one more tick of waiting."""
    syn, sl = runs[True], runs["sliced"]
    assert syn.request == sl.request
    p = gp.params_from_config(syn.sc["config"], **OVERRIDES)
    want = gp.plan_paths(syn.sc["environment"], [syn.request], p)[0]
    need = gp.slices_needed(want, p, 64)
    assert want["status"] == gp.PLAN_OK and need >= 2
    a, b = syn.export["global_planner"], sl.export["global_planner"]
    assert a == b and len(a["requests"]) == 1 and a["failed"] == []
    assert a["requests"][0] == {"robot": 0, "status": 0, "n_nodes": want["n_nodes"], "iterations": want["iterations"], "n_points": len(want["path"])}
    assert np.array(syn.s.robots[0]["waypoints"], F).tobytes() == np.array(sl.s.robots[0]["waypoints"], F).tobytes()
    assert np.array(sl.s.robots[0]["waypoints"], F)[:, :2].tobytes() == want["path"].tobytes()
    assert syn.active_at == 1 and sl.active_at == need
    # while it waits it neither iterates nor moves
    assert len(sl.idle_positions) == need - 1 and all(np.array_equal(x, sl.spawned_at) for x in sl.idle_positions)
    ra, rb = syn.export["robots"]["0"], sl.export["robots"]["0"]
    assert len(ra["positions"]) > 100 and ra["positions"] == rb["positions"]
    shift = (need - 1) * syn.export["delta_t"]
    assert len(ra["velocities"]) == len(rb["velocities"]) > 100
    for va, vb in zip(ra["velocities"], rb["velocities"]):  # the same samples, stamped that many ticks later
        assert va["velocity"] == vb["velocity"] and va["measured_over"] == vb["measured_over"]
        assert abs(vb["timestamp"] - va["timestamp"] - shift) < 1e-6
    assert sl.s.finished() and syn.s.finished()
    assert abs((rb["mission"]["finished_at"] - ra["mission"]["finished_at"]) - shift) < 1e-6
