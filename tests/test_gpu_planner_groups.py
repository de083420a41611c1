"""A planner parameter set per group (mgx_planner_set_group_params, mgx_planner_group_params, mgx_plan_paths_groups,
mgx_plan_submit_groups, mgx_plan_done.group): one launch runs requests of many groups, each under its own group's `rrt.*`, and
every plan and every tree is the host restatement's under that group's parameters, bit for bit — in both libraries, wherever the
slices fall, through the synchronous call and through submit / advance / collect.  Every set here changes ONE field, and the
restatement shows that each changes every DENSE result: a kernel that ignored a field would fail an equality below."""

import numpy as np
import pytest

from magics_amd import World, config, hostlib, scenarios as S
from magics_amd import global_planner as gp
from test_gpu_planner import DENSE, SOLO_GP, _same

pytestmark = pytest.mark.gpu

# group -> what its set changes (the groups are indices of sets, not dense: rows of the table are handed out as sets come)
SETS = {1: dict(step_size=2.5, smoothing_step=2.5), 2: dict(neighbourhood_radius=16.0), 3: dict(collision_radius=1.5),
        7: dict(smoothing_enabled=False), 40: dict(sample_half_extent=250.0), hostlib.GROUPS_MAX - 1: dict(max_iterations=300)}
SHORT = hostlib.GROUPS_MAX - 1   # the group whose requests run out of iterations
PLAIN = 5                        # a group that never has a set
GROUPS = [0] + sorted(SETS)


@pytest.fixture(scope="module")
def solo():
    sc = config.load_scenario(SOLO_GP)
    p = gp.params_from_config(sc["config"], max_iterations=20000, smoothing_max_iterations=60, sample_half_extent=125.0, max_nodes=2048)
    return sc["environment"], p


def _params(p, group):
    return dict(p, **SETS.get(group, {}))


def _key(r):
    return (r["status"], r["n_nodes"], r["iterations"], r["smoothing_iterations"], r["cost"], r["wyrand_state"], r["path"].tobytes())


@pytest.fixture(scope="module")
def expected(solo):
    """the restatement's results of the DENSE requests under every group's parameters, computed once: group -> [result]"""
    env, p = solo
    out = {g: gp.plan_paths(env, DENSE, _params(p, g)) for g in GROUPS}
    assert all(r["status"] == gp.PLAN_OK for r in out[0])
    for g in SETS:   # the precondition: under every set every request gives another result than under the world's parameters
        for r, r0 in zip(out[g], out[0]):
            assert _key(r) != _key(r0), f"group {g}: its set does not show in a result"
        if g == SHORT:
            assert all(r["status"] == gp.PLAN_MAX_ITERATIONS and r["iterations"] == 300 for r in out[g])
        else:
            assert all(r["status"] == gp.PLAN_OK and 1 < r["n_nodes"] < p["max_nodes"] for r in out[g])
    assert max(r["n_nodes"] for rs in out.values() for r in rs) > 256   # (the strided loops run more than once)
    return out


def _world(env, p, fma=None, sets=True):
    w = World(S.JUNCTION_PARAMS, fma=fma)
    w.planner_enable(env, p)
    if sets:
        for g in SETS:
            w.planner_set_group_params(g, _params(p, g))
    return w


def _interleaved():
    """every DENSE request under every group, the groups of one request side by side -> (requests, groups, (group, request index))"""
    which = [(g, i) for i in range(len(DENSE)) for g in GROUPS]
    return [DENSE[i] for g, i in which], [g for g, i in which], which


def _same_plan(d, ref):
    _same(d, None, ref)
    assert d["smoothing_iterations"] == ref["smoothing_iterations"]


# ---- 1. one synchronous call, every group in it ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
@pytest.mark.parametrize("per_launch", [1, 7, 1024])
def test_every_group_runs_under_its_own_set(solo, expected, per_launch, fma):
    env, p = solo
    w = _world(env, dict(p, iterations_per_launch=per_launch), fma)
    requests, groups, which = _interleaved()
    res = w.plan_paths(requests, groups)
    assert len(res) == len(which)
    for k, (g, i) in enumerate(which):
        _same(res[k], w.plan_tree(k), expected[g][i])
        assert res[k]["smoothing_iterations"] == expected[g][i]["smoothing_iterations"]


# ---- 2. the same riding the stream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [7, 64, 100])   # (100 divides the 300 iterations of the short group; 7 and 64 do not)
def test_submitted_groups_come_back_with_their_group_and_slice(solo, expected, budget):
    env, p = solo
    w = _world(env, p)
    requests, groups, which = _interleaved()
    tickets = w.plan_submit(requests, groups=groups)
    assert w.plan_pending() == len(tickets) == len(which)
    got = []
    for _ in range((p["max_iterations"] + p["smoothing_max_iterations"]) // budget + 2):
        if not w.plan_pending():
            break
        w.plan_advance(budget)
        got += w.plan_collect(wait=True, capacity=len(tickets))
    assert w.plan_pending() == 0 and len(got) == len(tickets)
    order = [(d["slices"], d["ticket"]) for d in got]
    assert order == sorted(order)
    by_ticket = {d["ticket"]: d for d in got}
    for t, (g, i) in zip(tickets, which):
        d, ref = by_ticket[t], expected[g][i]
        _same_plan(d, ref)
        assert d["group"] == g
        assert d["slices"] == gp.slices_needed(ref, _params(p, g), budget)   # (the group's own max_iterations)
    assert {d["slices"] for d in got if d["group"] == SHORT} == {300 // budget + 1}


# ---- 3. a world with sets computes the plain call's plans for requests that name none -----------------------------------------------
def test_requests_without_a_set_are_the_plain_calls(solo, expected):
    env, p = solo
    plain = _world(env, p, sets=False)
    ref = plain.plan_paths(DENSE)
    trees = [plain.plan_tree(i) for i in range(len(DENSE))]
    w = _world(env, p)
    for groups in (None, [PLAIN] * len(DENSE), [0] * len(DENSE)):
        res = w.plan_paths(DENSE, groups)
        for i, (a, b) in enumerate(zip(res, ref)):
            assert _key(a) == _key(b)
            _same(a, w.plan_tree(i), dict(expected[0][i]))
            for x, y in zip(w.plan_tree(i), trees[i]):
                assert x.tobytes() == y.tobytes()
    # ... and beside requests that do: the same launch, both kinds
    res = w.plan_paths(DENSE + DENSE, [PLAIN] * len(DENSE) + [3] * len(DENSE))
    for i in range(len(DENSE)):
        assert _key(res[i]) == _key(ref[i])
        _same_plan(res[len(DENSE) + i], expected[3][i])
    # the plain submit is group 0
    (t,) = plain.plan_submit(DENSE[:1])
    plain.plan_advance(1 << 20)
    (d,) = plain.plan_collect(wait=True)
    assert (d["ticket"], d["group"]) == (t, 0)
    _same_plan(d, expected[0][0])


# ---- 4. what a group runs under ------------------------------------------------------------------------------------------------------
def _held(q):
    """a parameter dict as the engine holds it: f32 fields, flags as bool"""
    return {k: (bool(v) if k == "smoothing_enabled" else float(np.float32(v)) if isinstance(v, float) else int(v)) for k, v in q.items()}


def test_group_params_round_trip_and_enable_forgets_them(solo):
    env, p = solo
    w = _world(env, p)
    world = dict(_held(p), iterations_per_launch=1024)   # (0 became the default)
    assert w.planner_group_params(0) == world and w.planner_group_params(PLAIN) == world
    for g in SETS:
        assert w.planner_group_params(g) == dict(world, **_held(SETS[g]))
    # a set may name the launch's two fields as the world has them, and 0 for the half extent is the default's 2000
    w.planner_set_group_params(2, dict(_params(p, 2), max_nodes=2048, iterations_per_launch=1024, sample_half_extent=0.0))
    assert w.planner_group_params(2) == dict(world, neighbourhood_radius=16.0, sample_half_extent=2000.0)
    # taken back: the world's again; set again: the same row is written over
    w.planner_set_group_params(3, None)
    assert w.planner_group_params(3) == world
    w.planner_set_group_params(3, _params(p, 1))
    assert w.planner_group_params(3) == dict(world, **_held(SETS[1]))
    w.planner_set_group_params(PLAIN, None)   # (a group that has none: nothing to take back)
    # more sets than the table's first allocation holds
    for g in range(100, 140):
        w.planner_set_group_params(g, dict(p, max_iterations=1000 + g))
    assert [w.planner_group_params(g)["max_iterations"] for g in range(100, 140)] == [1000 + g for g in range(100, 140)]
    assert w.planner_group_params(1) == dict(world, **_held(SETS[1]))
    # mgx_planner_enable, a new map: every set is forgotten
    w.planner_enable(env, p)
    for g in list(SETS) + [100, 139]:
        assert w.planner_group_params(g) == world


def test_sets_survive_a_grown_table_in_the_plans(solo, expected):
    """the rows written before the table grew are the rows the kernel reads afterwards"""
    env, p = solo
    w = _world(env, p)
    for g in range(100, 140):
        w.planner_set_group_params(g, _params(p, 3) if g == 139 else dict(p, max_iterations=1000 + g))
    res = w.plan_paths([DENSE[0], DENSE[0], DENSE[1]], [1, 139, SHORT])
    _same_plan(res[0], expected[1][0])
    _same_plan(res[1], expected[3][0])
    _same_plan(res[2], expected[SHORT][1])


# ---- 5. what is refused, and that it changed nothing -----------------------------------------------------------------------------------
ERR_INVALID, ERR_STATE = -1, -4   # MGX_ERR_INVALID, MGX_ERR_STATE


def _refused(call, code):
    with pytest.raises(hostlib.MgxError, match=f"mgx error {code}:"):
        call()


def test_refusals_change_nothing(solo, expected):
    env, p = solo
    w = World(S.JUNCTION_PARAMS)
    # planner off comes before everything else
    _refused(lambda: w.planner_set_group_params(hostlib.GROUPS_MAX, dict(p, step_size=-1.0)), ERR_STATE)
    _refused(lambda: w.planner_group_params(0), ERR_STATE)
    w.planner_enable(env, p)
    w.planner_set_group_params(3, _params(p, 3))
    before = {g: w.planner_group_params(g) for g in (0, 3, PLAIN)}

    def unchanged():
        assert {g: w.planner_group_params(g) for g in (0, 3, PLAIN)} == before
    # the group, then the values, then the launch's two fields
    _refused(lambda: w.planner_set_group_params(hostlib.GROUPS_MAX, dict(p, step_size=-1.0)), ERR_INVALID)
    _refused(lambda: w.planner_set_group_params(hostlib.GROUPS_MAX, None), ERR_INVALID)
    _refused(lambda: w.planner_group_params(hostlib.GROUPS_MAX), ERR_INVALID)
    for bad in (dict(step_size=0.0), dict(step_size=float("nan")), dict(neighbourhood_radius=-1.0), dict(neighbourhood_radius=float("inf")),
                dict(smoothing_step=0.0), dict(collision_radius=-0.5), dict(collision_radius=float("nan")), dict(sample_half_extent=-1.0),
                dict(sample_half_extent=float("inf")), dict(max_nodes=(1 << 16) + 1), dict(max_nodes=1024), dict(max_nodes=4096),
                dict(iterations_per_launch=7), dict(step_size=-1.0, max_nodes=1024)):
        for g in (3, PLAIN):
            _refused(lambda: w.planner_set_group_params(g, dict(p, **bad)), ERR_INVALID)
        unchanged()
    w.planner_set_group_params(PLAIN, dict(p, smoothing_enabled=False, smoothing_step=0.0))   # (no smoothing: its step is not looked at)
    w.planner_set_group_params(PLAIN, None)
    unchanged()
    # a group beyond the last: nothing is queued, nothing is planned
    _refused(lambda: w.plan_submit(DENSE[:2], groups=[3, hostlib.GROUPS_MAX]), ERR_INVALID)
    assert w.plan_pending() == 0
    rc, *_ = w.plan_paths_raw(np.zeros(1, hostlib.plan_request_dtype()), 64, groups=[hostlib.GROUPS_MAX])
    assert rc == ERR_INVALID
    with pytest.raises(ValueError):
        w.plan_submit(DENSE[:2], groups=[3])
    # a set does not change under a request that pends — neither set nor taken back — and does once it is collected
    (t,) = w.plan_submit(DENSE[:1], groups=[3])
    for g in (3, PLAIN):
        _refused(lambda: w.planner_set_group_params(g, _params(p, 1)), ERR_STATE)
        _refused(lambda: w.planner_set_group_params(g, None), ERR_STATE)
    _refused(lambda: w.planner_set_group_params(3, dict(p, step_size=-1.0)), ERR_INVALID)   # (the values come before the pool)
    unchanged()
    w.plan_advance(1 << 20)
    (d,) = w.plan_collect(wait=True)
    assert (d["ticket"], d["group"]) == (t, 3)
    _same_plan(d, expected[3][0])
    w.planner_set_group_params(3, _params(p, 1))
    (d,) = w.plan_paths(DENSE[:1], [3])
    _same_plan(d, expected[1][0])
    # a request that was cancelled pends no longer either
    (t,) = w.plan_submit(DENSE[:1], groups=[3])
    w.plan_cancel(t)
    w.planner_set_group_params(3, None)
    assert w.planner_group_params(3) == before[0]
