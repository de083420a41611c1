"""The forms of the resident sweep kernel (mgx_sweep.h, FEAT; include/mgx.h, mgx_last_sweep_features): a resident launch runs the
smallest instantiation that covers it — lean (0) where the world's tracking factors are off and no prior updates ride, with
the prior-update path (2) once an mgx_tick has come, full (3) where tracking factors are on or mgx_set_specialize(w, 0) says
so.  Whatever form runs, the beliefs are the CPU oracle's bit for bit, and every test asserts the form that ran.  Worlds of at
most 48 robots.  (A resident launch the residency census declined runs launch by launch, in the full form: compared all the
same, its form not asserted — as in test_gpu_gather_paths.py.)"""
import numpy as np
import pytest

import oracle
from magics_amd import World, hostlib, scenarios as S, sharded
from test_gpu_gather_paths import POSTED, RESIDENT, SEGMENTS, SHARDED, _grid, _same, _stages

pytestmark = pytest.mark.gpu

LEAN, UPD, FULL = 0, 2, 3  # MGX_SWEEP_F_TRACKING = 1, MGX_SWEEP_F_UPDATES = 2
HORIZONS = (10, 11, 12, 13, 16, 17, 20, 21, 32, 35)  # every constant-K instantiation
MODES = ("resident_lingering", "resident", "unspecialised")


def _world(sc, mode):
    w = World(sc["params"])
    w.set_linger(0 if mode == "resident" else 50000)
    if mode == "unspecialised":
        w.set_specialize(False)
    return w


def _ran(w, want_features, what, forms=(RESIDENT, POSTED), declined0=0):
    """the form of the last sweep: asserted unless the census sent a launch back (then the segments' full form ran)"""
    variant, _, form, _ = w.last_sweep()
    feat = w.last_sweep_features()
    print(f"[{what}] variant {variant}, form {form}, features {feat}")
    if w.resident_stats()[1] != declined0:
        return
    assert form in forms and feat == want_features, (what, form, feat, want_features)


# ---- horizons -------------------------------------------------------------------------------------------------------------
_HORIZON_REF = {}  # K -> (scenario, the oracle's beliefs after 1, 2 and 12 iterations): computed once, never changed


def _horizon_reference(K):
    if K not in _HORIZON_REF:
        sc = _grid(12, K, interrobot=True, pitch=2.5, comm_radius=4.5)
        assert not sc["params"]["enable_mask"] & S.EN_TRK
        ref = oracle.OracleWorld(sc["params"])
        S.populate(ref, sc)
        beliefs = {}
        for n, steps in _stages(sc):
            ref.iterate(steps)
            beliefs[n] = [a.copy() for a in ref.read_beliefs()]
        _HORIZON_REF[K] = (sc, beliefs)
    return _HORIZON_REF[K]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", HORIZONS)
def test_horizons(K, mode):
    sc, beliefs = _horizon_reference(K)
    eng = _world(sc, mode)
    S.populate(eng, sc)
    d0 = eng.resident_stats()[1]
    for n, steps in _stages(sc):
        eng.iterate(steps)
        if len(steps) > 1:
            _ran(eng, FULL if mode == "unspecialised" else LEAN, f"K{K}, {mode}, {n} iterations", declined0=d0)
            assert eng.last_sweep()[0] == K
        _same(eng.read_beliefs(), beliefs[n], f"K{K}, {mode}, {n} iterations")


# ---- mgx_tick and tracking worlds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (12, 16))
def test_tick_runs_the_update_form_and_tracking_the_full_one(K):
    sc = _grid(12, K, interrobot=True, pitch=2.5, comm_radius=4.5)
    eng, ref = _world(sc, "resident_lingering"), oracle.OracleWorld(sc["params"])
    tick = S.tick_inputs(sc)
    d0 = eng.resident_stats()[1]
    for w in (eng, ref):
        S.populate(w, sc)
        for _ in range(3):
            w.tick(steps=sc["steps"], **tick)
    _ran(eng, UPD, f"K{K}, three ticks", declined0=d0)
    _same(eng.read_beliefs(), ref.read_beliefs(), f"K{K}, three ticks in the update form")

    sct = _grid(12, K, interrobot=True, pitch=3.0, comm_radius=7.0, tracking=True)
    eng, ref = _world(sct, "resident_lingering"), oracle.OracleWorld(sct["params"])
    d0 = eng.resident_stats()[1]
    for w in (eng, ref):
        S.populate(w, sct)
        w.iterate(sct["steps"])
        w.iterate(sct["steps"])  # (the tracking factors' gate opens at the tenth iteration)
    _ran(eng, FULL, f"K{K}, tracking", declined0=d0)
    _same(eng.read_beliefs(), ref.read_beliefs(), f"K{K}, tracking factors in the full form")


# ---- transitions ----------------------------------------------------------------------------------------------------------
def _pair(sc):
    eng, ref = _world(sc, "resident_lingering"), oracle.OracleWorld(sc["params"])
    for w in (eng, ref):
        S.populate(w, sc)
    return eng, ref


def test_a_tick_ends_the_lean_launch_and_the_world_stays_on_the_update_form():
    sc = _grid(16, 16, interrobot=True, pitch=2.5, comm_radius=4.5)
    eng, ref = _pair(sc)
    eng.set_post_merge(0)  # (every schedule a post of its own: what is posted follows from the calls alone)
    tick = S.tick_inputs(sc)
    d0 = eng.resident_stats()[1]
    eng.iterate(sc["steps"])
    _ran(eng, LEAN, "iterate", forms=(RESIDENT,), declined0=d0)
    eng.iterate(sc["steps"])
    _ran(eng, LEAN, "iterate, iterate", forms=(POSTED,), declined0=d0)
    l0 = eng.linger_stats()
    eng.tick(steps=sc["steps"], **tick)  # not posted into the lean launch: that one ends, a launch of the update form starts
    _ran(eng, UPD, "iterate, iterate, tick", forms=(RESIDENT,), declined0=d0)
    eng.iterate(sc["steps"])
    _ran(eng, UPD, "iterate, iterate, tick, iterate", forms=(POSTED,), declined0=d0)
    l1 = eng.linger_stats()
    if eng.resident_stats()[1] == d0:
        assert l1[0] == l0[0] + 1 == 2, (l0, l1)            # the launch ended and a new one started
        assert l1[1] + l1[2] == l0[1] + l0[2] + 1, (l0, l1)  # the tick was no post; the iterate behind it was
    for st in (sc["steps"], sc["steps"]):
        ref.iterate(st)
    ref.tick(steps=sc["steps"], **tick)
    ref.iterate(sc["steps"])
    _same(eng.read_beliefs(), ref.read_beliefs(), "iterate, iterate, tick, iterate")
    # later launches keep the form: no launch ends for the next tick
    eng.iterate(sc["steps"]); ref.iterate(sc["steps"])
    _ran(eng, UPD, "a launch after the read", forms=(RESIDENT,), declined0=d0)
    l2 = eng.linger_stats()
    eng.tick(steps=sc["steps"], **tick); ref.tick(steps=sc["steps"], **tick)
    _ran(eng, UPD, "a tick posted into it", forms=(POSTED,), declined0=d0)
    if eng.resident_stats()[1] == d0:
        assert eng.linger_stats()[0] == l2[0]
    _same(eng.read_beliefs(), ref.read_beliefs(), "iterate, tick on the update form")


def test_the_same_inside_a_batch():
    sc = _grid(16, 16, interrobot=True, pitch=2.5, comm_radius=4.5)
    eng, ref = _pair(sc)
    tick = S.tick_inputs(sc)
    d0 = eng.resident_stats()[1]
    short = sc["steps"][:4]
    eng.batch_begin()
    eng.iterate(short)
    eng.iterate(short)
    eng.tick(steps=sc["steps"], **tick)  # (submits what was recorded — one lean launch — and does not ride in it)
    _ran(eng, UPD, "batch: iterate, iterate, tick", forms=(RESIDENT,), declined0=d0)
    eng.iterate(short)
    eng.batch_end()
    _ran(eng, UPD, "batch: iterate, iterate, tick, iterate", declined0=d0)
    if eng.resident_stats()[1] == d0:
        assert eng.linger_stats()[0] == 2, eng.linger_stats()
    ref.iterate(short); ref.iterate(short)
    ref.tick(steps=sc["steps"], **tick)
    ref.iterate(short)
    _same(eng.read_beliefs(), ref.read_beliefs(), "batch: iterate, iterate, tick, iterate")


def test_tracking_switched_off_and_on_between_schedules():
    """... and the host starts no resident launch while a kind thaws: the schedule behind mgx_set_enabled runs launch by launch"""
    sc = _grid(8, 16, interrobot=True, pitch=3.0, comm_radius=7.0, tracking=True)
    eng, ref = _pair(sc)
    d0 = eng.resident_stats()[1]

    def both(f):
        f(eng); f(ref)

    both(lambda w: (w.iterate(sc["steps"]), w.iterate(sc["steps"])))
    _ran(eng, FULL, "tracking on", declined0=d0)
    _same(eng.read_beliefs(), ref.read_beliefs(), "tracking on")
    both(lambda w: w.set_enabled(15 & ~S.EN_TRK))
    both(lambda w: w.iterate(sc["steps"]))
    _ran(eng, LEAN, "tracking off", forms=(RESIDENT,), declined0=d0)
    _same(eng.read_beliefs(), ref.read_beliefs(), "tracking off")
    both(lambda w: w.set_enabled(15))
    assert eng.is_thawing()
    both(lambda w: w.iterate(sc["steps"]))
    assert eng.last_sweep()[2] == SEGMENTS and eng.last_sweep_features() == FULL  # the thaw: never inside a resident launch
    assert not eng.is_thawing()
    _same(eng.read_beliefs(), ref.read_beliefs(), "tracking back on: the thaw, launch by launch")
    both(lambda w: w.iterate(sc["steps"]))
    _ran(eng, FULL, "tracking on again", forms=(RESIDENT,), declined0=d0)
    _same(eng.read_beliefs(), ref.read_beliefs(), "tracking on again")


# ---- what stays a run-time value in the lean form -------------------------------------------------------------------------
RUNTIME_CASES = ("idle", "antenna_off", "lonely_one_sided", "undelivered")


def _runtime_scenario(case, K):
    if case == "lonely_one_sided":  # robot 5 has no neighbour at all, robot 1 hears robot 0 but not the other way round
        sc = _grid(6, K, interrobot=True, comm_radius=1000.0, pitch=2.0, grid_side=6)
        pos = np.array(sc["positions"], dtype=np.float64)
        shift = np.array([60.0, 40.0]) - pos[5]
        sc["robots"][5]["mean0"] = np.array(sc["robots"][5]["mean0"], dtype=np.float64)
        sc["robots"][5]["mean0"][:, :2] += shift
        pos[5] += shift
        sc["positions"] = pos
        pairs = [(a, b) for a, b in S.neighbour_pairs(pos, 15.0)]
        assert not any(5 in p for p in pairs)
        pairs.remove((0, 1))
        sc["ir"] = S.number_ir_pairs(pairs, K)
        return sc
    return _grid(12, K, interrobot=True, pitch=2.5, comm_radius=4.5)


def _runtime_script(w, sc, case):
    S.populate(w, sc)
    if case == "idle":
        w.set_idle(3, True)
    if case == "antenna_off":
        w.set_antenna(4, False)
    if case == "undelivered":  # new priors before anything has iterated, then an external-only schedule
        w.update_priors(**S.tick_inputs(sc))
        w.iterate([hostlib.STEP_EXTERNAL, hostlib.STEP_EXTERNAL])
        yield "external only"
    for n, steps in _stages(sc):
        w.iterate(steps)
        yield n


@pytest.mark.parametrize("K", (10, 17))
@pytest.mark.parametrize("case", RUNTIME_CASES)
def test_runtime_state_in_the_lean_form(case, K):
    sc = _runtime_scenario(case, K)
    ref = oracle.OracleWorld(sc["params"])
    want = {n: [a.copy() for a in ref.read_beliefs()] for n in _runtime_script(ref, sc, case)}
    eng = _world(sc, "resident_lingering")
    d0 = eng.resident_stats()[1]
    for n in _runtime_script(eng, sc, case):
        if n in ("external only", 12):
            _ran(eng, LEAN, f"{case}, K{K}, {n}", declined0=d0)
        _same(eng.read_beliefs(), want[n], f"{case}, K{K}, {n}")


# ---- sharded --------------------------------------------------------------------------------------------------------------
def test_two_ranks_run_the_sharded_lean_form():
    from test_gpu_sharded import _own_stream_factory
    sc = S.grid_scenario(48, 16, interrobot=True, pitch=2.5, comm_radius=4.5)
    make, _streams = _own_stream_factory()
    cluster = sharded.LocalCluster(sc, 2, make, direct=True, resident=True)
    assert cluster.resident and all(len(sw.plan.local) == 24 and sw.plan.ghosts for sw in cluster.ranks)
    single = World(sc["params"])
    ref = oracle.OracleWorld(sc["params"])
    for w in (single, ref):
        S.populate(w, sc)
    d0 = cluster.declined
    for n, steps in _stages(sc):
        cluster.iterate(steps)
        single.iterate(steps)
        ref.iterate(steps)
        for sw in cluster.ranks:
            sw.synchronize()  # raises if a wait inside a launch gave up
        got = cluster.read_beliefs()
        _same(got, ref.read_beliefs(), f"two ranks of 24 robots, {n} iterations")
        _same(got, single.read_beliefs(), f"two ranks against the single world, {n} iterations")
    ran = [(sw.world.last_sweep()[2], sw.world.last_sweep_features()) for sw in cluster.ranks]
    print(f"[two ranks] (form, features) {ran}, schedules declined by the ranks' census: {cluster.declined - d0}")
    if cluster.declined == d0:
        assert ran == [(SHARDED, LEAN), (SHARDED, LEAN)], ran
