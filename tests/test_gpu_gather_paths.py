"""The paths of the resident launch's gather (mgx_sweep.h, gather_records: the owners' exchange records loaded in place, polled,
only the missing chunks asked for again), each on a world
small enough for a few hundred milliseconds: against the CPU oracle bit for bit after 1, 2 and 12 iterations of the 10 / 10
schedule — resident with lingering, resident without, and launch by launch.  Every wait inside a launch is bounded
(MGX_RESIDENT_TIMEOUT_MS, 2000 by default): a gather that never sees its records ends as a reported error, not as a hang.

  K9, K10, K16, K17, K21   twelve robots on a grid.  10 and 16: the headline's code (one address register, the chunk's offset in
                    the instruction, four-lane belief finish); 17: the same addressing with the one-lane finish; 21: the chunk's
                    offset no longer fits the instruction; 9: the run-time-K kernel, the chunk stride a run-time value
  cluster           ten robots inside one comms radius at K = 16: 135 edge lanes for a workgroup of 128 threads, so the gather
                    runs a second round (j0 > 0)
  lonely_one_sided  robot 5 has no neighbour at all, robot 1 hears robot 0 but not the other way round: whole waves of lanes that
                    are not `mine`, workgroups nobody waits for
  late              the robots iterate a whole schedule on their own, THEN they are connected: the first external iterations
                    meet owners whose variables have not answered the new factors yet
  zero_precision    dynamics and obstacle factors switched off, a prior precision of 1e-9 on robot 0's first variable (the ABI
                    takes it): only the priors inform a variable, so every robot's variables 1 .. K - 2 and that first variable
                    have no entry above 1e-6 and go through the finish in every iteration next to variables that are informed
  two_ranks         (its own test) 2 x 24 robots at K = 16 as two in-process ranks with resident launches: ghost records arrive
                    from the other rank inside the launch, their sequence words mixed with the payload
"""
import numpy as np
import pytest

import oracle
from magics_amd import World, hostlib, scenarios as S, sharded

pytestmark = pytest.mark.gpu

SEGMENTS, RESIDENT, POSTED, SHARDED = 0, 1, 2, 3  # MGX_SWEEP_FORM_*
FORMS = ("resident_lingering", "resident", "launch_per_segment")


def _grid(n, K, **kw):
    if K in S.HORIZON_FOR_K:
        return S.grid_scenario(n, K, **kw)
    S.HORIZON_FOR_K[K] = next(h for h in range(1, 1000) if len(hostlib.variable_timesteps(h, 3)) == K)
    try:
        return S.grid_scenario(n, K, **kw)
    finally:
        del S.HORIZON_FOR_K[K]


def _six(K, **kw):
    """six robots in a row, 2 m apart, robot 5 far away; everyone of 0 .. 4 hears everyone"""
    sc = _grid(6, K, interrobot=True, comm_radius=1000.0, pitch=2.0, grid_side=6, **kw)
    pos = np.array(sc["positions"], dtype=np.float64)
    shift = np.array([60.0, 40.0]) - pos[5]
    sc["robots"][5]["mean0"] = np.array(sc["robots"][5]["mean0"], dtype=np.float64)
    sc["robots"][5]["mean0"][:, :2] += shift
    pos[5] += shift
    sc["positions"] = pos
    return sc, [(a, b) for a, b in S.neighbour_pairs(pos, 15.0)]


def _scenario(case):
    """(scenario, pairs connected only after a first schedule on their own)"""
    if case in ("K9", "K10", "K16", "K17", "K21"):
        return _grid(12, int(case[1:]), interrobot=True, pitch=2.5, comm_radius=4.5), []
    if case == "cluster":
        sc = _grid(10, 16, interrobot=True, pitch=1.2, comm_radius=1000.0, obstacles=False)
        assert max(sum(1 for a, _, _ in sc["ir"] if a == r) for r in range(10)) * 15 == 135  # more edge lanes than threads
        return sc, []
    if case == "lonely_one_sided":
        sc, pairs = _six(16)
        assert not any(5 in p for p in pairs)
        pairs.remove((0, 1))  # robot 0 owns no factor towards robot 1; robot 1 keeps its own towards robot 0
        sc["ir"] = S.number_ir_pairs(pairs, 16)
        return sc, []
    if case == "late":
        sc = _grid(12, 16, interrobot=True, pitch=2.5, comm_radius=4.5)
        late, sc["ir"] = sc["ir"], []
        return sc, late
    if case == "zero_precision":
        sc, pairs = _six(16, obstacles=False)
        sc["params"] = dict(sc["params"], enable_mask=S.EN_IR)
        sc["ir"] = S.number_ir_pairs(pairs, 16)
        sc["robots"][0]["prior_diag"] = np.array(sc["robots"][0]["prior_diag"], dtype=np.float64)
        sc["robots"][0]["prior_diag"][0] = 1e-9
        return sc, []
    raise ValueError(case)


CASES = ("K9", "K10", "K16", "K17", "K21", "cluster", "lonely_one_sided", "late", "zero_precision")


def _stages(sc):
    steps = list(sc["steps"])
    assert len(steps) == 10 and all(s == 3 for s in steps)  # ten iterations, each an external and an internal one
    return (1, steps[:1]), (2, steps[:1]), (12, steps)


def _run(w, sc, late):
    """the case's script; yields the number of iterations so far after every schedule"""
    S.populate(w, sc)
    if late:
        w.iterate(sc["steps"])
        for a, b, n0 in late:
            w.ir_connect(a, b, n0)
    for n, steps in _stages(sc):
        w.iterate(steps)
        yield n


_REFERENCE = {}  # case -> (scenario, late pairs, the oracle's beliefs after 1, 2 and 12 iterations): computed once, never changed


def _reference(case):
    if case not in _REFERENCE:
        sc, late = _scenario(case)
        ref = oracle.OracleWorld(sc["params"])
        beliefs = {n: [a.copy() for a in ref.read_beliefs()] for n in _run(ref, sc, late)}
        _REFERENCE[case] = (sc, late, beliefs)
    return _REFERENCE[case]


def _same(got, want, what):
    for name, a, b in zip(("eta", "lam", "mean"), got, want):
        if not np.array_equal(a, b, equal_nan=True):
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
            raise AssertionError(f"{what}: {name} differs from the oracle in {bad.sum()} elements, first at {tuple(np.argwhere(bad)[0])}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_gather_path_bit_identical(case, form):
    sc, late, beliefs = _reference(case)
    eng = World(sc["params"])
    if form == "launch_per_segment":
        eng.set_resident_launches(False)
    else:
        eng.set_linger(50000 if form == "resident_lingering" else 0)
    declined0 = eng.resident_stats()[1]
    for n in _run(eng, sc, late):
        _same(eng.read_beliefs(), beliefs[n], f"{case}, {form}, {n} iterations")
    if case == "zero_precision":
        lam = beliefs[12][1].reshape(len(beliefs[12][1]), -1)
        uninformed = ~(lam > 1e-6).any(axis=1)
        # (without dynamics factors nothing but the priors informs a variable: the inter-robot factors' Schur complements stay empty)
        assert uninformed[0] and uninformed[1:15].all() and not uninformed[15] and not uninformed[16], "the world was meant to mix both kinds"
    variant, ir_mode, ran, capacity = eng.last_sweep()
    print(f"[{case}, {form}] (variant, ir_mode, form, capacity) = {(variant, ir_mode, ran, capacity)}")
    if form == "launch_per_segment":
        assert ran == SEGMENTS
    elif eng.resident_stats()[1] == declined0:  # (a launch the residency census declined ran launch by launch: compared all the same)
        assert ran in (RESIDENT, POSTED), (case, form, eng.last_sweep())


def test_two_ranks_ghost_records_bit_identical():
    from test_gpu_sharded import _own_stream_factory
    sc = S.grid_scenario(48, 16, interrobot=True, pitch=2.5, comm_radius=4.5)
    make, _streams = _own_stream_factory()
    cluster = sharded.LocalCluster(sc, 2, make, direct=True, resident=True)
    assert cluster.resident and all(len(sw.plan.local) == 24 and sw.plan.ghosts for sw in cluster.ranks)
    ref = oracle.OracleWorld(sc["params"])
    S.populate(ref, sc)
    d0 = cluster.declined
    for n, steps in _stages(sc):
        cluster.iterate(steps)
        ref.iterate(steps)
        for sw in cluster.ranks:
            sw.synchronize()  # raises if a wait inside a launch gave up
        _same(cluster.read_beliefs(), ref.read_beliefs(), f"two ranks of 24 robots, {n} iterations")
    ran = [sw.world.last_sweep()[2] for sw in cluster.ranks]
    print(f"[two ranks] forms {ran}, schedules declined by the ranks' census: {cluster.declined - d0}")
    if cluster.declined == d0:
        assert ran == [SHARDED, SHARDED], ran
