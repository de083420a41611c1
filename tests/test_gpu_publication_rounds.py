"""The publication of the exchange records at the end of a resident launch's segment (mgx_sweep.h: for a constant horizon the
ceil(15 K / 64) passes are written out, every LDS read of every pass in front of one wait; the run-time-K kernels keep the loop),
each on a world small enough for a few hundred milliseconds: against the CPU oracle bit for bit after 1, 2 and 12 iterations of
the 10 / 10 schedule — resident with lingering, resident without, and launch by launch.  Every wait inside a launch is bounded
(MGX_RESIDENT_TIMEOUT_MS, 2000 by default): a record that never arrives ends as a reported error, not as a hang.

  K9                twelve robots on a grid, the run-time-K kernel: the loop form
  K10               150 chunks: three passes, the last one partly masked (22 lanes); the delivery counts sit in lanes 12 .. 21 of it
  K16               240 chunks: four passes, the delivery counts in lanes 32 .. 47 of the last (the headline's kernel)
  K17               255 chunks: the last pass holds one lane fewer than a wave
  K21               315 chunks: five passes
  lonely_one_sided  robot 5 has no neighbour at all, robot 1 hears robot 0 but not the other way round: records nobody reads,
                    workgroups nobody waits for
  undelivered       every robot's first and last variable get a new prior (a delivery each) before anything has iterated, then
                    two external-only iterations run as one schedule: the records carry delivery counts of 1, 0, ..., 0, 1, and
                    the first factor sweeps meet variables that have not answered
  two_ranks         (its own test) 2 x 24 robots at K = 16 as two in-process ranks with resident launches: boundary robots publish
                    into the other rank's ghost area as well, the sequence word mixed with the payload
"""
import numpy as np
import pytest

import oracle
from magics_amd import World, hostlib, scenarios as S, sharded
from test_gpu_gather_paths import FORMS, POSTED, RESIDENT, SEGMENTS, SHARDED, _grid, _same, _stages  # the same worlds, forms and comparison

pytestmark = pytest.mark.gpu

CASES = ("K9", "K10", "K16", "K17", "K21", "lonely_one_sided", "undelivered")


def _scenario(case):
    """(scenario, whether the case's prelude runs: new priors, then two external-only iterations)"""
    if case in ("K9", "K10", "K16", "K17", "K21"):
        return _grid(12, int(case[1:]), interrobot=True, pitch=2.5, comm_radius=4.5), False
    if case == "undelivered":
        return _grid(12, 16, interrobot=True, pitch=2.5, comm_radius=4.5), True
    if case == "lonely_one_sided":
        # six robots in a row, 2 m apart, robot 5 far away; everyone of 0 .. 4 hears everyone, but robot 0 owns no factor towards robot 1
        sc = _grid(6, 16, interrobot=True, comm_radius=1000.0, pitch=2.0, grid_side=6)
        pos = np.array(sc["positions"], dtype=np.float64)
        shift = np.array([60.0, 40.0]) - pos[5]
        sc["robots"][5]["mean0"] = np.array(sc["robots"][5]["mean0"], dtype=np.float64)
        sc["robots"][5]["mean0"][:, :2] += shift
        pos[5] += shift
        sc["positions"] = pos
        pairs = [(a, b) for a, b in S.neighbour_pairs(pos, 15.0)]
        assert not any(5 in p for p in pairs)
        pairs.remove((0, 1))
        sc["ir"] = S.number_ir_pairs(pairs, 16)
        return sc, False
    raise ValueError(case)


def _run(w, sc, prelude):
    """the case's script; yields the number of iterations of the 10 / 10 schedule so far after every schedule"""
    S.populate(w, sc)
    if prelude:
        w.update_priors(**S.tick_inputs(sc))
        w.iterate([hostlib.STEP_EXTERNAL, hostlib.STEP_EXTERNAL])
    for n, steps in _stages(sc):
        w.iterate(steps)
        yield n


_REFERENCE = {}  # case -> (scenario, prelude, the oracle's beliefs after 1, 2 and 12 iterations): computed once, never changed


def _reference(case):
    if case not in _REFERENCE:
        sc, prelude = _scenario(case)
        ref = oracle.OracleWorld(sc["params"])
        beliefs = {n: [a.copy() for a in ref.read_beliefs()] for n in _run(ref, sc, prelude)}
        _REFERENCE[case] = (sc, prelude, beliefs)
    return _REFERENCE[case]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_publication_bit_identical(case, form):
    sc, prelude, beliefs = _reference(case)
    eng = World(sc["params"])
    if form == "launch_per_segment":
        eng.set_resident_launches(False)
    else:
        eng.set_linger(50000 if form == "resident_lingering" else 0)
    declined0 = eng.resident_stats()[1]
    for n in _run(eng, sc, prelude):
        _same(eng.read_beliefs(), beliefs[n], f"{case}, {form}, {n} iterations")
    variant, ir_mode, ran, capacity = eng.last_sweep()
    print(f"[{case}, {form}] (variant, ir_mode, form, capacity) = {(variant, ir_mode, ran, capacity)}")
    if form == "launch_per_segment":
        assert ran == SEGMENTS
    elif eng.resident_stats()[1] == declined0:  # (a launch the residency census declined ran launch by launch: compared all the same)
        assert ran in (RESIDENT, POSTED), (case, form, eng.last_sweep())


def test_two_ranks_remote_publication_bit_identical():
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
