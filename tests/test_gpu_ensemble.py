"""magics_amd.ensemble.Ensemble: M scenario runs as the groups of ONE world against the same M runs by a Simulation on a world of
its own each.  For every member json.dumps(member.export(), sort_keys=True) must EQUAL the solo run's — spawns, topology events,
comms draws, tracker samples, collisions, message counts, makespan; there is no tolerance.  The scenarios are the reference's
(tests/golden/scenarios.json); members differ in seed, failure rate and formation."""
import copy
import json
import os

import pytest

from magics_amd import World, config, sim
from magics_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenario(name, seed=None, failure_rate=None, tweak=None):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)[name]
    if seed is not None:
        sc["config"]["simulation"]["prng-seed"] = seed
    if failure_rate is not None:
        sc["config"]["robot"]["communication"]["failure-rate"] = failure_rate
    if tweak:
        tweak(sc)
    return sc


def _world(sc):
    return World(config.world_params(sc["config"]))


def _dump(export):
    return json.dumps(export, sort_keys=True)


def _against_solo(scs, max_ticks=None):
    """the ensemble and, member by member, the solo run to the same bound; returns (ensemble, solo simulations)"""
    ens = Ensemble([copy.deepcopy(sc) for sc in scs], _world(scs[0])).run(max_ticks=max_ticks)
    solos = []
    for m, sc in enumerate(scs):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc)).run(max_ticks=max_ticks)
        assert len(solo.robots) > 0
        assert ens.members[m].tick_no == solo.tick_no, m
        assert _dump(ens.members[m].export()) == _dump(solo.export()), m
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), m
        solos.append(solo)
    return ens, solos


def test_environment_obstacles_failure_rates_and_seeds():
    scs = [_scenario("Environment Obstacles Experiment", seed, rate) for rate in (0.0, 0.3) for seed in (805, 7)]
    ens, solos = _against_solo(scs, max_ticks=70)
    assert any(s.events for s in solos)                                   # robots met: connections were numbered per group
    assert _dump(solos[0].export()) != _dump(solos[2].export())           # (the failure rate shows: the members are different runs)


def test_junction_twoway_seeds():
    """random placement, repeating spawns, despawns"""
    scs = [_scenario("Junction Twoway", seed) for seed in (2, 7, 805)]
    ens, solos = _against_solo(scs, max_ticks=90)
    assert len({_dump(s.export()) for s in solos}) == 3
    assert all(len(s.robots) > 1 for s in solos)


def test_members_retire_at_different_ticks():
    """the Circle Experiment brought within reach of a short run (as tests/test_gpu_sim.py shortens it), members of 6 and of 12
    robots, run to the end: each member's makespan is its solo one, and the others go on when one has retired"""
    def short(n):
        def tweak(sc):
            f = sc["formation"]["formations"][0]
            f["robots"] = n
            f["initial-position"]["shape"]["radius"] = 12.0
            f["waypoints"][0]["shape"]["radius"] = 12.0
        return tweak
    scs = [_scenario("Circle Experiment", tweak=short(6)), _scenario("Circle Experiment", tweak=short(12))]
    ens, solos = _against_solo(scs)
    assert all(s.finished() for s in solos)
    assert [m.export()["makespan"] for m in ens.members] == [s.export()["makespan"] for s in solos]
    assert solos[0].tick_no != solos[1].tick_no and ens.tick_no == max(s.tick_no for s in solos)
    assert all(m.retired for m in ens.members)


def test_an_ensemble_of_one_is_the_solo_run():
    _against_solo([_scenario("Environment Obstacles Experiment", 805, 0.2)], max_ticks=40)


def test_one_launch_sequence_per_tick_serves_all_members():
    scs = [_scenario("Environment Obstacles Experiment", seed) for seed in (805, 7, 11, 13)]
    ens = Ensemble(scs, _world(scs[0]))
    solo = sim.Simulation(copy.deepcopy(scs[0]), _world(scs[0]))
    compared = 0
    for _ in range(25):           # (the formation spawns after one second: ten ticks without robots, then ticks of 4 x 5 and of 5)
        ens.tick()
        solo.tick()
        if solo.robots:
            assert all(m.sim.robots for m in ens.members)
            assert ens.world.last_launch_count() == solo.w.last_launch_count()
            compared += 1
    assert compared >= 10 and ens.world.num_robots()[0] == 4 * len(solo.robots)
