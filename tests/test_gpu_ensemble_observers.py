"""The device's per-robot observers under an Ensemble — environment collisions, goal areas, the run metrics, with and without the
sample log: every member against the same scenario run by a Simulation with the same options on a world of its own,
json.dumps(export) and json.dumps(metrics) EQUAL, no tolerance.  The observers do not look at the group; what is checked here is
the routing: one log, one set of first arrivals and one table of records for the world, every member reading its own robots'.

Environment Obstacles Experiment: its formation circle (radius 50) keeps the robots off the obstacles for the first seconds, so
the circle is drawn in to radius 14, where the first robot starts ON an obstacle (checked with the host's contact below)."""
import copy
import json
import os

import numpy as np
import pytest

from magics_amd import World, config, environment, hostlib, sim, spawner
from magics_amd.ensemble import Ensemble
from magics_amd.prng import WyRand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_AN_OBSTACLE = 14.0
JUNCTION_TICKS = 90


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


def _drawn_in(sc):
    f = sc["formation"]["formations"][0]
    f["initial-position"]["shape"]["radius"] = ON_AN_OBSTACLE
    f["waypoints"][0]["shape"]["radius"] = ON_AN_OBSTACLE


def _world(sc):
    return World(config.world_params(sc["config"]))


def _dump(export):
    return json.dumps(export, sort_keys=True)


def _against_solo(scs, max_ticks=None, **options):
    """the ensemble and, member by member, the solo run to the same bound with the same options; returns (ensemble, solo simulations)"""
    ens = Ensemble([copy.deepcopy(sc) for sc in scs], _world(scs[0]), **options).run(max_ticks=max_ticks)
    solos = []
    for m, sc in enumerate(scs):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **options).run(max_ticks=max_ticks)
        assert len(solo.robots) > 0
        assert ens.members[m].tick_no == solo.tick_no, m
        assert _dump(ens.members[m].export()) == _dump(solo.export()), m
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), m
        solos.append(solo)
    return ens, solos


def test_the_drawn_in_formation_starts_on_an_obstacle():
    for seed in (805, 7):
        sc = _scenario("Environment Obstacles Experiment", seed, tweak=_drawn_in)
        colliders, vertices = hostlib.env_colliders(sc["environment"])
        robots = spawner.spawn_formation(sc["formation"]["formations"][0], sc["config"], environment.world_size(sc["environment"]), WyRand(seed))
        pos = np.array([np.asarray(r["waypoints"][0])[:2] for r in robots])
        touches = sim.environment_contacts(colliders, vertices, pos, np.array([r["radius"] for r in robots]))
        assert touches[0].any() and pos[0, 1] == 0.0, seed      # (on the x axis: whichever way z points)


@pytest.mark.gpu
@pytest.mark.parametrize("sample_log", [True, False])
def test_environment_collisions_and_metrics(sample_log):
    scs = [_scenario("Environment Obstacles Experiment", seed, rate, _drawn_in) for rate in (0.0, 0.3) for seed in (805, 7)]
    ens, solos = _against_solo(scs, max_ticks=70, environment_collisions=True, device_metrics=True, sample_log=sample_log)
    assert all(s._dev_env_coll and s._dev_metrics for s in solos) and all(m.sim._dev_env_coll and m.sim._dev_metrics for m in ens.members)
    exports = [s.export() for s in solos]
    assert any(e["collisions"]["environment"] for e in exports)
    assert sum(s.metrics()["collisions"]["environment"] for s in solos) > 0
    assert all(sum(r["distance_travelled"] for r in s.metrics()["robots"].values()) > 0 for s in solos)   # also without the sample log
    assert _dump(exports[0]) != _dump(exports[2])                          # (the failure rate shows: the members are different runs)


@pytest.mark.gpu
def test_goal_areas_and_metrics():
    scs = [_scenario("Junction Twoway", seed) for seed in (2, 7)]
    ens, solos = _against_solo(scs, max_ticks=JUNCTION_TICKS, goal_areas="junction", device_metrics=True)
    for m, s in zip(ens.members, solos):
        assert s._dev_goals and m.sim._dev_goals
        assert _dump(m.export()["goal_areas"]) == _dump(s.export()["goal_areas"])
        assert _dump(m.metrics()["goal_areas"]) == _dump(s.metrics()["goal_areas"])
    assert sum(s.metrics()["goal_areas"]["reached"] for s in solos) >= 1      # somebody reached an exit
    assert _dump(solos[0].export()) != _dump(solos[1].export())               # (the seed shows: the members are different runs)


@pytest.mark.gpu
@pytest.mark.parametrize("option, word", [({"global_planner": True}, "global_planner"), ({"environment_collisions": "host"}, "environment_collisions"),
                                          ({"goal_areas": "junction", "device_goal_areas": False}, "device_goal_areas"),
                                          ({"device_collisions": False}, "device_collisions")])
def test_what_is_still_refused(option, word):
    sc = _scenario("Environment Obstacles Experiment")
    with pytest.raises(NotImplementedError, match=word):
        Ensemble([sc], _world(sc), **option)
