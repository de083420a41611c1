"""Members of an Ensemble that differ in robot.communication.radius — the reference's Varying Network Connectivity Experiment as ONE
world: every member against the same scenario run by a Simulation on a world of its own, json.dumps(export) and
json.dumps(metrics) EQUAL, no tolerance.  The scenario is brought within reach of a short run as tests/test_gpu_ensemble.py shortens
the Circle: 10 robots on a circle of radius 12; members are seeds (0, 31) x radii (5, 30).  On that circle the nearest two
robots are 7.4 apart and the farthest 24: under radius 5 nobody is connected until the robots have closed in, under 30 everybody is
from the first tick (checked with the numpy predicate below) — so members that differ only in radius must differ in their events
and their exports."""
import copy
import json
import os

import numpy as np
import pytest

from magics_amd import World, config, sim
from magics_amd.ensemble import Ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS, CIRCLE, SEEDS, RADII, TICKS = 10, 12.0, (0, 31), (5.0, 30.0), 80
F = np.float32


def _scenario(name, seed=None, radius=None, tweak=None):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)[name]
    if seed is not None:
        sc["config"]["simulation"]["prng-seed"] = seed
    if radius is not None:
        sc["config"]["robot"]["communication"]["radius"] = radius
    if tweak:
        tweak(sc)
    return sc


def _short(sc):
    f = sc["formation"]["formations"][0]
    f["robots"] = ROBOTS
    f["initial-position"]["shape"]["radius"] = CIRCLE
    f["waypoints"][0]["shape"]["radius"] = CIRCLE


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


def test_the_circle_straddles_the_radii():
    sc = _scenario("Varying Network Connectivity Experiment", tweak=_short)
    f = sc["formation"]["formations"][0]
    assert f["initial-position"]["placement-strategy"][0] == "equal" and f["initial-position"]["shape"]["kind"] == "circle"
    a = 2 * np.pi * np.arange(ROBOTS) / ROBOTS
    pos = np.stack([CIRCLE * np.cos(a), np.zeros(ROBOTS), CIRCLE * np.sin(a)], axis=1).astype(F)
    d = pos[:, None, :] - pos[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    off = ~np.eye(ROBOTS, dtype=bool)
    assert dist.dtype == F
    assert (F(RADII[0]) < dist[off]).all()           # radius 5: nobody in range at the start
    assert (~(F(RADII[1]) < dist[off])).all()        # radius 30: everybody
    assert sc["config"]["robot"]["communication"]["radius"] not in RADII


@pytest.mark.gpu
def test_varying_network_connectivity_as_one_world():
    scs = [_scenario("Varying Network Connectivity Experiment", seed, radius, _short) for radius in RADII for seed in SEEDS]
    ens, solos = _against_solo(scs, max_ticks=TICKS)
    assert all(len(s.robots) == ROBOTS for s in solos)
    for k in range(len(SEEDS)):                      # the same seed, the other radius: another run
        near, far = solos[k], solos[k + len(SEEDS)]
        assert near.cfg["simulation"]["prng-seed"] == far.cfg["simulation"]["prng-seed"]
        assert near.events != far.events and far.events
        assert _dump(near.export()) != _dump(far.export())
        assert ens.members[k].sim.events == near.events and ens.members[k + len(SEEDS)].sim.events == far.events
    assert far.events[0][1] == ROBOTS * (ROBOTS - 1)  # radius 30: everybody connects to everybody in the first tick with robots
