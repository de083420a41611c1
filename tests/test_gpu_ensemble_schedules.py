"""Members of an Ensemble that differ in gbp.iteration-schedule — the reference's Iteration Amount and Schedules experiments as ONE
world (mgx_mission_tick_end_groups): every member against the same scenario run by a Simulation on a world of its own,
json.dumps(export) and json.dumps(metrics) EQUAL, no tolerance, on the pattern of tests/test_gpu_ensemble_radii.py.  The Iteration
Amount Experiment is brought within reach of a short run: 10 robots on a circle of radius 12, comms radius 50 — everybody is
connected from the first tick with robots, and the robots meet in the middle well within the 80 ticks.  Members are seeds (0, 31) x
schedules (interleave-evenly 10 / 10, centered 5 / 2, interleave-evenly 1 / 3 — more external than internal iterations: segments that
are an external iteration alone).  Once more with the device's environment-collision pass and run metrics switched on."""
import copy
import json
import os

import pytest

from magics_amd import World, config, sim
from magics_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS, CIRCLE, SEEDS, TICKS = 10, 12.0, (0, 31), 80
SCHEDULES = (("interleave-evenly", 10, 10), ("centered", 5, 2), ("interleave-evenly", 1, 3))


def _scenario(seed, schedule):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)["Iteration Amount Experiment"]
    sc["config"]["simulation"]["prng-seed"] = seed
    kind, internal, external = schedule
    sc["config"]["gbp"]["iteration-schedule"] = {"schedule": kind, "internal": internal, "external": external}
    f = sc["formation"]["formations"][0]
    f["robots"] = ROBOTS
    f["initial-position"]["shape"]["radius"] = CIRCLE
    f["waypoints"][0]["shape"]["radius"] = CIRCLE
    return sc


def _world(sc):
    return World(config.world_params(sc["config"]))


def _dump(export):
    return json.dumps(export, sort_keys=True)


@pytest.mark.parametrize("options", [{}, {"environment_collisions": True, "device_metrics": True}], ids=["plain", "observers"])
def test_iteration_schedules_as_one_world(options):
    scs = [_scenario(seed, schedule) for schedule in SCHEDULES for seed in SEEDS]
    ens = Ensemble([copy.deepcopy(sc) for sc in scs], _world(scs[0]), **options).run(max_ticks=TICKS)
    solos = []
    for m, sc in enumerate(scs):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **options).run(max_ticks=TICKS)
        assert len(solo.robots) == ROBOTS
        assert ens.members[m].tick_no == solo.tick_no, m
        assert _dump(ens.members[m].export()) == _dump(solo.export()), m
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), m
        solos.append(solo)
    for k in range(len(SEEDS)):                      # the same seed under the three schedules: three different runs
        runs = [solos[k + len(SEEDS) * j] for j in range(len(SCHEDULES))]
        assert len({r.cfg["simulation"]["prng-seed"] for r in runs}) == 1
        assert len({_dump(r.export()) for r in runs}) == len(SCHEDULES)
        assert all(r.events and r.events[0][1] == ROBOTS * (ROBOTS - 1) for r in runs)   # everybody connected in the first tick with robots
    calls, launches, sat_out = ens.world.group_schedule_stats()
    assert calls > 0 and launches > calls and sat_out > 0      # the ticks ran mixed, and the shorter schedules sat launches out
