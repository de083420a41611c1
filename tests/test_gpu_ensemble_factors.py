"""Members of an Ensemble that differ in gbp.factors-enabled.tracking — the reference's Structured Junction Twoway experiment
(scripts/run-structured-junction-twoway.fish: tracking on and off x the comms failure rates) as ONE world (mgx_set_group_enabled):
every member against the same scenario run by a Simulation on a world of its own, json.dumps(export) and json.dumps(metrics) EQUAL,
no tolerance, on the pattern of tests/test_gpu_ensemble_schedules.py.  The scenario is brought within reach of a short run: every
formation spawns twice instead of a hundred times, 80 ticks.  Members are tracking (on, off) x failure rate (0.0, 0.3) x seeds
(0, 31).  Once more with the device's environment-collision pass and run metrics switched on."""
import copy
import json
import os

import pytest

from magics_amd import World, config, sim
from magics_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAWNS, SEEDS, RATES, TICKS = 2, (0, 31), (0.0, 0.3), 80


def _scenario(seed, rate, tracking):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)["Structured Junction Twoway"]
    sc["config"]["simulation"]["prng-seed"] = seed
    sc["config"]["robot"]["communication"]["failure-rate"] = rate
    sc["config"]["gbp"]["factors-enabled"]["tracking"] = tracking
    for f in sc["formation"]["formations"]:
        f["repeat"]["times"] = SPAWNS
    return sc


def _world(sc):
    return World(config.world_params(sc["config"]))


def _dump(export):
    return json.dumps(export, sort_keys=True)


@pytest.mark.parametrize("options", [{}, {"environment_collisions": True, "device_metrics": True}], ids=["plain", "observers"])
def test_tracking_on_and_off_as_one_world(options):
    keys = [(tracking, rate, seed) for tracking in (True, False) for rate in RATES for seed in SEEDS]
    scs = [_scenario(seed, rate, tracking) for tracking, rate, seed in keys]
    ens = Ensemble([copy.deepcopy(sc) for sc in scs], _world(scs[0]), **options).run(max_ticks=TICKS)
    assert [ens.world.group_enabled(m) for m in range(len(scs))] == [config.enable_mask(sc["config"]) for sc in scs]
    solos = {}
    for m, (key, sc) in enumerate(zip(keys, scs)):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **options).run(max_ticks=TICKS)
        assert len(solo.robots) > 2
        assert ens.members[m].tick_no == solo.tick_no == TICKS, m
        assert _dump(ens.members[m].export()) == _dump(solo.export()), (m, key)
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), (m, key)
        solos[key] = solo
    for rate in RATES:                               # the same seed and rate with tracking on and off: two different runs
        for seed in SEEDS:
            assert _dump(solos[(True, rate, seed)].export()) != _dump(solos[(False, rate, seed)].export()), (rate, seed)
    plans, launches = ens.world.group_enabled_stats()
    assert plans > 0 and launches > plans            # the ticks ran as group plans, launch by launch
    assert ens.world.group_schedule_stats() == (0, 0, 0) and ens.world.resident_stats()[0] == 0
