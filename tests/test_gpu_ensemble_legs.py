"""Missions of several legs in an Ensemble: two members of the three-taskpoint Solo GP scenario (tests/sim_legs_common.py) with
different seeds under `Ensemble(..., global_planner="sliced")` — the ensemble reads the robots that ended a leg once per tick, routes
them to their members by id, and each member's next-leg request goes out under its group — against the same scenarios run by a
Simulation on a world of its own: json.dumps(export) EQUAL, no tolerance."""
import copy
import json

import pytest

from magics_amd import World, config, sim
from magics_amd import global_planner as gp
from magics_amd.ensemble import Ensemble
from sim_legs_common import BUDGET, OVERRIDES, SEEDS, expected, scenario

pytestmark = pytest.mark.gpu

MAX_TICKS = 600
OPTIONS = {"global_planner": "sliced", "planner_overrides": OVERRIDES, "plan_budget": BUDGET}


def _dump(x):
    return json.dumps(x, sort_keys=True)


def test_each_member_equals_its_solo_run():
    scs = [scenario(seed) for seed in SEEDS]
    for sc in scs:   # the condition: every leg of every member is planned at the first attempt
        assert all(leg["result"]["status"] == gp.PLAN_OK for leg in expected(sc)["legs"])
    solos = []
    for sc in scs:
        s = sim.Simulation(copy.deepcopy(sc), World(config.world_params(sc["config"])), **OPTIONS).run(max_ticks=MAX_TICKS)
        assert s.finished() and len(s.export()["robots"]["0"]["mission"]["routes"]) == 2
        solos.append((_dump(s.export()), _dump(s.metrics())))
    assert solos[0][0] != solos[1][0]   # different seeds: different runs
    ens = Ensemble([copy.deepcopy(sc) for sc in scs], World(config.world_params(scs[0]["config"])), **OPTIONS).run(max_ticks=MAX_TICKS)
    for m, (export, metrics) in zip(ens.members, solos):
        assert m.retired and m.sim.finished()
        assert _dump(m.export()) == export
        assert _dump(m.metrics()) == metrics
