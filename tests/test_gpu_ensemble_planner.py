"""Members of an Ensemble whose robots are `planning-strategy: rrt-star` — the reference's Collaborative GP experiment
(scripts/run-collaborative-gp-experiment.fish: seeds x tracking off / on x sigma-factor-tracking 0.15 / 0.5), which
tests/test_gpu_ensemble_sigmas.py could only stand in for — as ONE world whose one planner pool serves every member
(global_planner="sliced": mgx_plan_submit_groups, one collect, one apply and one slice per tick for all of them): every member
against the same scenario run by a Simulation on a world of its own with the same options, json.dumps(export) and
json.dumps(metrics) EQUAL, no tolerance.  The world is masked (the members differ in tracking on / off and in a sigma) and its
robots are planned.  Run at a budget at which every plan of the first spawn wave is back before the second wave asks, and at one
at which the second wave is submitted while the first still pends; each as group plans and with masked_resident=True."""
import copy
import json
import os

import pytest

from magics_amd import World, config, hostlib, sim
from magics_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLABORATIVE_GP = os.path.join(ROOT, "tests", "golden", "scenario_files", "Collaborative GP")
SOLO_GP = os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP")
OVERRIDES = {"sample_half_extent": 125.0, "max_iterations": 20000}
SEEDS = (0, 31)
VARIANTS = ((False, None), (True, 0.15), (True, 0.5))      # (gbp.factors-enabled.tracking, gbp.sigma-factor-tracking; None: the scenario's own)
KEYS = [(variant, seed) for variant in VARIANTS for seed in SEEDS]
# 10 Hz: the formations with delay 0 spawn in tick 0, those with delay 5 s fifty ticks on.  The first wave's requests take up to 23
# slices at a budget of 256 and up to 89 at 64 (the restatement's figures): 100 ticks hold both waves and every plan of the first
TICKS = 100
BUDGETS = (256, 64)


def _dump(export):
    return json.dumps(export, sort_keys=True)


def _member(key, where=COLLABORATIVE_GP):
    (tracking, sigma), seed = key
    sc = config.load_scenario(where)
    sc["config"]["simulation"]["prng-seed"] = seed
    sc["config"]["gbp"]["factors-enabled"]["tracking"] = tracking
    if sigma is not None:
        sc["config"]["gbp"]["sigma-factor-tracking"] = config.f32(sigma)
    return sc


def _world(sc):
    return World(config.world_params(sc["config"]))


def _options(budget, mode="sliced"):
    return {"global_planner": mode, "planner_overrides": OVERRIDES, "plan_budget": budget}


@pytest.fixture(scope="module")
def solos():
    """every member run by a Simulation on a world of its own, once per budget: (budget, key) -> (export, metrics) as text"""
    out = {}
    for budget in BUDGETS:
        for key in KEYS:
            sc = _member(key)
            solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **_options(budget)).run(max_ticks=TICKS)
            assert solo.tick_no == TICKS
            out[(budget, key)] = (_dump(solo.export()), _dump(solo.metrics()))
        for variant in VARIANTS:                            # different seeds: different runs
            assert out[(budget, (variant, SEEDS[0]))][0] != out[(budget, (variant, SEEDS[1]))][0]
    return out


class _Spied:
    """an Ensemble whose world's planner calls are counted per Ensemble tick"""

    def __init__(self, scs, **options):
        self.world = w = _world(scs[0])
        self.ticks = []          # per tick: {"applies": n, "waits": n, "collects": n, "submits": [(groups, pending before)]}
        self.before = {"applies": 0, "waits": 0, "collects": 0, "submits": []}   # what the constructor and run()'s ends did
        self._now = self.before
        apply, collect, submit = w.apply_global_paths, w.plan_collect, w.plan_submit

        def spy_apply(robots, paths, means, **kw):
            self._now["applies"] += 1
            return apply(robots, paths, means, **kw)

        def spy_collect(wait=False, **kw):
            self._now["collects"] += 1
            self._now["waits"] += 1 if wait else 0
            return collect(wait=wait, **kw)

        def spy_submit(requests, groups=None):
            self._now["submits"].append((None if groups is None else [int(g) for g in groups], w.plan_pending()))
            return submit(requests, groups=groups)
        w.apply_global_paths, w.plan_collect, w.plan_submit = spy_apply, spy_collect, spy_submit
        self.ens = e = Ensemble([copy.deepcopy(sc) for sc in scs], w, **options)
        tick = e.tick

        def spy_tick():
            self._now = {"applies": 0, "waits": 0, "collects": 0, "submits": []}
            self.ticks.append(self._now)
            tick()
            self._now = self.before
        e.tick = spy_tick

    def check_calls(self):
        """per Ensemble tick: at most one apply, at most one collect that waits; every submit under ONE member's group"""
        assert self.before == {"applies": 0, "waits": 0, "collects": 0, "submits": []}
        assert max(t["applies"] for t in self.ticks) == 1 and max(t["waits"] for t in self.ticks) == 1
        submitted = {}
        for t in self.ticks:
            for groups, _ in t["submits"]:
                assert groups is not None and len(set(groups)) == 1 and 0 <= groups[0] < len(self.ens.members)
                submitted[groups[0]] = submitted.get(groups[0], 0) + len(groups)
        for g, m in enumerate(self.ens.members):        # a member's requests went in under its group (what still pended at its end is not logged)
            assert submitted.get(g, 0) >= len(m.export()["global_planner"]["requests"]) > 0, g


@pytest.mark.parametrize("masked_resident", [False, True], ids=["group-plans", "masked-resident"])
@pytest.mark.parametrize("budget", BUDGETS)
def test_collaborative_gp_sweep_as_one_world(solos, budget, masked_resident):
    scs = [_member(key) for key in KEYS]
    run = _Spied(scs, masked_resident=masked_resident, **_options(budget))
    ens = run.ens.run(max_ticks=TICKS)
    assert ens.world.plan_pending() == 0
    for m, key in enumerate(KEYS):
        member = ens.members[m]
        assert member.tick_no == TICKS, m
        export = member.export()
        assert _dump(export) == solos[(budget, key)][0], (m, key)
        assert _dump(member.metrics()) == solos[(budget, key)][1], (m, key)
        assert export["global_planner"]["failed"] == [] and export["global_planner"]["requests"], (m, key)
        # both spawn waves fall inside the run, and every plan of the first has been applied and its robot has moved
        robots, forms = member.sim.robots, member.sim.formations
        first = [r for r in robots if forms[r["formation"]]["delay"] == 0 and r["started_at"] == 0.0]
        second = [r for r in robots if forms[r["formation"]]["delay"] == 5_000_000_000]
        assert len(first) == 4 and len(second) == 4, (m, key)
        planned = {q["robot"] for q in export["global_planner"]["requests"]}
        for r in first:
            assert r["id"] in planned and not r["idle"] and r["travelled"] > 0.0, (m, key, r["id"])
    # the members' own requests: a robot's plan is not another member's (different seeds, different streams)
    assert _dump(ens.members[0].export()["global_planner"]) != _dump(ens.members[1].export()["global_planner"])
    # the one pool: requests still pending when a tick submits, at the small budget; never at the large one
    behind = [t["submits"][0][1] for t in run.ticks if t["submits"]]   # (what earlier ticks left pending when a tick first submits)
    assert len(behind) >= 2 and (max(behind) > 0) == (budget == 64), (budget, behind)
    run.check_calls()
    # a masked world all the same: the members differ in their kinds and in a sigma
    assert ens.world.group_enabled_stats()[0] > 0
    assert (ens.world.group_resident_stats()[0] > 0) == masked_resident


def test_a_member_retired_with_a_request_pending_leaves_none(solos):
    """max_ticks ends every member while its first requests still pend (no plan takes fewer than 9 slices at a budget of 64)"""
    scs = [_member(key) for key in KEYS[:3]]
    run = _Spied(scs, **_options(64))
    ens = run.ens
    for _ in range(3):
        ens.tick()
    assert ens.world.plan_pending() == 12 and [m._view.plan_pending() for m in ens.members] == [4, 4, 4]
    ens.run(max_ticks=3)
    assert all(m.retired and m.tick_no == 3 for m in ens.members)
    assert ens.world.plan_pending() == 0 and [m._view.plan_pending() for m in ens.members] == [0, 0, 0]
    for m, key in enumerate(KEYS[:3]):
        sc = _member(key)
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **_options(64)).run(max_ticks=3)
        assert _dump(ens.members[m].export()) == _dump(solo.export()), (m, key)
        assert ens.members[m].export()["global_planner"] == {"requests": [], "failed": []}


def test_members_that_differ_in_rrt_collision_radius():
    """rrt.collision-radius per member: member 1's is a parameter set of group 1 (mgx_planner_set_group_params)"""
    scs = [_member(((False, None), 0)), _member(((False, None), 0))]
    scs[1]["config"]["rrt"]["collision-radius"] = config.f32(1.5)
    run = _Spied(scs, **_options(256))
    ens = run.ens.run(max_ticks=40)
    own = config.f32(scs[0]["config"]["rrt"]["collision-radius"])
    assert own != config.f32(1.5)
    assert ens.world.planner_group_params(0)["collision_radius"] == own
    assert ens.world.planner_group_params(1)["collision_radius"] == config.f32(1.5)
    assert {k: v for k, v in ens.world.planner_group_params(1).items() if k != "collision_radius"} == \
        {k: v for k, v in ens.world.planner_group_params(0).items() if k != "collision_radius"}
    texts = []
    for m, sc in enumerate(scs):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **_options(256)).run(max_ticks=40)
        texts.append(_dump(solo.export()))
        assert _dump(ens.members[m].export()) == texts[m], m
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), m
        assert solo.export()["global_planner"]["requests"] and solo.export()["global_planner"]["failed"] == []
    assert texts[0] != texts[1]                             # (the radius shows: other plans, another run)
    run.check_calls()
    assert ens.world.plan_pending() == 0


def test_members_on_the_host_restatement():
    """global_planner="host": each member's requests under its own parameters by the restatement; the engine's planner stays off"""
    scs = [_member(((False, None), seed), SOLO_GP) for seed in SEEDS]
    scs[1]["config"]["rrt"]["collision-radius"] = config.f32(1.5)
    run = _Spied(scs, **_options(64, "host"))
    ens = run.ens.run(max_ticks=30)
    for m, sc in enumerate(scs):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **_options(64, "host")).run(max_ticks=30)
        assert _dump(ens.members[m].export()) == _dump(solo.export()), m
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), m
        assert len(solo.export()["global_planner"]["requests"]) == 1 and not solo.robots[0]["idle"]
    assert max(t["applies"] for t in run.ticks) == 1 and all(t["collects"] == 0 and t["submits"] == [] for t in run.ticks)
    with pytest.raises(hostlib.MgxError, match="planner is off"):
        ens.world.planner_group_params(0)


def test_solo_gp_two_seeds_to_the_end_of_the_mission():
    scs = [_member(((False, None), seed), SOLO_GP) for seed in SEEDS]
    run = _Spied(scs, **_options(64))
    ens = run.ens.run()
    for m, sc in enumerate(scs):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **_options(64)).run()
        assert solo.finished() and ens.members[m].sim.finished() and ens.members[m].tick_no == solo.tick_no
        assert _dump(ens.members[m].export()) == _dump(solo.export()), m
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), m
        assert solo.robots and all(r["completed"] and r["travelled"] > 0.0 for r in solo.robots)
    assert _dump(ens.members[0].export()) != _dump(ens.members[1].export())
    run.check_calls()
    assert ens.world.plan_pending() == 0


def test_what_the_ensemble_says_about_its_planner():
    scs = [_member(key) for key in KEYS[:2]]
    with pytest.raises(NotImplementedError, match="sliced"):
        Ensemble(copy.deepcopy(scs), _world(scs[0]), global_planner=True)
    with pytest.raises(NotImplementedError, match="rrt-star"):
        Ensemble(copy.deepcopy(scs), _world(scs[0]))
