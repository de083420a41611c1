"""The Solo GP scenario (one robot of `planning-strategy: rrt-star`) through the scenario runner with the global
planner: the engine's planner and its host restatement give the same export; a robot spawns Idle, is planned for in the tick it
spawns, gets its path at the start of the next tick, follows it to the end and keeps clear of the map's colliders."""
import json
import os

import numpy as np
import pytest

from magics_amd import World, config, hostlib, sim
from magics_amd import global_planner as gp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLO_GP = os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP")
# the reference's sampler (+-2000 on a 250 x 175 maze) grows the tree from its hull only and does not get round the first corner in
# any number of iterations a test can wait for: the runs below sample about the map's half width
OVERRIDES = {"sample_half_extent": 125.0, "max_iterations": 20000}


def _scenario():
    return config.load_scenario(SOLO_GP)


class _Run:
    def __init__(self, mode):
        sc = _scenario()
        self.sc = sc
        self.w = World(config.world_params(sc["config"]))
        self.applied = []
        inner = self.w.apply_global_paths

        def spy(robots, paths, means, **kw):
            self.applied.append(([int(r) for r in robots], [np.array(p, np.float32) for p in paths], dict(kw)))
            return inner(robots, paths, means, **kw)
        self.w.apply_global_paths = spy
        self.s = sim.Simulation(sc, self.w, global_planner=mode, planner_overrides=OVERRIDES)
        s = self.s
        s.tick()                                        # the tick the first robot spawns in
        self.spawned_at = s.translation[0].copy()
        self.after_spawn_tick = (len(s.robots), bool(s.robots[0]["idle"]), len(self.applied), len(s._plans_ready))
        self.request = (tuple(float(v) for v in s.robots[0]["waypoints"][0][:2]), tuple(float(v) for v in s.robots[0]["waypoints"][1][:2]),
                        s.robots[0]["rng"].state)
        s.tick()
        self.after_next_tick = (bool(s.robots[0]["idle"]), len(self.applied))
        self.route = np.array([w_[:2] for w_ in s.robots[0]["waypoints"]], np.float32)
        s.tick()
        self.moved_to = s.translation[0].copy()
        s.run()
        self.export = s.export()


@pytest.fixture(scope="module")
def runs():
    return {mode: _Run(mode) for mode in (True, "host")}


def test_device_and_host_planner_give_the_same_export(runs):
    a, b = (json.dumps(runs[m].export, sort_keys=True) for m in (True, "host"))
    assert a == b
    gpx = runs[True].export["global_planner"]
    assert len(gpx["requests"]) == len(runs[True].export["robots"]) == 1 and gpx["failed"] == [] and all(q["status"] == 0 and q["n_points"] >= 2 for q in gpx["requests"])


@pytest.mark.parametrize("mode", [True, "host"], ids=["device", "host"])
def test_spawn_plan_apply(runs, mode):
    r = runs[mode]
    # the tick it spawns: idle, where it spawned, planned for but nothing applied
    assert r.after_spawn_tick == (1, True, 0, 1)
    assert tuple(r.spawned_at[[0, 2]]) == tuple(np.float32(r.request[0]))
    # the start of the next tick: ONE call with route, activation and the tracking factors' reset; the planned path
    assert r.after_next_tick == (False, 1)
    robots, paths, kw = r.applied[0]
    assert robots == [0] and kw == {"reset_tracking": True, "route": True, "activate": True}
    sc = r.sc
    want = gp.plan_paths(sc["environment"], [r.request], gp.params_from_config(sc["config"], **OVERRIDES))[0]
    assert want["status"] == gp.PLAN_OK and len(want["path"]) >= 3
    assert paths[0].tobytes() == want["path"].tobytes() == r.route.tobytes()
    assert tuple(paths[0][0]) == tuple(np.float32(r.request[0])) and tuple(paths[0][-1]) == tuple(np.float32(r.request[1]))
    # ... which it follows from then on
    assert not np.array_equal(r.moved_to, r.spawned_at)
    assert len(r.applied) == 1


def test_finishes_in_time_and_clear_of_the_colliders(runs):
    r = runs[True]
    ex, s = r.export, r.s
    assert s.finished() and ex["makespan"] < r.sc["config"]["simulation"]["max-time"] and ex["makespan"] < 200.0
    cols, verts = hostlib.env_colliders(r.sc["environment"])
    for rid, rob in ex["robots"].items():
        pos = np.array(rob["positions"], np.float32)
        assert len(pos) > 100 and rob["planning_strategy"] == "rrt-star"
        touching = sim.environment_contacts(cols, verts, pos, np.full(len(pos), rob["radius"], np.float32))
        assert not touching.any(), (rid, np.nonzero(touching.any(axis=1))[0][:5])
        goal = np.array(rob["mission"]["waypoints"][-1])
        assert np.hypot(*(pos[-1] - goal)) < 3 * rob["radius"]


def test_without_the_option_the_strategy_is_still_rejected():
    sc = _scenario()
    s = sim.Simulation(sc, World(config.world_params(sc["config"])))
    with pytest.raises(NotImplementedError, match="rrt-star"):
        s.tick()
