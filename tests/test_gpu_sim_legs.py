"""A global-planner mission of three taskpoints through the scenario runner (tests/sim_legs_common.py: Solo GP with an
intermediate taskpoint): the robot plans taskpoint 0 -> 1 when it spawns and 1 -> 2 when the first route ends — Idle in between,
complete only at the third taskpoint — with the engine's planner, its host restatement and the plans that ride the ticks; chunked
and tick by tick; export and metrics."""
import json

import numpy as np
import pytest

from magics_amd import World, config, sim
from magics_amd import global_planner as gp
from sim_legs_common import BUDGET, OVERRIDES, expected, scenario

pytestmark = pytest.mark.gpu

F = np.float32
MAX_TICKS = 600


class _Run:
    """one run, with what went to the planner and what came back to the world noted as it happened"""

    def __init__(self, mode, chunk=1, **options):
        sc = self.sc = scenario()
        self.w = World(config.world_params(sc["config"]))
        self.s = s = sim.Simulation(sc, self.w, global_planner=mode, planner_overrides=OVERRIDES, plan_budget=BUDGET, **options)
        self.applied, self.requests, self.states = [], [], []
        apply_, plan_ = self.w.apply_global_paths, s._plan

        def apply_spy(robots, paths, means, **kw):
            self.applied.append((s.tick_no, [int(r) for r in robots], [np.array(p, F) for p in paths], dict(kw), self.w.layout_stats()))
            out = apply_(robots, paths, means, **kw)
            self.applied[-1] += (self.w.layout_stats(),)
            return out

        def plan_spy():
            self.requests += [(s.tick_no,) + tuple(q) for q in s._plan_requests]
            return plan_()
        self.w.apply_global_paths, s._plan = apply_spy, plan_spy
        if chunk == 1:
            while not s.finished() and s.tick_no < MAX_TICKS:
                s.tick()
                r = s.robots[0]
                self.states.append((bool(r["idle"]), bool(r["completed"]), r["leg"], s.translation[0].copy()))
        else:
            s.run(max_ticks=MAX_TICKS, chunk=chunk)
        self.export = s.export()
        self.json = json.dumps(self.export, sort_keys=True)


@pytest.fixture(scope="module")
def want():
    return expected(scenario())


@pytest.fixture(scope="module")
def runs():
    return {"device": _Run(True), "host": _Run("host"), "sliced": _Run("sliced"), "device chunked": _Run(True, chunk=256),
            "sliced chunked": _Run("sliced", chunk=256), "device metrics": _Run(True, chunk=256, device_metrics=True)}


def test_both_legs_are_planned_at_the_first_attempt(want):
    """a condition of everything below, not a measurement: the taskpoints were chosen so"""
    assert len(want["taskpoints"]) == 3 and len(want["legs"]) == 2
    for leg in want["legs"]:
        assert leg["result"]["status"] == gp.PLAN_OK and len(leg["result"]["path"]) >= 2
    assert want["legs"][0]["slices"] >= 2 and want["legs"][1]["slices"] >= 2  # (riding the ticks makes a difference)


def test_device_and_host_planner_give_the_same_export(runs):
    assert runs["device"].json == runs["host"].json
    gpx = runs["device"].export["global_planner"]
    assert gpx["failed"] == [] and [q["robot"] for q in gpx["requests"]] == [0, 0] and all(q["status"] == 0 for q in gpx["requests"])


@pytest.mark.parametrize("mode", ["device", "host", "sliced"])
def test_every_leg_is_requested_planned_and_applied(runs, want, mode):
    r = runs[mode]
    rob = r.s.robots[0]
    assert r.s.finished() and rob["completed"] and len(r.requests) == len(r.applied) == 2
    ended = [None] + [leg["end_tick"] for leg in rob["routes"]]   # the tick leg k - 1 ended in (leg 0: it spawned in tick 0)
    for k, leg in enumerate(want["legs"]):
        tick, rid, start, end, state = r.requests[k]
        # the request: between the taskpoints' own positions, from the robot's forked stream as it stands, in the tick the leg before
        # it ended (leg 0: the tick it spawned in)
        assert (rid, start, end, state) == (0,) + leg["request"] and state == rob["rng"].state
        assert tick == (0 if k == 0 else ended[k])
        at, robots, paths, kw, before, after = r.applied[k]
        assert robots == [0] and kw == {"reset_tracking": True, "route": True, "activate": True}
        assert paths[0].tobytes() == leg["result"]["path"].tobytes()
        assert before == after  # in place, at the spawn and between the legs: nothing pulled, nothing laid out again
        # applied at the start of the next tick — or, riding the ticks, of the tick that many slices on
        assert at == tick + (leg["slices"] if mode == "sliced" else 1), (k, at, tick)
        assert [q["n_points"] for q in r.export["global_planner"]["requests"]][k] == len(leg["result"]["path"])


def test_sliced_gives_the_same_paths(runs):
    a, b = runs["device"], runs["sliced"]
    assert [p[2][0].tobytes() for p in a.applied] == [p[2][0].tobytes() for p in b.applied]
    assert a.export["global_planner"] == b.export["global_planner"]
    ra, rb = a.export["robots"]["0"], b.export["robots"]["0"]
    assert [x["waypoints"] for x in ra["mission"]["routes"]] == [x["waypoints"] for x in rb["mission"]["routes"]]
    assert ra["positions"] == rb["positions"] and len(ra["positions"]) > 50  # the same way, later


@pytest.mark.parametrize("mode", ["device", "sliced"])
def test_export_has_the_taskpoints_and_one_route_per_leg(runs, want, mode):
    r = runs[mode]
    m = r.export["robots"]["0"]["mission"]
    tps = [[float(F(x)), float(F(y))] for x, y in want["taskpoints"]]
    assert m["waypoints"] == tps and len(m["routes"]) == 2
    for k, route in enumerate(m["routes"]):
        assert route["waypoints"][0] == tps[k] and route["waypoints"][-1] == tps[k + 1]
        assert np.array(route["waypoints"], F).tobytes() == want["legs"][k]["result"]["path"].tobytes()
    end = r.s.robots[0]["routes"][0]["end_tick"]
    assert m["routes"][0]["started_at"] == m["started_at"] == 0.0
    assert m["routes"][0]["finished_at"] == m["routes"][1]["started_at"] == end * r.s.dt_ns * 1e-9
    assert m["routes"][1]["finished_at"] == m["finished_at"] == (len(r.states) - 1) * r.s.dt_ns * 1e-9 > m["routes"][1]["started_at"]
    assert r.export["makespan"] == len(r.states) * r.s.dt_ns * 1e-9


@pytest.mark.parametrize("mode", ["device", "sliced"])
def test_idle_between_the_legs_and_complete_only_at_the_third_taskpoint(runs, want, mode):
    r = runs[mode]
    end = r.s.robots[0]["routes"][0]["end_tick"]
    woke = r.applied[1][0]
    first = r.applied[0][0]
    assert first < end < woke
    for tick, (idle, completed, leg, tr) in enumerate(r.states):
        assert idle == (tick < first or end <= tick < woke), tick   # (as it stands behind tick `tick`)
        assert completed == (tick == len(r.states) - 1), tick
        assert leg == (0 if tick < end else 1), tick
    # it waits where the first leg left it: within its radius of the second taskpoint, and does not move
    held = [tr for (_, _, _, tr) in r.states[end:woke]]
    assert len(held) == woke - end and all(np.array_equal(x, held[0]) for x in held)
    radius = r.export["robots"]["0"]["radius"]
    assert np.hypot(*(held[0][[0, 2]] - np.array(want["taskpoints"][1]))) < 2 * radius
    assert not np.array_equal(r.states[woke][3], held[0])
    assert np.hypot(*(r.states[-1][3][[0, 2]] - np.array(want["taskpoints"][2]))) < 2 * radius


@pytest.mark.parametrize("mode", ["device", "sliced"])
def test_chunked_run_equals_the_tick_by_tick_run(runs, mode):
    a, b = runs[mode], runs[mode + " chunked"]
    assert [(p[0], p[2][0].tobytes()) for p in a.applied] == [(p[0], p[2][0].tobytes()) for p in b.applied]
    assert [q[1:] for q in a.requests] == [q[1:] for q in b.requests]
    assert a.json == b.json


def test_device_metrics_equal_the_host_streaming_form(runs):
    dev, host = runs["device metrics"], runs["device chunked"]
    assert dev.json == host.json
    a, b = dev.s.metrics(), host.s.metrics()
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    rec = a["robots"]["0"]
    assert rec["n_positions"] > 50 and rec["n_unrouted"] == 0 and np.isfinite(rec["path_deviation"]) and np.isfinite(rec["ldj"])
    # both legs' samples were measured, each against its own leg's path: against the first leg's path alone — two points, the line
    # x = -87.5 — the second leg's last samples, taken within two radii (4 m) of its taskpoint 25 m to the side, lie over 20 m off
    r = host.s.robots[0]
    from magics_amd import track_metrics as tm
    one = tm.stream([(v["velocity"][0], v["velocity"][2]) for v in r["velocities"]], r["positions"], r["routes"][0]["waypoints"])
    assert one["deviation_max"] > 20.0 and rec["max_deviation"] < one["deviation_max"]
