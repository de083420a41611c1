"""Goal areas as far as they can be checked without a device: the contact restated in numpy against answers written out by hand,
the seconds rule, the export and the metrics of a junction run on the CPU oracle (host pass), the throughput against what the
reference's own analysis function returned (tests/golden/goal_area_flow.json), the bindings and the argument errors of
mgx_goal_areas_enable.  The device pass is held against the same answers in tests/test_gpu_goal_areas.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle
from magics_amd import World, config, hostlib, sim

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNCTION = os.path.join(ROOT, "tests", "golden", "scenario_files", "Junction Experiment")
CALLS = ["mgx_goal_areas_enable", "mgx_goal_areas_set_clock", "mgx_goal_areas_update", "mgx_goal_areas_read", "mgx_goal_areas_clear"]
# 150 ticks of the Junction Experiment (10 Hz, 15 m/s, a robot per second and lane): the host pass sees 8 arrivals in each of the
# two areas, and every robot that arrived has been despawned since (tests/test_gpu_goal_areas.py runs the same ticks)
JUNCTION_TICKS = 150

NAN = F(np.nan)
UP = lambda v: np.nextafter(F(v), F(np.inf), dtype=F)    # noqa: E731
DOWN = lambda v: np.nextafter(F(v), F(-np.inf), dtype=F)  # noqa: E731
# The known answers, written out by hand — (what, area ((x0, z0), (x1, z1)), (x, z), r, touches):
#   box A = [-8, 8] x [-4, 4]: centre (0, 0), half extents (8, 4), all exact in f32
KNOWN = [
    ("centre inside", ((-8, -4), (8, 4)), (1.5, -2.0), 1.0, True),
    ("on the edge, zero radius", ((-8, -4), (8, 4)), (8.0, 0.0), 0.0, True),
    ("outside the edge x = 8 at distance exactly r", ((-8, -4), (8, 4)), (9.0, 0.0), 1.0, True),
    ("one ulp further", ((-8, -4), (8, 4)), (UP(9.0), 0.0), 1.0, False),
    ("one ulp nearer", ((-8, -4), (8, 4)), (DOWN(9.0), 0.0), 1.0, True),
    ("outside the edge z = -4 at distance exactly r", ((-8, -4), (8, 4)), (-3.0, -6.5), 2.5, True),
    ("... and one ulp further", ((-8, -4), (8, 4)), (-3.0, DOWN(-6.5)), 2.5, False),
    ("corner, e = (3, 4), r = 5: 9 + 16 <= 25", ((-8, -4), (8, 4)), (11.0, 8.0), 5.0, True),
    ("corner, e = (3, 4), r just below 5", ((-8, -4), (8, 4)), (11.0, 8.0), DOWN(5.0), False),
    ("the opposite corner, e = (3, 4), r = 5", ((-8, -4), (8, 4)), (-11.0, -8.0), 5.0, True),
    ("swapped corners: the reference's first junction area, inside", ((-8, -48), (8, -52)), (0.0, -50.0), 1.0, True),
    ("swapped corners, outside z = -48 at distance exactly r", ((-8, -48), (8, -52)), (0.0, -47.0), 1.0, True),
    ("swapped corners, one ulp further", ((-8, -48), (8, -52)), (0.0, UP(-47.0)), 1.0, False),
    ("swapped in both axes", ((8, -48), (-8, -52)), (9.0, -50.0), 1.0, True),
    ("zero extent: a point, e = (3, 4), r = 5", ((2, 3), (2, 3)), (5.0, 7.0), 5.0, True),
    ("zero extent, r just below 5", ((2, 3), (2, 3)), (5.0, 7.0), DOWN(5.0), False),
    ("zero extent, on the point with zero radius", ((2, 3), (2, 3)), (2.0, 3.0), 0.0, True),
    ("NaN x", ((-8, -4), (8, 4)), (NAN, 0.0), 1.0, False),
    ("NaN z", ((-8, -4), (8, 4)), (0.0, NAN), 1.0, False),
    ("NaN radius, centre inside", ((-8, -4), (8, 4)), (0.0, 0.0), NAN, False),
    ("far away", ((-8, -4), (8, 4)), (1000.0, -1000.0), 1.0, False),
]


@pytest.mark.parametrize("what,area,p,r,touches", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_answers(what, area, p, r, touches):
    got = sim.goal_area_contacts([area], np.array([p], dtype=F), np.array([r], dtype=F))
    assert got.shape == (1, 1) and got.dtype == bool and bool(got[0, 0]) is touches, what


def test_known_answers_as_one_table_and_swapped_equals_sorted():
    areas = [k[1] for k in KNOWN]
    pos, rad = np.array([k[2] for k in KNOWN], dtype=F), np.array([k[3] for k in KNOWN], dtype=F)
    table = sim.goal_area_contacts(areas, pos, rad)
    assert table.shape == (len(KNOWN), len(KNOWN))
    assert [bool(table[i, i]) for i in range(len(KNOWN))] == [k[4] for k in KNOWN]
    srt = [((min(a[0][0], a[1][0]), min(a[0][1], a[1][1])), (max(a[0][0], a[1][0]), max(a[0][1], a[1][1]))) for a in areas]
    assert np.array_equal(table, sim.goal_area_contacts(srt, pos, rad))
    lo, hi = sim.goal_area_boxes([((-8, -48), (8, -52))])
    assert lo.tolist() == [[-8.0, -52.0]] and hi.tolist() == [[8.0, -48.0]] and lo.dtype == F
    assert sim.JUNCTION_GOAL_AREAS == (((-8.0, -48.0), (8.0, -52.0)), ((48.0, -8.0), (52.0, 8.0)))


@pytest.mark.parametrize("k", [0, 9, 10, 655, 123456])
def test_seconds_rule(k):
    tick_ns = 100_000_000
    secs, nanos = divmod((k + 1) * tick_ns, 10**9)
    want = np.float32(secs) + np.float32(nanos) / np.float32(1e9)
    assert isinstance(want, np.float32)
    got = hostlib.goal_seconds(k, tick_ns)
    assert type(got) is float and got == float(want) and np.float32(got) == want
    assert json.loads(json.dumps(got)) == got


@pytest.fixture(scope="module")
def junction_run():
    sc = config.load_scenario(JUNCTION)
    s = sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"])), goal_areas="junction")
    s.run(max_ticks=JUNCTION_TICKS)
    return s, s.export(), s.metrics()


def test_export_and_metrics_on_the_cpu_oracle(junction_run):
    s, exp, met = junction_run
    assert s.tick_no == JUNCTION_TICKS and not s.dev
    ga = exp["goal_areas"]
    assert list(ga) == ["0", "1"]
    assert ga["0"]["aabb"] == {"mins": [-8.0, -52.0], "maxs": [8.0, -48.0]} and ga["1"]["aabb"] == {"mins": [48.0, -8.0], "maxs": [52.0, 8.0]}
    n = [len(a["history"]) for a in ga.values()]
    assert sum(n) >= 4 and min(n) >= 1, n
    seen = set()
    for a, area in ga.items():
        for rid, t in area["history"].items():
            assert rid in exp["robots"], rid
            assert type(t) is float and t >= exp["robots"][rid]["mission"]["started_at"], (rid, t)
            assert (a, rid) not in seen  # (JSON object keys: once per area by construction, and the table agrees)
            seen.add((a, rid))
    ticks = s.goal_arrivals
    assert [len(h) for h in ticks] == n and all(ga[str(a)]["history"][str(r)] == hostlib.goal_seconds(k, s.dt_ns) for a, h in enumerate(ticks) for r, k in h.items())
    assert any(not s.robots[r]["alive"] for h in ticks for r in h), "a robot despawned after arriving keeps its entry"
    assert json.loads(json.dumps(exp["goal_areas"])) == exp["goal_areas"]
    # the hand count: robots that started before the window and are in some history, per second of the window
    for window in (50.0, 5.0, 0.4):
        reached = {rid for area in ga.values() for rid in area["history"]}
        count = sum(1 for rid, r in exp["robots"].items() if r["mission"]["started_at"] < window and rid in reached)
        assert count > 0 or window == 0.4
        assert s.goal_flow(window) == sim.goal_flow(exp, window) == (1 / (window / count) if count else 0.0)
    m = met["goal_areas"]
    assert m["arrivals"] == n and m["reached"] == len({rid for area in ga.values() for rid in area["history"]})
    assert m["flow"] == sim.goal_flow(exp, 50.0) and m["window"] == 50.0
    first = {}
    for area in ga.values():
        for rid, t in area["history"].items():
            first[rid] = min(first.get(rid, t), t)
    assert m["time_to_goal"] == {rid: t - exp["robots"][rid]["mission"]["started_at"] for rid, t in sorted(first.items(), key=lambda kv: int(kv[0]))}
    assert all(v > 0 for v in m["time_to_goal"].values())


def test_without_areas_nothing_changes(junction_run):
    sc = config.load_scenario(JUNCTION)
    s = sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"])))
    s.run(max_ticks=JUNCTION_TICKS)
    exp = s.export()
    assert exp["goal_areas"] == {} and "goal_areas" not in s.metrics() and s.goal_arrivals == []
    with_areas = junction_run[1]
    assert {k: v["positions"] for k, v in exp["robots"].items()} == {k: v["positions"] for k, v in with_areas["robots"].items()}
    assert {k: v for k, v in exp.items() if k != "goal_areas"} == {k: v for k, v in with_areas.items() if k != "goal_areas"}


def test_options_are_checked():
    class NoWorld:
        pass
    empty = {"config": {}, "environment": {}, "formation": {"formations": []}}
    with pytest.raises(ValueError, match="device_goal_areas needs device_missions"):
        sim.Simulation(empty, NoWorld(), device_missions=False, goal_areas="junction", device_goal_areas=True)
    with pytest.raises(ValueError, match='or "junction"'):
        sim.Simulation(empty, NoWorld(), device_missions=False, goal_areas="crossroads")
    with pytest.raises(ValueError, match="between 1 and 64"):
        sim.Simulation(empty, NoWorld(), device_missions=False, goal_areas=[((0, 0), (1, 1))] * 65)


def test_flow_against_the_reference_function():
    with open(os.path.join(ROOT, "tests", "golden", "goal_area_flow.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 3
    for name, c in cases.items():
        assert set(c["export"]) == {"goal_areas", "robots", "makespan"}
        assert sim.goal_flow(c["export"], c["window"]) == c["flow"], name
    assert sim.goal_flow({"goal_areas": {"0": {"history": {}}}, "robots": {"0": {"mission": {"started_at": 0.0}}}}) == 0.0


def test_header_bindings_and_records_agree():
    header = open(os.path.join(ROOT, "include", "mgx.h"), encoding="utf-8").read()
    rust = open(os.path.join(ROOT, "rust", "magics-hip", "src", "sys.rs"), encoding="utf-8").read()
    L = hostlib.lib()
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in hostlib.SYMBOLS and "pub fn " + name + "(" in rust, name
        assert getattr(L, name) is not None
    assert re.search(r"#define MGX_GOAL_AREAS_MAX 64u", header) and hostlib.GOAL_AREAS_MAX == 64
    assert ctypes.sizeof(hostlib.GoalArea) == hostlib.goal_area_dtype().itemsize == 16
    assert ctypes.sizeof(hostlib.GoalArrival) == hostlib.goal_arrival_dtype().itemsize == 16
    dt = hostlib.goal_arrival_dtype()
    assert [dt.fields[f][1] for f in ("tick", "area", "robot")] == [getattr(hostlib.GoalArrival, f).offset for f in ("tick", "area", "robot")] == [0, 8, 12]
    assert "pub struct mgx_goal_area {" in rust and "pub struct mgx_goal_arrival {" in rust
    for fn in ("goal_areas_enable", "goal_areas_set_clock", "goal_areas_update", "goal_areas_read", "goal_areas_clear"):
        assert callable(getattr(World, fn)), fn


@pytest.mark.parametrize("fma", [False, True])
def test_argument_errors_need_no_device(fma):
    """what is wrong with the areas is said before the world is looked at, so also where there is no device to make a world on"""
    L = hostlib.lib(fma)
    INVALID = -1
    boxes = np.zeros(65, hostlib.goal_area_dtype())
    boxes["maxs"] = 1.0
    assert L.mgx_goal_areas_enable(None, boxes.ctypes.data, 65, 0) == INVALID and b"65 goal areas" in L.mgx_last_error()
    assert L.mgx_goal_areas_enable(None, None, 2, 0) == INVALID and b"null areas" in L.mgx_last_error()
    for field, q, bad in (("mins", 0, np.nan), ("maxs", 1, np.inf), ("mins", 1, -np.inf)):
        b = boxes[:3].copy()
        b[field][2, q] = bad
        assert L.mgx_goal_areas_enable(None, b.ctypes.data, 3, 0) == INVALID and b"goal area 2: a corner is not finite" in L.mgx_last_error()
    assert L.mgx_goal_areas_enable(None, boxes.ctypes.data, 64, 2**32 - 1) == INVALID and b"next_tick" in L.mgx_last_error()
    assert L.mgx_goal_areas_enable(None, boxes.ctypes.data, 64, 0) == INVALID and b"null world" in L.mgx_last_error()
    for call, args in (("mgx_goal_areas_set_clock", (0,)), ("mgx_goal_areas_update", (None, 0)), ("mgx_goal_areas_read", (None, 0, None, None)),
                       ("mgx_goal_areas_clear", ())):
        assert getattr(L, call)(None, *args) == INVALID, call
