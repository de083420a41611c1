"""The run metrics without a device: magics_amd/track_metrics.py against the values the reference's own functions gave
(tests/golden/track_metrics.json, made by tests/golden/make_track_metrics.py), its streaming form against its batch form, the lane
arithmetic of magics_amd/csrc/mgx_track_metrics.h in a host build against the streaming form bit for bit, and the interface.

TOLERANCES.  Measured when the fixture was made (numpy 2.2.6 / scipy 1.15.3, profiles/track_metrics.md): the batch restatement
differs from the recorded reference values by at most 1.9e-15 relative on the LDJ and 1.2e-15 relative on the deviation figure
("RMSE").  Other numpy / scipy builds get 100 times that.  A difference of the LDJ above 1e-9 would mean the restatement is wrong."""
import ctypes as C
import json
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from magics_amd import hostlib
from magics_amd import track_metrics as tm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LDJ_MEASURED, DEV_MEASURED = 1.9e-15, 1.2e-15
LDJ_TOL, DEV_TOL = 100 * LDJ_MEASURED, 100 * DEV_MEASURED
LENGTHS = [3, 4, 5, 6, 7, 8, 9, 10, 50, 51]
CALLS = ["mgx_track_metrics_enable", "mgx_track_metrics_set_route", "mgx_tracks_set_logging", "mgx_track_metrics_read"]
FIELDS = ["n_positions", "n_velocities", "n_unrouted", "flags", "dimensionless_jerk", "vmax2", "deviation_sum", "deviation_max"]
OFFSETS = [0, 4, 8, 12, 16, 24, 32, 40]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def series(n, seed):
    """[n, 2] velocities as the trackers make them: f32 values, here a random walk"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-2.0, 2.0, 2) + np.cumsum(rng.normal(0.0, 0.4, (n, 2)), axis=0)).astype(np.float32).astype(np.float64)


def positions(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-12.0, 12.0, (n, 2)).astype(np.float32).astype(np.float64)


ROUTES = {
    "plain": [[-10.0, -3.0], [-2.5, 1.0], [4.0, 0.5], [11.0, 6.0]],
    "vertical": [[-10.0, -3.0], [-10.0, 5.0], [3.0, 5.5]],
    "zero-length": [[-4.0, 2.0], [-4.0, 2.0], [6.0, -1.0], [6.0, -1.0]],
    "only zero-length": [[1.0, 1.0], [1.0, 1.0]],
    "one point": [[1.0, 1.0]],
    "none": None,
}


# ---- 1. the batch restatement against the reference's values --------------------------------------------------------------------
def test_batch_form_against_the_reference_fixture():
    with open(os.path.join(HERE, "golden", "track_metrics.json"), encoding="utf-8") as f:
        doc = json.load(f)
    assert len(doc["cases"]) >= 30 and {c["n"] % 2 for c in doc["cases"]} == {0, 1} and min(c["n"] for c in doc["cases"]) == 3
    worst_ldj = worst_dev = 0.0
    for c in doc["cases"]:
        v = np.array(c["velocities_f32"], np.float32).astype(np.float64).reshape(-1, 2)
        p = np.array(c["positions_f32"], np.float32).astype(np.float64).reshape(-1, 2)
        route = np.array(c["route"]).reshape(-1, 2)
        assert len(v) == c["n"] and math.isfinite(c["ldj"]) and -25.0 < c["ldj"] < 0.0   # (the range the reference plots)
        d = tm.deviations(p, route)
        worst_ldj = max(worst_ldj, abs(tm.ldj(tm.dimensionless_jerk(v)) - c["ldj"]) / abs(c["ldj"]))
        worst_dev = max(worst_dev, abs(tm.path_deviation(float(d.sum()), len(d)) - c["rmse"]) / c["rmse"])
    print(f"batch form against the fixture: LDJ {worst_ldj:.3g} relative, deviation figure {worst_dev:.3g} relative")
    assert worst_ldj <= LDJ_TOL < 1e-9 and worst_dev <= DEV_TOL


# ---- 2. the streaming form against the batch form ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_streaming_form_against_batch_form(n):
    for seed in range(5):
        v, p, route = series(n, 10 * n + seed), positions(n + 1, seed), ROUTES["plain"]
        rec = tm.stream(v, p, route)
        want = tm.ldj(tm.dimensionless_jerk(v))
        assert rec["flags"] == tm.JERK_VALID | tm.DEVIATION_VALID and rec["n_velocities"] == n and rec["n_positions"] == n + 1
        assert abs(tm.ldj(rec["dimensionless_jerk"]) - want) <= LDJ_TOL * abs(want), (n, seed)
        assert rec["vmax2"] == float((v ** 2).sum(axis=1).max())
        d = tm.deviations(p, route)
        assert abs(rec["deviation_sum"] - d.sum()) <= DEV_TOL * d.sum() and abs(rec["deviation_max"] - d.max()) <= DEV_TOL * d.max()
        assert abs(tm.robot_metrics(rec)["path_deviation"] - math.sqrt(d.sum() / len(d))) <= DEV_TOL * math.sqrt(d.sum() / len(d))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_short_series_have_no_jerk(n):
    rec = tm.stream(series(n, n))
    assert rec["flags"] == 0 and math.isnan(rec["dimensionless_jerk"]) and rec["n_velocities"] == n
    assert math.isnan(tm.dimensionless_jerk(series(n, n))) and math.isnan(tm.ldj(rec["dimensionless_jerk"]))


def test_a_series_that_never_moves_has_no_jerk():
    rec = tm.stream(np.zeros((9, 2)), positions(3, 1), ROUTES["plain"])
    assert rec["flags"] == tm.DEVIATION_VALID and math.isnan(rec["dimensionless_jerk"]) and rec["vmax2"] == 0.0
    assert math.isnan(tm.dimensionless_jerk(np.zeros((9, 2))))


def test_reading_in_the_middle_changes_nothing():
    v, p = series(51, 7), positions(51, 8)
    a, b = tm.Stream(), tm.Stream()
    for i in range(51):
        for s in (a, b):
            s.velocity(*v[i])
            s.position(*p[i], ROUTES["plain"])
        mid = a.read()
        assert mid["n_velocities"] == i + 1
    assert {k: bits(x) for k, x in a.read().items()} == {k: bits(x) for k, x in b.read().items()}
    assert all(getattr(a, k) == getattr(b, k) for k in tm.Stream.__slots__)


def test_routes_with_vertical_and_zero_length_segments():
    p = positions(20, 4)
    for name in ("vertical", "zero-length"):
        rec, d = tm.stream((), p, ROUTES[name]), tm.deviations(p, ROUTES[name])
        assert rec["n_positions"] == 20 and rec["n_unrouted"] == 0 and math.isfinite(rec["deviation_sum"])
        assert abs(rec["deviation_sum"] - d.sum()) <= DEV_TOL * d.sum()
    assert abs(tm.stream((), [[-7.0, 0.0]], ROUTES["vertical"])["deviation_sum"] - 3.0) < 1e-15   # the vertical line x = -10
    for name in ("only zero-length", "one point", "none"):
        rec = tm.stream((), p, ROUTES[name])
        assert (rec["n_positions"], rec["n_unrouted"], rec["flags"]) == (0, 20, 0) and tm.deviations(p, ROUTES[name]) is None


def test_summary_has_the_statistics_modules_meaning():
    import statistics
    v = [-3.0, -7.5, -1.25, float("nan"), -9.0]
    s = tm.summary(v)
    clean = [x for x in v if not math.isnan(x)]
    assert s == {"robots": 4, "mean": statistics.mean(clean), "median": statistics.median(clean), "largest": -1.25, "smallest": -9.0,
                 "variance": statistics.variance(clean), "stdev": statistics.stdev(clean)}
    assert tm.summary([])["robots"] == 0 and math.isnan(tm.summary([1.0])["stdev"]) and tm.summary([1.0])["mean"] == 1.0


# ---- 3. the lane arithmetic in a host build, bit for bit ------------------------------------------------------------------------
def _harness(contract):
    src = os.path.join(HERE, "cpu_metrics", "metrics_harness.cpp")
    hdr = os.path.join(ROOT, "magics_amd", "csrc", "mgx_track_metrics.h")
    out = os.path.join(HERE, "cpu_metrics", f"libmetrics_harness_{contract}.so")
    flags = ["-O2", "-std=c++17", f"-ffp-contract={contract}"]
    if contract == "fast":  # (where the processor can fuse, let the compiler: the header has to keep it from doing so)
        try:
            with open("/proc/cpuinfo", encoding="utf-8") as f:
                if re.search(r"^flags\s*:.*\bfma\b", f.read(), flags=re.M):
                    flags.append("-mfma")
        except OSError:
            pass
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++"] + flags + ["-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.tm_velocity.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.tm_position.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_uint]
    lib.tm_read.argtypes = [C.c_void_p, C.c_void_p]
    for f in (lib.tm_velocity, lib.tm_position, lib.tm_read):
        f.restype = None
    return lib


class Native:
    """one robot's state in the host build"""

    def __init__(self, lib):
        assert lib.tm_state_size() == 152 and lib.tm_record_size() == C.sizeof(hostlib.TrackMetrics) == 48
        self.lib, self.state = lib, C.create_string_buffer(152)

    def velocity(self, u, w):
        self.lib.tm_velocity(self.state, float(u), float(w))

    def position(self, x, y, route):
        pts = np.zeros((0, 2)) if route is None else np.ascontiguousarray(route, dtype=np.float64).reshape(-1, 2)
        self.lib.tm_position(self.state, float(x), float(y), pts.ctypes.data if len(pts) else None, len(pts))

    def read(self):
        rec = hostlib.TrackMetrics()
        self.lib.tm_read(self.state, C.byref(rec))
        return {f: getattr(rec, f) for f in FIELDS}


def _same(got, want):
    assert {k: bits(v) if isinstance(v, float) else v for k, v in got.items()} == {k: bits(v) if isinstance(v, float) else v for k, v in want.items()}, (got, want)


@pytest.mark.parametrize("contract", ["off", "fast"])
def test_host_build_of_the_lane_arithmetic_equals_the_streaming_form(contract):
    lib = _harness(contract)
    order = ["plain", "vertical", "zero-length", "none", "only zero-length", "plain"]
    for n in [0, 1, 2] + LENGTHS:
        for seed in range(3):
            v, p = series(n, 100 * n + seed), positions(n + 2, seed)
            a, b = Native(lib), tm.Stream()
            _same(a.read(), b.read())
            for i in range(n + 2):
                route = ROUTES[order[(i // 3 + seed) % len(order)]]     # the route is replaced every three samples
                for s in (a, b):
                    if 1 <= i <= n:
                        s.velocity(*v[i - 1])
                    s.position(*p[i], route)
                _same(a.read(), b.read())                             # read after every sample: both parities of every length
            assert b.n_unrouted > 0 or n < 8
    a, b = Native(lib), tm.Stream()                                   # a series that never moves
    for s in (a, b):
        for _ in range(6):
            s.velocity(0.0, 0.0)
    _same(a.read(), b.read())
    assert a.read()["flags"] == 0 and math.isnan(a.read()["dimensionless_jerk"])


# ---- 4. the interface -------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_record_agree():
    header = open(os.path.join(ROOT, "include", "mgx.h"), encoding="utf-8").read()
    hpp = open(os.path.join(ROOT, "include", "mgx.hpp"), encoding="utf-8").read()
    rust = open(os.path.join(ROOT, "rust", "magics-hip", "src", "sys.rs"), encoding="utf-8").read()
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in hostlib.SYMBOLS and "pub fn " + name + "(" in rust and name + "(" in hpp, name
    m = re.search(r"typedef struct mgx_track_metrics \{(.*?)\} mgx_track_metrics;", header, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\b(" + "|".join(FIELDS) + r")\b", body) == FIELDS
    dt = hostlib.track_metrics_dtype()
    assert C.sizeof(hostlib.TrackMetrics) == dt.itemsize == 48 and "48 bytes" in m.group(0)
    assert [dt.fields[f][1] for f in FIELDS] == OFFSETS and [getattr(hostlib.TrackMetrics, f).offset for f in FIELDS] == OFFSETS
    assert "pub struct mgx_track_metrics" in rust
    assert (hostlib.TRACK_JERK_VALID, hostlib.TRACK_DEVIATION_VALID) == (tm.JERK_VALID, tm.DEVIATION_VALID) == (1, 2)
    assert re.search(r"#define MGX_TRACK_JERK_VALID\s+1u", header) and re.search(r"#define MGX_TRACK_DEVIATION_VALID\s+2u", header)
    assert [len(hostlib.SYMBOLS[c][1]) for c in CALLS] == [3, 4, 2, 3]
    kernel = open(os.path.join(ROOT, "magics_amd", "csrc", "mgx_tracks.hip"), encoding="utf-8").read()
    assert "sizeof(mgx_track_metrics) == 48" in kernel


def test_device_metrics_need_device_trackers():
    from magics_amd import sim

    class NoWorld:
        pass
    sc = {"config": {}, "environment": {}, "formation": {"formations": []}}
    with pytest.raises(ValueError, match="device_metrics needs device_trackers"):
        sim.Simulation(sc, NoWorld(), device_missions=False, device_metrics=True)
    with pytest.raises(ValueError, match="sample_log=False needs device_metrics"):
        sim.Simulation(sc, NoWorld(), device_missions=False, sample_log=False)


def test_simulation_metrics_on_the_host_path():
    """the oracle world over the first two simulated seconds of Circle Experiment: metrics() is the restatement applied to what
    export() holds"""
    import oracle
    from magics_amd import config, sim
    with open(os.path.join(HERE, "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)["Circle Experiment"]
    s = sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"])))
    s.run(max_time=2.0)
    m, exp = s.metrics(), s.export()
    assert len(m["robots"]) == len(exp["robots"]) > 1 and m["makespan"] == exp["makespan"]
    some = 0
    for rid, r in exp["robots"].items():
        v = np.array([x["velocity"] for x in r["velocities"]], dtype=np.float64).reshape(-1, 3)[:, [0, 2]]
        route = r["mission"]["routes"][0]["waypoints"]
        rec, got = tm.stream(v, r["positions"], route), m["robots"][rid]
        want = tm.robot_metrics(rec)
        for k in ("ldj", "path_deviation", "mean_deviation", "max_deviation"):
            assert bits(got[k]) == bits(want[k]), (rid, k)
        assert bits(got["dimensionless_jerk"]) == bits(rec["dimensionless_jerk"]) and got["n_positions"] == len(r["positions"])
        assert got["n_velocities"] == len(r["velocities"]) and got["n_unrouted"] == 0
        assert got["duration"] == r["mission"]["finished_at"] - r["mission"]["started_at"]
        if len(v) >= 3:
            some += 1
            batch = tm.ldj(tm.dimensionless_jerk(v))
            assert abs(got["ldj"] - batch) <= LDJ_TOL * abs(batch)
            d = tm.deviations(r["positions"], route)
            assert abs(got["mean_deviation"] - d.mean()) <= DEV_TOL * d.mean() + 1e-300
    assert some > 1
    assert m["summary"]["ldj"] == tm.summary([x["ldj"] for x in m["robots"].values()]) and m["summary"]["ldj"]["robots"] == some
    assert 2 * m["collisions"]["robots"] == sum(r["collisions"]["robots"] for r in exp["robots"].values())   # (a pair counts for both)
