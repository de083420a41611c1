"""The export of a scenario run with the trackers on the device (Simulation(device_trackers=True), the default on the engine)
against the same run with the host trackers: `positions` and `velocities` of every robot equal exactly, tick by tick and with
the default chunking, across robots that spawn while others drive; and the distance travelled — which only the device sums on
that path — against a run with the missions on the host."""
import json
import os

import pytest

import oracle
from magics_amd import World, config, sim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDS = 2.5  # Junction Twoway: waves of robots at 0 s and 2 s


def _scenario(name):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


def _run(device_trackers, chunk):
    sc = _scenario("Junction Twoway")
    s = sim.Simulation(sc, World(config.world_params(sc["config"])), device_trackers=device_trackers)
    assert s.dev and s._dev_coll and s._dev_trk == device_trackers
    return s.run(max_time=SECONDS, chunk=chunk)


_HOST = {}


def _host_trackers():
    """the checker, run once: the engine with the trackers on the host, tick by tick"""
    if not _HOST:
        s = _run(False, 1)
        _HOST["export"], _HOST["ticks"] = s.export(), s.tick_no
    return _HOST


@pytest.mark.parametrize("chunk", [1, 256], ids=["tick_by_tick", "chunked"])
def test_export_equals_the_host_trackers(chunk):
    want = _host_trackers()
    s = _run(True, chunk)
    assert s.tick_no == want["ticks"] >= 24
    assert all(r["travelled"] > 0 for r in s.robots)            # (brought up to date by run())
    got = s.export()
    assert len(got["robots"]) == len(want["export"]["robots"]) > 4  # the second wave has joined
    n_pos = n_vel = 0
    for rid, r in got["robots"].items():
        ref = want["export"]["robots"][rid]
        assert r["positions"] == ref["positions"] and r["velocities"] == ref["velocities"], rid
        n_pos, n_vel = n_pos + len(r["positions"]), n_vel + len(r["velocities"])
    assert n_pos > 50 and n_vel > 40
    assert json.dumps(got, sort_keys=True) == json.dumps(want["export"], sort_keys=True)
    if chunk == 1:  # no Transform came to the host, and nobody asked for one
        assert s._pending_track is None and not s._host_needs_transforms()


def test_distance_agrees_with_the_host_missions():
    """the host path sums np.hypot terms in `travelled`, the device sqrt(x*x + y*y) terms: both within about an ulp of the same
    positive terms, so sums of n <= 10^5 of them differ by at most about (n + 2) * 2^-52 ~ 2e-11 relative; 1e-9 leaves a margin"""
    sc = _scenario("Junction Twoway")
    dev = _run(True, 256)
    ref = sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"]))).run(max_time=SECONDS)
    assert not ref.dev and ref.tick_no == dev.tick_no and len(ref.robots) == len(dev.robots)
    for a, b in zip(dev.robots, ref.robots):
        assert a["travelled"] > 0 and abs(a["travelled"] - b["travelled"]) <= 1e-9 * b["travelled"], (a["id"], a["travelled"], b["travelled"])
