"""Head-room for robots that spawn while the world runs (mgx_world_reserve, mgx_append_stats), the host's part (no GPU): the
null-world contract of the two calls, their mirrors (C++ header, ctypes table, Rust declarations), and how many robots the
scenario front-end asks head-room for."""
import ctypes as C
import json
import os
import re

import pytest

import oracle
from magics_amd import config, hostlib, sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_null_world_contract():
    L = hostlib.lib()
    assert L.mgx_world_reserve(None, 8) == -1
    assert b"null" in L.mgx_last_error()
    assert L.mgx_world_reserve(None, 0) == -1
    assert L.mgx_append_stats(None, None, None, None) == -1
    assert b"null" in L.mgx_last_error()
    a, r, f = C.c_uint64(7), C.c_uint64(8), C.c_uint64(9)
    assert L.mgx_append_stats(None, C.byref(a), C.byref(r), C.byref(f)) == -1
    assert (a.value, r.value, f.value) == (7, 8, 9)  # (nothing written)


def test_header_and_mirrors_agree():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "mgx.h"), flags=re.S)
    assert re.search(r"int\s+mgx_world_reserve\(mgx_world \*w, uint32_t robots\);", header)
    assert re.search(r"int\s+mgx_append_stats\(mgx_world \*w, uint64_t \*appends, uint64_t \*robots_appended, uint64_t \*fallbacks\);", header)
    hpp = _read("include", "mgx.hpp")
    assert "mgx_world_reserve(w_, robots)" in hpp and "mgx_append_stats(w_, &appends, &robots, &fallbacks)" in hpp
    L = hostlib.lib()
    assert L.mgx_world_reserve.argtypes == [C.c_void_p, C.c_uint32] and L.mgx_world_reserve.restype == C.c_int
    assert L.mgx_append_stats.argtypes == [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3 and L.mgx_append_stats.restype == C.c_int
    rs = _read("rust", "magics-hip", "src", "sys.rs")
    assert "pub fn mgx_world_reserve(w: *mut mgx_world, robots: u32) -> c_int;" in rs
    assert "pub fn mgx_append_stats(w: *mut mgx_world, appends: *mut u64, robots_appended: *mut u64, fallbacks: *mut u64) -> c_int;" in rs


class _Recording(oracle.OracleWorld):
    """an oracle world that offers reserve() as the engine does, and notes what it was asked"""

    def __init__(self, params):
        super().__init__(params)
        self.asked = []

    def reserve(self, robots):
        self.asked.append(robots)


def _scenario(name):
    return json.loads(_read("tests", "golden", "scenarios.json"))[name]


@pytest.mark.parametrize("name, tweak, expected", [
    ("Circle Experiment", None, 60),                                   # 30 robots, repeated once: finite
    ("Junction Twoway", None, sim.Simulation.RESERVE_LIMIT),             # twelve formations that repeat forever within 10000 s
    ("Junction Twoway", lambda sc: sc["config"]["simulation"].update({"max-time": 13.0}), 4 * 3 + 4 * 2 + 4 * 2),
])
def test_simulation_reserves_what_the_formations_spawn(name, tweak, expected):
    sc = _scenario(name)
    if tweak:
        tweak(sc)
    w = _Recording(config.world_params(sc["config"]))
    s = sim.Simulation(sc, w)
    assert w.asked == [expected]
    assert s._robots_expected() == expected
    # a world without reserve() — the oracle, the test oracles — is left alone
    sim.Simulation(sc, oracle.OracleWorld(config.world_params(sc["config"])))
