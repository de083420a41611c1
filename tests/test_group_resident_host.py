"""mgx_set_group_resident / mgx_group_resident_stats without a device: the null-argument checks, and that every layer declares
the two calls — the C header, the C++ wrapper, hostlib, World, the Rust declarations and wrapper — and that Ensemble takes
masked_resident for itself and hands it to no Simulation."""
import copy
import ctypes as C
import inspect
import json
import os
import re

from magics_amd import World, ensemble, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1   # MGX_ERR_INVALID


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_null_arguments_are_refused():
    L = hostlib.lib()
    assert L.mgx_set_group_resident(None, 1) == ERR_INVALID
    assert b"null" in L.mgx_last_error()
    a, b, c = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    assert L.mgx_group_resident_stats(None, C.byref(a), C.byref(b), C.byref(c)) == ERR_INVALID
    assert (a.value, b.value, c.value) == (7, 7, 7)                    # nothing written
    assert L.mgx_group_resident_stats(None, None, None, None) == ERR_INVALID


def test_every_layer_declares_the_calls():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "mgx.h"), flags=re.S)
    assert re.search(r"int\s+mgx_set_group_resident\(mgx_world \*w, int32_t enabled\);", header)
    assert re.search(r"int\s+mgx_group_resident_stats\(mgx_world \*w, uint64_t \*launches, uint64_t \*posts, uint64_t \*fallbacks\);", header)
    assert re.search(r"#define\s+MGX_SWEEP_F_GROUP_KINDS\s+4u", header)
    hpp = _read("include", "mgx.hpp")
    assert "mgx_set_group_resident(w_" in hpp and "mgx_group_resident_stats(w_" in hpp
    sys_rs, lib_rs = _read("rust", "magics-hip", "src", "sys.rs"), _read("rust", "magics-hip", "src", "lib.rs")
    assert "pub fn mgx_set_group_resident(w: *mut mgx_world, enabled: i32) -> c_int;" in sys_rs
    assert "pub fn mgx_group_resident_stats(w: *mut mgx_world, launches: *mut u64, posts: *mut u64, fallbacks: *mut u64) -> c_int;" in sys_rs
    assert "sys::mgx_set_group_resident(" in lib_rs and "sys::mgx_group_resident_stats(" in lib_rs
    L = hostlib.lib()
    assert L.mgx_set_group_resident.argtypes[1] is C.c_int32 and len(L.mgx_group_resident_stats.argtypes) == 4
    assert callable(World.set_group_resident) and callable(World.group_resident_stats)


def test_ensemble_keeps_the_keyword_to_itself(monkeypatch):
    assert inspect.signature(ensemble.Ensemble.__init__).parameters["masked_resident"].default is False
    seen = {}

    class Stop(Exception):
        pass

    class FakeWorld:
        """what Ensemble asks of a world before it makes its first Simulation"""
        told = []
        mission_tick_begin_groups = neighbours_groups = group_schedule_stats = staticmethod(lambda *a, **k: None)

        def set_group_resident(self, enabled):
            self.told.append(("resident", bool(enabled)))

        def set_group_enabled(self, group, mask):
            self.told.append(("mask", group, mask))

    def fake_simulation(sc, view, **options):
        seen.update(options)
        assert FakeWorld.told and FakeWorld.told[0] == ("resident", True)   # before the first robot: before any Simulation exists
        raise Stop

    monkeypatch.setattr(ensemble, "Simulation", fake_simulation)
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)["Structured Junction Twoway"]
    other = copy.deepcopy(sc)
    other["config"]["gbp"]["factors-enabled"]["tracking"] = not sc["config"]["gbp"]["factors-enabled"]["tracking"]
    try:
        ensemble.Ensemble([sc, other], FakeWorld(), masked_resident=True, sample_log=False)
    except Stop:
        pass
    assert seen == {"sample_log": False}
    assert [t for t in FakeWorld.told if t[0] == "mask"], "the members' masks follow the switch"
    assert FakeWorld.told.index(("resident", True)) < min(i for i, t in enumerate(FakeWorld.told) if t[0] == "mask")
