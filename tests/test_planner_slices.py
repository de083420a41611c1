"""Plans that ride the ticks, the parts that need no GPU: the rule for the slice a request ends in (global_planner.slices_needed,
the statement of include/mgx.h), what Simulation refuses, the six new functions in the binding with the header's arity, and the
pool's bookkeeping (magics_amd/csrc/mgx_plan_pool.h) driven through 10 000 random steps by a stand-alone program built with
AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes
import os
import re
import subprocess

import pytest

from magics_amd import hostlib, sim
from magics_amd import global_planner as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mgx_plan_submit", "mgx_plan_advance", "mgx_planner_set_tick_budget", "mgx_plan_collect", "mgx_plan_cancel", "mgx_plan_pending")


def _res(status, iterations, smoothing=0):
    return {"status": status, "iterations": iterations, "smoothing_iterations": smoothing}


def test_slices_needed_ok_and_tree_full():
    p = {"max_iterations": 1000}
    for status in (gp.PLAN_OK, gp.PLAN_TREE_FULL):
        # B divides g + s: the launch that makes the last iteration finishes too
        assert gp.slices_needed(_res(status, 50, 14), p, 64) == 1
        assert gp.slices_needed(_res(status, 100, 28), p, 64) == 2
        assert gp.slices_needed(_res(status, 64, 0), p, 64) == 1
        # B does not divide
        assert gp.slices_needed(_res(status, 64, 1), p, 64) == 2
        assert gp.slices_needed(_res(status, 63, 0), p, 64) == 1
        assert gp.slices_needed(_res(status, 1, 0), p, 7) == 1
        assert gp.slices_needed(_res(status, 700, 60), p, 7) == 109   # 760 = 108 * 7 + 4
        assert gp.slices_needed(_res(status, 700, 56), p, 7) == 108   # 756 = 108 * 7
        assert gp.slices_needed(_res(status, 5, 3), p, 1) == 8
        # nothing done at all: a request still needs the launch that says so
        assert gp.slices_needed(_res(status, 0, 0), p, 64) == 1


def test_slices_needed_max_iterations():
    r = _res(gp.PLAN_MAX_ITERATIONS, 96)
    assert gp.slices_needed(r, {"max_iterations": 96}, 7) == 96 // 7 + 1 == 14
    assert gp.slices_needed(r, {"max_iterations": 96}, 64) == 2
    assert gp.slices_needed(r, {"max_iterations": 96}, 32) == 4     # B divides: the launch after the last iteration sees the limit
    assert gp.slices_needed(r, {"max_iterations": 96}, 96) == 2
    assert gp.slices_needed(r, {"max_iterations": 96}, 97) == 1
    assert gp.slices_needed(r, {"max_iterations": 96}, 1000) == 1
    assert gp.slices_needed(_res(gp.PLAN_MAX_ITERATIONS, 0), {"max_iterations": 0}, 5) == 1


def test_slices_needed_refuses_nonsense():
    with pytest.raises(ValueError):
        gp.slices_needed(_res(gp.PLAN_OK, 5), {"max_iterations": 9}, 0)
    with pytest.raises(ValueError):
        gp.slices_needed(_res(7, 5), {"max_iterations": 9}, 3)


def test_the_restatement_counts_its_smoothing_iterations():
    """a map without colliders: the goal is met by the first sample that falls within a step of it, every chord is free, and the
    smoothing pass stops when the path is down to two points or its iterations run out"""
    p = gp.params(5.0, 8.0, 1.0, 4000, smoothing_enabled=True, smoothing_max_iterations=9, smoothing_step=5.0, sample_half_extent=40.0, max_nodes=2048)
    r = gp.plan_paths(None, [((0.0, 0.0), (30.0, 20.0), 5)], p)[0]
    assert r["status"] == gp.PLAN_OK and 1 <= r["smoothing_iterations"] <= 9
    assert len(r["path"]) == 2 or r["smoothing_iterations"] == 9
    q = gp.plan_paths(None, [((0.0, 0.0), (30.0, 20.0), 5)], dict(p, smoothing_enabled=False))[0]
    assert q["smoothing_iterations"] == 0 and q["iterations"] == r["iterations"]
    f = gp.plan_paths(None, [((0.0, 0.0), (3000.0, 20.0), 5)], dict(p, max_iterations=30))[0]
    assert f["status"] == gp.PLAN_MAX_ITERATIONS and f["smoothing_iterations"] == 0
    assert gp.slices_needed(f, dict(p, max_iterations=30), 7) == 5


def test_simulation_refuses_bad_planner_arguments():
    sc = {}
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="plan_budget"):
            sim.Simulation(sc, None, global_planner="sliced", plan_budget=bad)
    with pytest.raises(ValueError, match="plan_budget"):
        sim.Simulation(sc, None, plan_budget=0)
    for bad in ("device", "slice", False, 2):
        with pytest.raises(ValueError, match="global_planner"):
            sim.Simulation(sc, None, global_planner=bad)


def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "mgx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_the_binding_declares_the_new_functions_with_the_headers_arity():
    L = ctypes.CDLL(hostlib.LIB_PATH)
    for name in NEW:
        restype, argtypes = hostlib.SYMBOLS[name]
        assert restype is ctypes.c_int and len(argtypes) == _header_arity(name), name
        assert hasattr(L, name), name
    assert _header_arity("mgx_plan_collect") == 8 and _header_arity("mgx_plan_submit") == 4
    d = hostlib.plan_done_dtype()
    assert d.itemsize == 16 + hostlib.plan_result_dtype().itemsize == 56 and d.fields["result"][1] == 16
    assert hostlib.plan_result_dtype().fields["smoothing_iterations"][1] == 20


def test_calls_without_a_world_fail_before_the_device():
    L = hostlib.lib()
    n = ctypes.c_uint32(7)
    assert L.mgx_plan_submit(None, 0, None, None) == -1
    assert L.mgx_plan_advance(None, 5) == -1
    assert L.mgx_planner_set_tick_budget(None, 5) == -1
    assert L.mgx_plan_collect(None, 0, 0, None, None, 0, ctypes.byref(n), ctypes.byref(n)) == -1
    assert L.mgx_plan_cancel(None, 1) == -1
    assert L.mgx_plan_pending(None, ctypes.byref(n)) == -1 and n.value == 7


def test_pool_bookkeeping_under_sanitizers(tmp_path):
    """slots in blocks, the free list, ticket -> slot, the order of collect, cancel, cooling until the slices in flight have
    completed: 10 000 random steps, two seeds, over two shapes of pool (16 x 256, and one block of 5 slots as a call's pool is
    one block), as a program of its own (host code only)"""
    exe = str(tmp_path / "plan_pool_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # (a program of its own: nothing of the runtimes is looked up when it starts)
                    os.path.join(ROOT, "tests", "c_abi", "plan_pool_fuzz.cpp"), "-o", exe], check=True)
    for seed in ("12345", "99"):
        r = subprocess.run([exe, "10000", seed], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode == 0 and r.stdout.count(b"plan pool ok") == 2, r.stdout.decode()  # (one line per shape)
