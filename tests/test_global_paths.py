"""Global paths, the host's part (no GPU): what the path-finding completion handler derives from a path
(magics_amd.driver.global_path_plan, robot.rs:652-667, 690-763), the argument checks of mgx_apply_global_paths that need no
device, and the host driver's chain — robots that wait for a path (MissionState::Idle) and then follow it — on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from magics_amd import hostlib, scenarios as S
from magics_amd.driver import Driver, global_path_plan
from global_paths_common import mission_kwargs, mission_scenario, replanned_path

F32 = np.float32


def test_plan_of_an_axis_aligned_path_is_exact():
    wps, means = global_path_plan([(0, 0), (8, 0), (16, 0)], 4.0, 5.0, 10)
    assert wps.dtype == np.float32 and wps.shape == (3, 4) and means.dtype == np.float64 and means.shape == (10, 4)
    assert np.array_equal(wps, np.array([(0, 0, -4, 0), (8, 0, -4, 0), (16, 0, 0, 0)], dtype=F32))
    next_x = F32(8) * F32(0.9)  # 0.9 |dir| = 7.2 < speed * horizon = 20
    for i in range(10):
        assert np.array_equal(means[i], np.array([float(next_x * (F32(i) / F32(10))), 0.0, 4.0, 0.0])), i


def test_plan_of_a_bent_path():
    """the velocity points BACK along the path (from - to), and `dir` is a Vec4: the velocity difference of the first two
    waypoints is part of its length and of its normalisation"""
    p = np.array([(1.0, 2.0), (4.0, 6.0), (4.0, 12.0)], dtype=F32)
    speed, horizon, K = F32(2.0), F32(1.5), 6
    wps, means = global_path_plan(p, speed, horizon, K)
    d0 = p[0] - p[1]
    d0 = d0 * (F32(1) / np.sqrt(F32(d0[0] * d0[0] + d0[1] * d0[1])))
    d1 = p[1] - p[2]
    d1 = d1 * (F32(1) / np.sqrt(F32(d1[0] * d1[0] + d1[1] * d1[1])))
    expect = np.array([(p[0, 0], p[0, 1], speed * d0[0], speed * d0[1]), (p[1, 0], p[1, 1], speed * d1[0], speed * d1[1]),
                       (p[2, 0], p[2, 1], 0, 0)], dtype=F32)
    assert np.array_equal(wps, expect)
    assert wps[0, 2] < 0 and wps[0, 3] < 0 and wps[1, 2] == 0 and wps[1, 3] < 0  # backwards
    dirv = expect[1] - expect[0]
    assert dirv[2] != 0 and dirv[3] != 0  # the velocities differ: the Vec4 is longer than the step between the points
    length = np.sqrt(F32(F32(F32(dirv[0] * dirv[0] + dirv[1] * dirv[1]) + dirv[2] * dirv[2]) + dirv[3] * dirv[3]))
    assert length > np.sqrt(F32(25.0))
    dn = dirv * (F32(1) / length)
    reach, most = F32(speed * horizon), F32(length * F32(0.9))
    s = reach if reach < most else most
    assert s == reach  # 3 m < 0.9 |dir|
    nxt = expect[0] + s * dn
    for i in range(K):
        r = F32(i) / F32(K)
        pos = expect[0, :2] + (nxt[:2] - expect[0, :2]) * r
        assert np.array_equal(means[i], np.array([pos[0], pos[1], speed * dn[0], speed * dn[1]], dtype=np.float64)), i
    with pytest.raises(ValueError):
        global_path_plan(p[:1], speed, horizon, K)


def test_refusals_on_a_null_world():
    L = hostlib.lib()
    robots, ptr = np.array([0], np.int32), np.array([0, 2], np.uint32)
    xy, means = np.zeros((2, 2), np.float32), np.zeros((1, 10, 4))
    a = (robots.ctypes.data, ptr.ctypes.data, xy.ctypes.data, means.ctypes.data)
    assert L.mgx_apply_global_paths(None, 1, *a, 1e30, float("inf"), 1) == -1
    assert L.mgx_apply_global_paths(None, 1, None, None, None, None, 1e30, float("inf"), 7) == -1
    assert L.mgx_apply_global_paths(None, 0, *a, 1e30, float("inf"), 0) == -1
    assert L.mgx_layout_stats(None, None, None) == -1
    assert b"null" in L.mgx_last_error()
    assert (hostlib.GLOBAL_PATH_RESET_TRACKING, hostlib.GLOBAL_PATH_ROUTE, hostlib.GLOBAL_PATH_ACTIVATE) == (1, 2, 4)
    nl = C.c_uint64(7)
    assert L.mgx_layout_stats(None, C.byref(nl), None) == -1 and nl.value == 7  # (nothing written)


def test_host_driver_waits_for_a_path_and_follows_it_on_the_oracle():
    from oracle_ext import ExtOracleWorld
    sc, n, K = mission_scenario()
    ref = ExtOracleWorld(sc["params"])
    S.populate(ref, sc)
    idle = (1, 4)
    d = Driver(ref, n, K, **mission_kwargs(sc, idle))
    spawn = d.translation.copy()
    sent = [ref.message_counts(r) for r in idle]
    for tick in range(60):
        if tick == 5:
            for r in idle:
                assert np.array_equal(d.translation[r], spawn[r]) and d.way[r] == [tuple(sc["robots"][r]["goal"])]
                assert ref.message_counts(r)[0] == sent[idle.index(r)][0]  # an idle robot's own graph has sent nothing
                d.global_path(r, replanned_path(sc["robots"][r]), 5.0)
                assert len(d.way[r]) == 2 and not d.idle[r]
        d.tick()
        if tick < 5:
            assert not np.array_equal(d.translation[0], spawn[0])
    assert not np.isnan(ref.read_beliefs()[2]).any()
    assert all(d.finished_at[r] > 5 for r in idle), d.finished_at
