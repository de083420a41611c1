"""The safety distance and the tracking paths changed at run time, on the device: mgx_set_safety_multiplier
(update_inter_robot_safety_distance_multiplier, factorgraph.rs:892-910, ui/settings.rs:586-590) and mgx_set_tracking_path
(modify_tracking_factors + set_tracking_path, factorgraph.rs:1467, tracking.rs:134-136, robot.rs:674-682) against the CPU
oracle extended with the same two mutators (tests/oracle_ext.py) — bit for bit after every step."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S, sharded
from magics_amd.hostlib import MgxError
from oracle_ext import ExtOracleWorld, make_pair
from parity import assert_identical

pytestmark = pytest.mark.gpu

SEGMENTS, RESIDENT, POSTED = 0, 1, 2  # MGX_SWEEP_FORM_*
# the script of most tests: ticks under the scenario's 2.2, then 4.0, then 1.0
SCRIPT = [(None, 3), (4.0, 3), (1.0, 2)]


def _horizon_for(K):
    """a look-ahead horizon whose variable timesteps (lookahead multiple 3) number K"""
    for h in range(1, 1000):
        n = len(hostlib.variable_timesteps(h, 3))
        if n == K:
            return h
        if n > K:
            break
    raise ValueError(f"no horizon gives K = {K}")


def _circle(n, K=10, radius=6.0, connect=None):
    """n robots on a small circle heading for the antipode — their variables cross in the middle, so inter-robot factors are
    live under every multiplier of the script and more of them under the larger ones (radii 2 .. 3: safety distances 2 .. 12) —
    everyone connected with everyone (or the ordered pairs in `connect`); dynamics + obstacle (white image) + inter-robot"""
    added = K not in S.HORIZON_FOR_K
    if added:
        S.HORIZON_FOR_K[K] = _horizon_for(K)
    try:
        sc = S.circle_scenario(n_robots=n, K=K, circle_radius=radius, n_internal=10, n_external=5)
    finally:
        if added:
            del S.HORIZON_FOR_K[K]
    pairs = connect if connect is not None else [(a, b) for a in range(n) for b in range(n) if a != b]
    sc["ir"] = S.number_ir_pairs(pairs, K)
    return sc


def _run_script(w, sc, script=SCRIPT):
    tick = S.tick_inputs(sc)
    for m, n_ticks in script:
        if m is not None:
            w.set_safety_multiplier(m)
        for _ in range(n_ticks):
            w.tick(steps=sc["steps"], **tick)


def _both_script(eng, ref, sc, what, script=SCRIPT, after_tick=None):
    tick = S.tick_inputs(sc)
    t = 0
    for m, n_ticks in script:
        for w in (eng, ref):
            if m is not None:
                w.set_safety_multiplier(m)
        for _ in range(n_ticks):
            for w in (eng, ref):
                w.tick(steps=sc["steps"], **tick)
            if after_tick:
                after_tick(m)
            assert_identical(eng, ref, what=f"{what}, tick {t} (multiplier {m if m is not None else 'as created'})")
            t += 1


# ---- 1. the multiplier, resident and launch by launch ------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "segments"])
def test_multiplier_script(resident):
    sc = _circle(6)
    eng, ref = make_pair(sc)
    if not resident:
        eng.set_resident_launches(False)
    forms = []

    def after_tick(m):
        forms.append(eng.last_sweep()[2])
        assert forms[-1] in ((RESIDENT, POSTED) if resident else (SEGMENTS,)), (m, forms)
    _both_script(eng, ref, sc, "multiplier script", after_tick=after_tick)
    assert len(forms) == 8 and np.isfinite(eng.read_beliefs()[2]).all()
    # guard: the same script without the calls ends elsewhere — the comparison above is not vacuous
    plain = ExtOracleWorld(sc["params"])
    S.populate(plain, sc)
    _run_script(plain, sc, script=[(None, 8)])
    assert not np.array_equal(plain.read_beliefs()[2], ref.read_beliefs()[2])


def test_multiplier_is_checked_and_a_refused_call_changes_nothing():
    sc = _circle(4)
    eng, ref = make_pair(sc)
    _both_script(eng, ref, sc, "before the refused calls", script=[(None, 1)])
    for bad in (0.0, -4.0, float("inf"), float("nan")):
        with pytest.raises(MgxError, match="finite and > 0"):
            eng.set_safety_multiplier(bad)
    _both_script(eng, ref, sc, "after the refused calls", script=[(None, 2)])


# ---- 2. the multiplier survives what rebuilds records ------------------------------------------------------------------------
def test_multiplier_survives_topology_passes_and_relayouts():
    n, K = 6, 10
    sc = _circle(n, K, connect=[(a, b) for a in range(n) for b in range(n) if a != b and abs(a - b) in (1, n - 1)])  # the ring
    eng, ref = make_pair(sc)
    tick = S.tick_inputs(sc)
    nxt = 1 + (K - 1) * len(sc["ir"])

    def ticks(what, k=2, inputs=tick):
        for t in range(k):
            for w in (eng, ref):
                w.tick(steps=sc["steps"], **inputs)
            assert_identical(eng, ref, what=f"{what}, tick {t}")
    ticks("ring", 1)
    for w in (eng, ref):
        w.set_safety_multiplier(4.0)
    # a topology pass that creates and deletes: robot 0 out of everybody's range, the others within range of each other
    pos = np.zeros((n, 3), dtype=np.float32)
    pos[:, 0], pos[:, 2] = sc["positions"][:, 0], sc["positions"][:, 1]
    pos[0, 0] += 1000.0
    outs = [w.update_topology(pos, 13.0, nxt) for w in (eng, ref)]
    assert outs[0] == outs[1] and outs[0][1] > 0 and outs[0][2] > 0, outs
    nxt = outs[0][0]
    ticks("after a pass that created and deleted connections")
    # a robot joins (the world is laid out again), with a radius of its own, and is connected
    ts = S.timesteps_for_K(K)
    mean0, prior, dt = S.robot_initial_state((0.5, -0.5, 3.0, 3.0), (9.0, 8.0, 3.0, 3.0), ts, 1.5, sc["target_speed"], 3.0)
    ids = [w.add_robot(mean0, prior, dt, 1.5, order_key=n) for w in (eng, ref)]
    assert ids == [n, n]
    for w in (eng, ref):
        w.ir_connect(n, 1, nxt)
        w.ir_connect(1, n, nxt + K - 1)
    nxt += 2 * (K - 1)
    ticks("after add_robot")  # (the joiner's priors stay: it has no waypoint here)
    for w in (eng, ref):
        w.set_safety_multiplier(1.5)  # (and once more on the re-laid world, the joiner's edges included)
    ticks("second multiplier after add_robot")
    for w in (eng, ref):
        w.remove_robot(2)
    pos = np.vstack([pos, np.array([[0.5, 0.0, -0.5]], dtype=np.float32)])
    outs = [w.update_topology(pos, 13.0, nxt) for w in (eng, ref)]
    assert outs[0] == outs[1], outs
    live = np.array([r for r in range(n) if r != 2], dtype=np.int32)
    ticks("after remove_robot", inputs=dict(tick, robots=live, waypoints_xy=tick["waypoints_xy"][live], time_scale=tick["time_scale"][live],
                                            what=tick["what"][live]))


def test_multiplier_reaches_the_slot_records_kept_on_the_device():
    """The call between two topology passes of which the second changes only some robots' lists: the others lay their edges
    out again from the slot records the device kept since the first pass — the ones the call rewrote in place.
    Ring of six (neighbours 6 m apart, search radius 7): the first pass closes the ring, the second takes robot 0 out of range,
    so robots 1 and 5 send new lists and robots 2, 3, 4 do not."""
    n, K = 6, 10
    ring = [(a, b) for a in range(n) for b in range(n) if a != b and abs(a - b) in (1, n - 1)]
    sc = _circle(n, K, connect=[p for p in ring if set(p) != {2, 3}])
    eng, ref = make_pair(sc)
    plain = ExtOracleWorld(sc["params"])  # the same script without the call
    S.populate(plain, sc)
    worlds = (eng, ref, plain)
    tick = S.tick_inputs(sc)

    def ticks(what, k):
        for t in range(k):
            for w in worlds:
                w.tick(steps=sc["steps"], **tick)
            assert_identical(eng, ref, what=f"{what}, tick {t}")
    pos = np.zeros((n, 3), dtype=np.float32)
    pos[:, 0], pos[:, 2] = sc["positions"][:, 0], sc["positions"][:, 1]
    nxt = 1 + (K - 1) * len(sc["ir"])
    ticks("open ring", 1)
    outs = [w.update_topology(pos, 7.0, nxt) for w in worlds]
    assert outs[0] == outs[1] == outs[2] and outs[0][1:] == (2, 0), outs  # 2 <-> 3 created
    nxt = outs[0][0]
    ticks("ring closed by a pass", 1)  # (the tables are laid out by the pass's differences: slot records on the device from here on)
    for w in (eng, ref):
        w.set_safety_multiplier(4.0)
    pos[0, 0] += 1000.0
    outs = [w.update_topology(pos, 7.0, nxt) for w in worlds]
    assert outs[0] == outs[1] == outs[2] and outs[0][1] == 0 and outs[0][2] > 0, outs  # robot 0's pairs deleted, nothing created
    assert [eng.connections(r) for r in range(n)] == [ref.connections(r) for r in range(n)]
    assert sorted(ref.connections(3)) == [2, 4] and sorted(ref.connections(2)) == [1, 3] and sorted(ref.connections(4)) == [3, 5]
    ticks("after the second pass", 3)
    # guard: robot 3 hears only 2 and 4, whose lists and its own did not change — without the new distance it ends elsewhere
    mu, mu_plain = ref.read_beliefs()[2].reshape(n, K, 4), plain.read_beliefs()[2].reshape(n, K, 4)
    assert not np.array_equal(mu[3], mu_plain[3])


# ---- 3. the multiplier while inter-robot factors are off ---------------------------------------------------------------------
@pytest.mark.parametrize("keyless", [False, True], ids=["thaw", "keyless"])
def test_multiplier_while_interrobot_factors_are_off(keyless):
    n, K = 6, 10
    sc = _circle(n, K)
    late = [c for c in sc["ir"] if 0 in c[:2]] if keyless else []  # (robot 0's connections: made while the kind is off)
    sc["ir"] = [c for c in sc["ir"] if c not in late]
    eng, ref = make_pair(sc)
    mask = sc["params"]["enable_mask"]
    tick = S.tick_inputs(sc)

    def ticks(what, k):
        for t in range(k):
            for w in (eng, ref):
                w.tick(steps=sc["steps"], **tick)
            assert_identical(eng, ref, what=f"{what}, tick {t}")
    ticks("kind on", 2)
    for w in (eng, ref):
        w.set_enabled(mask & ~S.EN_IR)
        for a, b, n0 in late:
            w.ir_connect(a, b, n0)
        w.set_safety_multiplier(4.0)
    ticks("kind off, multiplier set", 1)
    for w in (eng, ref):
        w.set_enabled(mask)
    ticks("kind on again", 2)


# ---- 4. the multiplier inside an open batch ----------------------------------------------------------------------------------
def test_multiplier_inside_an_open_batch():
    sc = _circle(6)
    eng, ref = make_pair(sc)
    steps = sc["steps"]
    eng.batch_begin()
    eng.iterate(steps)
    eng.set_safety_multiplier(4.0)  # (submits what was recorded: the first schedule runs under 2.2)
    eng.iterate(steps)
    assert eng.batch_end()[0] == 2
    ref.iterate(steps)
    ref.set_safety_multiplier(4.0)
    ref.iterate(steps)
    assert_identical(eng, ref, what="iterate; set; iterate inside one batch")


# ---- 5. run-time-K and long horizons -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [14, 35])
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "segments"])
def test_multiplier_script_other_horizons(K, resident):
    sc = _circle(4, K)
    assert sc["K"] == K
    eng, ref = make_pair(sc)
    if not resident:
        eng.set_resident_launches(False)
    _both_script(eng, ref, sc, f"K = {K}")
    assert eng.last_sweep()[0] == (35 if K == 35 else 0)  # the constant-K template / the run-time-K kernel


# ---- 6. and 7. tracking paths ------------------------------------------------------------------------------------------------
def _lanes(K, n=4, extra_without_path=True):
    """n robots on parallel lanes along +x, 10 m apart, tracking factors and no inter-robot ones; each follows a 3-point path
    whose corner lies half a metre beyond its variable K-2 — that variable's factor comes within the switch padding (1 m) of
    the first segment's end and its record advances to 1 (tracking.rs:294-296), the others' stay 0.  One more robot has no
    path at all."""
    ts = S.timesteps_for_K(K)
    speed = 5.0
    robots, corners = [], []
    for r in range(n + (1 if extra_without_path else 0)):
        y = 10.0 * r
        mean0, prior, dt = S.robot_initial_state((0.0, y, speed, 0.0), (1000.0, y, speed, 0.0), ts, 1.0, speed, S.HORIZON_FOR_K[K] / speed)
        corner = float(mean0[K - 2, 0]) + 0.5
        assert corner - float(mean0[K - 3, 0]) > 2.0
        path = np.array([(0.0, y), (corner, y), (corner, y + 20.0)], dtype=np.float32) if r < n else None
        robots.append(dict(mean0=mean0, prior_diag=prior, dt=dt, radius=1.0, path=path, order_key=r))
        corners.append(corner)
    params = dict(S.JUNCTION_PARAMS, enable_mask=S.EN_DYN | S.EN_OBS | S.EN_TRK)
    sdf = dict(rgb=np.full((16, 16, 3), 255, dtype=np.uint8), world_w=4000.0, world_h=4000.0)
    return dict(params=params, sdf=sdf, robots=robots, ir=[], steps=[1] * 6, K=K), corners


def _tracking_present(ref, robot, K):
    """per variable 1 .. K-2 of the oracle's graph: is the message of its tracking factor a message (not the empty one)?"""
    first = K + (K - 1) + (K - 2)
    out = []
    for i in range(1, K - 1):
        mine = [b for b in ref.variable_inbox(robot, i) if b[0] == robot and b[1] == first + i - 1]
        assert len(mine) == 1
        out.append(mine[0][2])
    return out


@pytest.mark.parametrize("K", [10, 35])  # (35: the tracking state lives in HBM inside the sweeps)
def test_tracking_paths_replaced(K):
    sc, corners = _lanes(K)
    eng, ref = make_pair(sc)

    def ticks(what, k):
        for t in range(k):
            for w in (eng, ref):
                w.iterate(sc["steps"])
            assert_identical(eng, ref, what=f"{what}, tick {t}")
    ticks("three-point paths", 3)  # (18 factor iterations: the tracking factors have been running for eight)
    assert all(_tracking_present(ref, 1, K)) and not any(_tracking_present(ref, 4, K))
    c0, c1 = corners[0], corners[1]
    longer = np.array([(0.0, 0.0), (c0, 0.0), (c0, 20.0), (c0 + 20.0, 20.0), (c0 + 20.0, 40.0)], dtype=np.float32)
    first = np.array([(0.0, 40.0), (30.0, 40.0), (30.0, 60.0)], dtype=np.float32)
    for w in (eng, ref):
        w.set_tracking_path(0, longer)
        w.set_tracking_path(1, np.array([(0.0, 10.0), (c1, 10.0)], dtype=np.float32))
        w.set_tracking_path(4, first)
    ticks("paths replaced", 3)
    # from the oracle: robot 1's factor on variable K-2 had advanced to record 1 and is silent under the two-point path, its
    # other factors go on; the robot that had no path is tracking
    assert _tracking_present(ref, 1, K) == [True] * (K - 3) + [False]
    assert all(_tracking_present(ref, 0, K)) and all(_tracking_present(ref, 4, K))
    # guard: without the calls the world ends elsewhere
    plain = ExtOracleWorld(sc["params"])
    S.populate(plain, sc)
    for _ in range(6):
        plain.iterate(sc["steps"])
    mu, mu_plain = ref.read_beliefs()[2].reshape(5, K, 4), plain.read_beliefs()[2].reshape(5, K, 4)
    assert not np.array_equal(mu[1], mu_plain[1]) and not np.array_equal(mu[4], mu_plain[4])
    assert np.array_equal(mu[2], mu_plain[2]) and np.array_equal(mu[3], mu_plain[3])  # (nothing else changed)


def test_tracking_path_arguments():
    sc, _ = _lanes(10, n=2, extra_without_path=False)
    eng, ref = make_pair(sc)
    rb = sc["robots"][0]
    ghost = eng.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], 1.0, order_key=7, ghost=True)  # (another rank's: the engine only)
    p = np.zeros((3, 2), np.float32)
    for w in (eng, ref):
        w.iterate([1] * 12)
    for robot, path, match in ((0, p[:1], "n_path"), (5, p, "bad robot"), (-1, p, "bad robot"), (ghost, p, "not a live local robot")):
        with pytest.raises(MgxError, match=match):
            eng.set_tracking_path(robot, path)
    for w in (eng, ref):
        w.iterate([1] * 3)
    assert_identical(eng, ref, what="after the refused calls")


def test_completion_handler_sequence():
    """robot.rs:674-769 on one robot of four: set_tracking_path, reset_variables(means, 1e30, inf), reset_tracking_factors —
    then twelve iterations: the ten skipped tracking updates and two live ones, the other three robots iterating throughout"""
    K = 10
    sc, corners = _lanes(K, extra_without_path=False)
    eng, ref = make_pair(sc)
    for t in range(3):
        for w in (eng, ref):
            w.iterate(sc["steps"])
        assert_identical(eng, ref, what=f"before the handler, tick {t}")
    y = 20.0
    path = np.array([(2.0, y + 1.0), (12.0, y + 3.0), (24.0, y + 3.0), (24.0, y + 30.0)], dtype=np.float32)
    means = sc["robots"][2]["mean0"].copy()
    means[:, 0] += 2.0
    means[:, 1] += 1.0 + 0.1 * np.arange(K)
    for w in (eng, ref):
        w.set_tracking_path(2, path)
        w.reset_variables(2, means)  # (the reference's call: 1e30, +inf)
        w.reset_tracking_factors(2)
    assert_identical(eng, ref, what="right after the handler")
    silent = []
    for it in range(12):
        for w in (eng, ref):
            w.iterate([1])
        assert_identical(eng, ref, what=f"after the handler, iteration {it}")
        silent.append(not any(_tracking_present(ref, 2, K)))
    assert silent == [True] * 10 + [False] * 2, silent


# ---- 8. sharded, in one process ----------------------------------------------------------------------------------------------
def test_multiplier_on_a_sharded_world():
    sc = _circle(6)
    cluster = sharded.LocalCluster(sc, 2, World)
    assert [len(sw.plan.local) for sw in cluster.ranks] == [3, 3] and all(sw.plan.ghosts for sw in cluster.ranks)
    ref = ExtOracleWorld(sc["params"])
    S.populate(ref, sc)
    _both_script(cluster, ref, sc, "2 ranks x 3 robots")
