"""Every instantiation of the sweep kernel against the CPU oracle, cell by cell.

mgx_sweep_inst.hip compiles k_robot_sweep for twelve horizon variants (constant-K templates and the run-time-K kernels 0 / -1)
in five code paths each: launch per segment without inter-robot factors, with staged and with unstaged (read from L2)
inter-robot messages, the resident schedule launch and the sharded resident launch.  Which one runs follows from K, the
largest number of inter-robot edges of any robot, the LDS it needs, the device's resident capacity and per-world switches.
Every cell below states the (variant, ir_mode, form) it is meant to run, asserts it through World.last_sweep() — what the
launcher that enqueued the sweeps chose — and compares the beliefs with the oracle bit for bit.  A threshold that moves a
cell onto another kernel fails the cell instead of quietly running a path twice.

A resident or sharded cell whose launch the residency census declined (another tenant held the CUs) is skipped with a
reason; launch-per-segment cells never skip."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

import oracle
from magics_amd import World, hostlib, scenarios as S, sharded
from magics_amd.hostlib import MgxError
from parity import assert_identical, assert_identical_where_finite

INST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magics_amd", "csrc", "mgx_sweep_inst.hip")

IR_NONE, IR_UNSTAGED, IR_STAGED = 0, 1, 2  # MGX_SWEEP_IR_*
SEGMENTS, RESIDENT, POSTED, SHARDED = 0, 1, 2, 3  # MGX_SWEEP_FORM_*
# what each form of a cell asks for, and the (ir_mode, form) it must report
FORMS = {"seg_none": (IR_NONE, SEGMENTS), "seg_staged": (IR_STAGED, SEGMENTS), "seg_global": (IR_UNSTAGED, SEGMENTS),
         "resident": (IR_STAGED, RESIDENT), "posted": (IR_STAGED, POSTED), "sharded": (IR_STAGED, SHARDED)}

CONST_K = (10, 11, 12, 13, 16, 17, 20, 21, 32, 35)
# the horizon that stands for each variant in the form matrix: 33 fills exactly 64 lanes with the run-time-K kernel, 34 is the
# first horizon with two dynamic messages per lane
FORM_K = {**{k: k for k in CONST_K}, 0: 33, -1: 34}

INT_FIRST = [1, 3, 1, 3]  # segments: [int] [ext int int] [ext int]
EXT_FIRST = [2, 3, 3, 1, 3]


def _seg_lds(K, ir_edges):
    """sweep_lds_bytes(K, ir_edges) of mgx_kernels.hip (launch per segment): used here only to SIZE the crowded clusters — which
    mode ran is read back from the engine"""
    E1 = 4 * K - 5
    inout = 16 * K + 4 * K + 20 * E1 + K
    io = inout + (inout & 1)
    return 8 * ((24 + 40) * K + io + 7 * (ir_edges + 1)) + 4 * (2 * ((K + 1) & ~1) + ((3 * (K + 1) + 1) & ~1))


def _crowd(K, limit=64 * 1024):
    """robots of a cluster in which everyone hears everyone and a robot's staged messages need more than `limit` bytes"""
    n = 2
    while _seg_lds(K, (n - 1) * (K - 1)) <= limit:
        n += 1
    return n


def _horizon_for(K):
    """a look-ahead horizon whose variable timesteps (lookahead multiple 3) number K"""
    for h in range(1, 1000):
        n = len(hostlib.variable_timesteps(h, 3))
        if n == K:
            return h
        if n > K:
            break
    raise ValueError(f"no horizon gives K = {K}")


def _grid(n, K, **kw):
    if K in S.HORIZON_FOR_K:
        return S.grid_scenario(n, K, **kw)
    S.HORIZON_FOR_K[K] = _horizon_for(K)
    try:
        return S.grid_scenario(n, K, **kw)
    finally:
        del S.HORIZON_FOR_K[K]


def _scenario(layout, K, n, tracking=False):
    if layout == "none":  # no inter-robot factors
        return _grid(n, K, interrobot=False, pitch=2.5, tracking=tracking)
    if layout == "grid":  # up to eight neighbours
        return _grid(n, K, interrobot=True, pitch=2.5, comm_radius=4.5, tracking=tracking)
    if layout == "line":  # one row: two neighbours
        return _grid(n, K, interrobot=True, pitch=2.5, comm_radius=3.5, grid_side=n, tracking=tracking)
    if layout == "dense":  # everyone within range of everyone
        return _grid(n, K, interrobot=True, pitch=1.2, comm_radius=1000.0, obstacles=False, tracking=tracking)
    if layout == "border":  # a non-square image (160 x 96 px over 40 x 24 m); the robots' horizons run across its border
        sc = _grid(n, K, interrobot=True, pitch=2.5, comm_radius=4.5, origin=(14.0, 7.0), tracking=tracking)
        rgb = S.synthetic_sdf(S.SplitMix64(97), 40.0, 24.0, px_per_m=4, disc_area_frac=0.08)
        assert rgb.shape == (96, 160, 3)
        return dict(sc, sdf=dict(rgb=rgb, world_w=40.0, world_h=24.0))
    raise ValueError(layout)


Cell = namedtuple("Cell", "name K variant form layout n script tracking")


def _cell(K, variant, form, layout, n, script, tracking=False, tag=""):
    return Cell(f"K{K}-{form}-{layout}-{script}{tag}", K, variant, form, layout, n, script, tracking)


def _table():
    cells = []
    scripts = ("tick", "int_first", "ext_first", "prior", "reconnect")
    for i, (variant, K) in enumerate(FORM_K.items()):
        layout = "line" if K >= 45 else "grid"
        rot = lambda j, pool=scripts: pool[(i + j) % len(pool)]
        cells += [
            _cell(K, variant, "seg_none", "none", 9, rot(0, scripts[:4])),
            _cell(K, variant, "seg_staged", layout, 12, rot(1)),
            _cell(K, variant, "seg_global", "dense", _crowd(K), rot(2)),
            _cell(K, variant, "resident", layout, 12, rot(3)),
            _cell(K, variant, "posted", layout, 12, "tick" if i % 2 == 0 else "int_first"),
            _cell(K, variant, "sharded", layout, 16, rot(4, ("int_first", "ext_first", "prior"))),
        ]
    # the other horizons: the smallest the reference's timestep rule and the engine allow (3, 4), a run-time-K horizon below
    # the first template (9), and the largest allowed (45, two messages per lane, ever fewer neighbours before LDS runs out)
    cells += [
        _cell(3, 0, "seg_none", "none", 6, "tick"),
        _cell(3, 0, "seg_staged", "grid", 9, "reconnect"),
        _cell(3, 0, "resident", "grid", 9, "tick"),
        _cell(4, 0, "seg_staged", "grid", 9, "ext_first"),
        _cell(4, 0, "resident", "grid", 9, "prior"),
        _cell(9, 0, "seg_staged", "grid", 12, "tick"),
        _cell(9, 0, "resident", "grid", 12, "reconnect"),
        _cell(45, -1, "seg_none", "none", 6, "prior"),
        _cell(45, -1, "seg_staged", "line", 8, "tick"),
        _cell(45, -1, "seg_global", "dense", _crowd(45), "reconnect"),
        _cell(45, -1, "resident", "grid", 12, "ext_first"),
        _cell(45, -1, "posted", "line", 8, "tick"),
        _cell(45, -1, "sharded", "line", 10, "int_first"),
        # inter-robot and tracking factors together (the reference's arithmetic leaves the finite range)
        _cell(12, 12, "seg_staged", "grid", 12, "tick", tracking=True, tag="-trk"),
        _cell(16, 16, "resident", "grid", 12, "tick", tracking=True, tag="-trk"),
        # a non-square obstacle image whose border the robots' horizons cross: one constant K, one run-time K
        _cell(16, 16, "seg_staged", "border", 12, "tick"),
        _cell(16, 16, "resident", "border", 12, "tick"),
        _cell(9, 0, "seg_staged", "border", 12, "tick"),
        _cell(9, 0, "resident", "border", 12, "int_first"),
    ]
    return cells


CELLS = _table()


def _run(w, sc, script, after=None):
    """the cell's script on the engine (a World or a LocalCluster) or on the oracle; `after` runs behind every schedule"""
    after = after or (lambda: None)
    K, n = sc["K"], len(sc["robots"])
    if script == "tick":  # whole ticks with prior updates, back to back
        tick = S.tick_inputs(sc)
        for _ in range(3):
            w.tick(steps=INT_FIRST, **tick)
            after()
    elif script == "int_first":
        for steps in (INT_FIRST, [1, 1, 3], INT_FIRST):
            w.iterate(steps)
            after()
    elif script == "ext_first":
        for steps in (EXT_FIRST, [3, 1, 3]):
            w.iterate(steps)
            after()
    elif script == "prior":
        w.iterate(INT_FIRST)
        after()
        w.change_prior(n // 2, K - 1, np.array([3.0, -2.0, 0.5, 0.25]))
        w.change_prior(0, 0, np.array([-1.0, 1.5, 0.0, 0.0]))
        w.iterate(EXT_FIRST)
        after()
    elif script == "reconnect":
        a, b, n0 = sc["ir"][len(sc["ir"]) // 2]
        w.iterate(INT_FIRST)
        after()
        w.ir_disconnect(a, b)
        w.iterate(EXT_FIRST)
        after()
        w.ir_connect(a, b, n0 + 100000)
        w.iterate(INT_FIRST)
        after()
    else:
        raise ValueError(script)


def _compare(eng, ref, sc, tracking, what):
    if tracking:
        assert_identical_where_finite(eng, ref, what=what, max_nan_only_mismatch=5e-3)
    else:
        assert_identical(eng, ref, what=what)
    n = len(sc["robots"])
    for r in sorted({0, n // 2, n - 1}):
        assert eng.message_counts(r) == ref.message_counts(r), (what, r, eng.message_counts(r), ref.message_counts(r))


def _oracle(sc, script):
    ref = oracle.OracleWorld(sc["params"])
    S.populate(ref, sc)
    _run(ref, sc, script)
    return ref


def _run_world(cell, sc):
    eng = World(sc["params"])
    S.populate(eng, sc)
    if cell.form.startswith("seg_"):
        eng.set_resident_launches(False)
    elif cell.form == "resident":
        eng.set_linger(0)
    elif cell.form == "posted":
        eng.set_linger(50000)  # (long enough for the host's time between two ticks: the launch waits for the post)
    declined0 = eng.resident_stats()[1]
    seen = []
    _run(eng, sc, cell.script, after=lambda: seen.append(eng.last_sweep()))
    declined = eng.resident_stats()[1] - declined0
    if declined and not cell.form.startswith("seg_"):
        pytest.skip(f"{cell.name}: {declined} resident launch(es) declined by the residency census (shared GPU)")
    return eng, seen


def _run_sharded(cell, sc):
    from test_gpu_sharded import _own_stream_factory
    make, _streams = _own_stream_factory()
    cluster = sharded.LocalCluster(sc, 2, make, direct=True, resident=True)
    assert cluster.resident and all(sw.resident for sw in cluster.ranks)
    seen, declined = [], []

    def after():
        for sw in cluster.ranks:
            sw.synchronize()  # raises if a wait inside a launch gave up
        seen.append(cluster.ranks[0].world.last_sweep())
        for sw in cluster.ranks[1:]:
            assert sw.world.last_sweep() == seen[-1], (cell.name, sw.plan.rank, sw.world.last_sweep(), seen[-1])

    d0 = cluster.declined
    backing_off = any(sw.world.resident_stats()[2] > 0 for sw in cluster.ranks)
    _run(cluster, sc, cell.script, after=after)
    if cluster.declined > d0 or backing_off:
        pytest.skip(f"{cell.name}: {cluster.declined - d0} sharded resident launch(es) declined by the ranks' residency census "
                    "(shared GPU)")
    return cluster, seen


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_sweep_instantiation_matches_oracle(cell):
    sc = _scenario(cell.layout, cell.K, cell.n, tracking=cell.tracking)
    assert sc["K"] == cell.K
    eng, seen = (_run_sharded if cell.form == "sharded" else _run_world)(cell, sc)
    ir_mode, form = FORMS[cell.form]
    want = (cell.variant, ir_mode, form)
    got = seen[-1][:3]
    print(f"[{cell.name}] (variant, ir_mode, form) = {got}, resident capacity {seen[-1][3]}")
    assert got == want, (cell.name, "ran", got, "meant to run", want)
    for s in seen:  # every schedule of the script ran the same instantiation (a post runs in the launch it was posted into)
        assert s[:2] == want[:2], (cell.name, s, want)
        if cell.form == "posted":
            assert s[2] in (RESIDENT, POSTED), (cell.name, s)
        else:
            assert s[2] == form, (cell.name, s, want)
    if cell.form == "posted":
        assert eng.linger_stats()[1] >= 1, eng.linger_stats()
    if cell.form in ("resident", "posted", "sharded"):
        assert seen[-1][3] >= cell.n // (2 if cell.form == "sharded" else 1) + 1
    ref = _oracle(sc, cell.script)
    _compare(eng, ref, sc, cell.tracking, cell.name)


@pytest.mark.gpu
def test_no_resident_form_falls_back_to_unstaged_segments():
    """K = 45 with 31 neighbours: the resident workgroup would need more than the CU's 160 KB of LDS.  The world reports no
    resident capacity, runs launch per segment with the inter-robot messages read from L2 — with resident launches left on."""
    n = 32
    sc = _scenario("dense", 45, n)
    eng = World(sc["params"])
    S.populate(eng, sc)
    _run(eng, sc, "int_first")
    got = eng.last_sweep()
    print(f"[no resident form] {got}")
    assert got == (-1, IR_UNSTAGED, SEGMENTS, 0), got
    assert eng.resident_stats()[0] == 0
    _compare(eng, _oracle(sc, "int_first"), sc, False, "no resident form")


@pytest.mark.gpu
def test_resident_capacity_boundary():
    """The host keeps one workgroup slot free for the residency census' decider: with `cap` workgroups resident at once,
    cap - 1 robots run as one resident launch and cap robots fall back to launch per segment.  K = 45 on a line of robots
    (two neighbours each): the staged workgroup takes more than half a CU's LDS, so the capacity is one per CU."""
    probe = _scenario("line", 45, 8)
    w = World(probe["params"])
    S.populate(w, probe)
    w.set_linger(0)
    w.iterate(INT_FIRST)
    cap = w.last_sweep()[3]
    w.close()
    print(f"[capacity] K = 45, two neighbours: {cap} workgroups resident at once")
    assert cap > 2
    for n, form in ((cap - 1, RESIDENT), (cap, SEGMENTS)):
        sc = _scenario("line", 45, n)
        eng = World(sc["params"])
        S.populate(eng, sc)
        eng.set_linger(0)
        declined0 = eng.resident_stats()[1]
        _run(eng, sc, "int_first")
        got = eng.last_sweep()
        print(f"[capacity] {n} robots: {got}")
        if form == RESIDENT and eng.resident_stats()[1] > declined0:
            pytest.skip(f"{n} robots: the resident launch was declined by the residency census (shared GPU)")
        assert got == (-1, IR_STAGED, form, cap), (n, got)
        _compare(eng, _oracle(sc, "int_first"), sc, False, f"capacity boundary, {n} robots")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 46])
def test_horizon_out_of_range_is_refused(K):
    """K = 2 (below the smallest horizon the sweep kernel supports) and K = 46 (the first beyond the documented bound of 45 —
    its graph alone still fits the 60 KB check at commit, which let it through): an MgxError, not a crash"""
    ts = hostlib.variable_timesteps(_horizon_for(K), 3)
    assert len(ts) == K
    w = World(S.JUNCTION_PARAMS)
    w.set_sdf(np.full((16, 16, 3), 255, dtype=np.uint8), 50.0, 50.0)
    with pytest.raises(MgxError):  # (K = 2: when the robot is added; K = 46: when the world first goes to the device)
        w.add_robot(np.zeros((K, 4)), np.ones(K), np.ones(K - 1), 1.0)
        w.iterate(INT_FIRST)
    w.close()


@pytest.mark.gpu
def test_tick_rejects_cached_arguments_of_the_wrong_length():
    """World.tick remembers array arguments by identity: the same waypoint / time-scale / `what` objects with a longer robot
    list must be refused, not read past their ends"""
    sc = _scenario("grid", 10, 6)
    eng = World(sc["params"])
    S.populate(eng, sc)
    tick = S.tick_inputs(sc)
    eng.tick(steps=INT_FIRST, **tick)
    longer = np.arange(len(sc["robots"]) + 2, dtype=np.int32) % len(sc["robots"])
    with pytest.raises(ValueError):
        eng.tick(steps=INT_FIRST, **dict(tick, robots=longer))
    good_wp = np.zeros((len(longer), 2))
    good_ts = np.ones(len(longer))
    with pytest.raises(ValueError):  # `what` alone too short
        eng.tick(steps=INT_FIRST, **dict(tick, robots=longer, waypoints_xy=good_wp, time_scale=good_ts))
    eng.tick(steps=INT_FIRST, **tick)  # the remembered arrays still serve the robot list they fit


def test_table_covers_every_instantiation():
    """Static: the (variant, ir_mode, form) triples mgx_sweep_inst.hip instantiates — every horizon of its three sets in
    launch-per-segment form with no, unstaged and staged inter-robot messages, and in resident and sharded resident form —
    each have a cell, as has the lingering form; every cell's horizon runs the variant it claims."""
    src = open(INST).read()
    variants = []
    for m in re.finditer(r"#define MGX_K_LIST\(DO\)(.*)", src):
        variants += [int(v) for v in re.findall(r"DO\((-?\d+)\)", m.group(1))]
    assert sorted(variants) == sorted(FORM_K), variants
    triples = {(v, ir, form) for v in variants for ir, form in
               ((IR_NONE, SEGMENTS), (IR_UNSTAGED, SEGMENTS), (IR_STAGED, SEGMENTS), (IR_STAGED, RESIDENT), (IR_STAGED, SHARDED))}
    assert len(triples) == 60
    table = {(c.variant, *FORMS[c.form]) for c in CELLS}
    assert triples <= table, sorted(triples - table)
    assert {(v, IR_STAGED, POSTED) for v in variants} <= table
    for c in CELLS:
        assert c.variant == (c.K if c.K in CONST_K else (0 if 2 * (c.K - 1) <= 64 else -1)), c
        if c.form == "seg_global":
            assert _seg_lds(c.K, (c.n - 1) * (c.K - 1)) > 64 * 1024, c
    assert {3, 4, 9, 10, 11, 12, 13, 16, 17, 20, 21, 32, 33, 34, 35, 45} <= {c.K for c in CELLS}
    assert len({c.name for c in CELLS}) == len(CELLS)
    assert {c.script for c in CELLS} == {"tick", "int_first", "ext_first", "prior", "reconnect"}
