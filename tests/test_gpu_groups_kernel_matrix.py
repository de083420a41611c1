"""Mixed per-group schedules (mgx_iterate_groups, mgx_mission_tick_end_groups) on EVERY launch-per-segment instantiation of the
sweep kernel, against the CPU oracle.

A mixed call runs launch by launch through run_group_plan (mgx_world_launch.inc): the host passes all-zero kernel scalars and a
world-wide snap_out, and every !PERSIST instantiation of k_robot_sweep overwrites the scalars with its group's GroupSeg record
(mgx_sweep.h).  The twelve horizon variants x {no, unstaged, staged} inter-robot messages differ exactly where that code sits:
run-time K or constant K, the four-lane belief finish (K <= 16), two dynamic messages per lane (K >= 34), messages staged in LDS or
read from L2, and what the HINT_* bits let the write-back skip.  Every cell below is one shared World of four groups — robot ids
interleaved across the groups — against one oracle.OracleWorld per group that holds that group's robots and is driven with the
plain calls; the vocabulary (FORM_K, _crowd ...) is the ungrouped matrix's, the world layout is Pair's (test_gpu_groups_schedules).

Four rounds per cell: the four mixed schedules; one mutator, then the schedules permuted with one group sitting out; EQUAL
schedules (the plain call: resident or posted where the world can) followed with no read in between by the mixed schedules again —
the hand-over from a launch that may still linger, on the buffer parity it left.  Which kernel ran is read back from the engine
(last_sweep), the launches and the workgroups that sat out are computed from the restated plans (segments()).

Same file: the plan's edges at K = 10 (more than MAX_SEGS segments, more than 255 internal iterations in a segment, external-only
schedules, sparse group ids up to MGX_GROUPS_MAX - 1, an emptied group, a group of one) and mission ticks with per-group schedules."""
import re
from collections import namedtuple

import numpy as np
import pytest

import oracle
from magics_amd import hostlib, scenarios as S
from test_gpu_groups_schedules import E, I, Pair, schedules, segments
from test_gpu_kernel_matrix import CONST_K, FORM_K, FORMS, INST, IR_NONE, IR_STAGED, IR_UNSTAGED, SEGMENTS, _crowd, _grid, _seg_lds

SEEDS = (805, 805, 806, 807)           # (groups 0 and 1: the same robots)
PER_GROUP, SPAWN_GROUP, REMOVE_GROUP = 3, 1, 2
MUTATORS = ("prior", "topology", "flags", "spawn", "remove")
F = np.float32


def group_scenario(layout, K, n, seed, tracking=False):
    """one group's robots (and the comms radius that goes with the layout)"""
    if layout == "none":     # no inter-robot factors
        return _grid(n, K, interrobot=False, pitch=2.5, seed=seed, tracking=tracking), 6.0
    if layout == "near":     # a 2 x 2 block, everyone within range of everyone
        return _grid(n, K, interrobot=True, pitch=2.5, comm_radius=6.0, seed=seed, tracking=tracking), 6.0
    if layout == "open":     # the same block wider apart and without obstacles: where the tracking factors keep the oracle finite
        return _grid(n, K, interrobot=True, pitch=4.0, comm_radius=12.0, obstacles=False, seed=seed, tracking=tracking), 12.0
    if layout == "line":     # one row, neighbours in range, next but one out of it
        return _grid(n, K, interrobot=True, pitch=2.5, comm_radius=3.6, grid_side=n, seed=seed, tracking=tracking), 3.6
    if layout == "dense":    # the crowd: everyone hears everyone
        return _grid(n, K, interrobot=True, pitch=1.2, comm_radius=1000.0, obstacles=False, seed=seed, tracking=tracking), 1000.0
    raise ValueError(layout)


def group_schedules():
    """interleave-evenly 3 / 3 and 5 / 3 (groups 0 and 1: four segments each, one and two internal iterations a segment),
    internal 1 / external 4 (external-only segments), late-as-possible 2 / 2 (three segments: it sits the last launch out)"""
    s = schedules()
    s[1] = hostlib.schedule(hostlib.SCHEDULE_INTERLEAVE_EVENLY, 5, 3)
    assert [len(segments(x)) for x in s] == [4, 4, 4, 3] and len({tuple(x) for x in s}) == 4
    return s


def writing_launches(per_group):
    """launches of a mixed call in which some group runs an internal iteration: the ones that write snapshots"""
    plans = [segments(s) for s in per_group]
    return sum(any(k < len(p) and p[k][1] > 0 for p in plans) for k in range(max(len(p) for p in plans)))


class OraclePair(Pair):
    """Pair with the groups' own worlds on the CPU oracle"""

    def __init__(self, layout, K, seeds=SEEDS, sizes=None, tracking=False, crowd=0, **kw):
        sizes = list(sizes) if sizes is not None else [PER_GROUP] * len(seeds)
        scs, radius = [], None
        for g, seed in enumerate(seeds):
            if g == 0 and crowd:   # group 0 is the dense crowd: the world-wide inter-robot mode follows the most crowded robot
                sc, radius = group_scenario("dense", K, crowd, seed, tracking)
                sizes[0] = crowd
            else:
                sc, r = group_scenario(layout, K, sizes[g] + 1, seed, tracking)   # (+ 1: the robot that may be spawned later)
                radius = radius if crowd else r
            assert sc["K"] == K
            scs.append(sc)
        # (the crowd's oracle is the slow one: threaded, as every oracle of the suite that has many robots)
        super().__init__(scs=scs, sizes=sizes, radius=radius, spawn_group=SPAWN_GROUP, reserve=1,
                         alone=lambda params: oracle.OracleWorld(params, threads=8 if crowd and params is scs[0]["params"] else 1), **kw)

    def live(self, g):
        return [i for i in range(len(self.ids[g])) if (g, i) not in self.gone]

    def remove(self, g, i):
        self.shared.remove_robot(self.ids[g][i])
        self.alone[g].remove_robot(i)
        self.gone.add((g, i))

    def finite(self, what):
        """a condition on the chosen inputs: every oracle belief is a number"""
        for g, w in enumerate(self.alone):
            for name, a in zip(("eta", "lam", "mean"), w.read_beliefs()):
                assert np.isfinite(a).all(), (what, "the oracle of group", g, "left the finite range in", name)

    def plan(self, per_group):
        """(launches, workgroups that sit a launch out) of one mixed call, from the restated plans and the live group sizes"""
        counts = [len(segments(s)) for s in per_group]
        most = max(counts)
        return most, sum(len(self.live(g)) * (most - c) for g, c in enumerate(counts))

    def mixed(self, per_group, what, want=None):
        """one mixed call: the launches it has to take, the kernel it has to run, every group against its oracle"""
        assert len({tuple(s) for g, s in enumerate(per_group) if self.live(g)}) > 1, (what, "not a mixed call")
        self.iterate(per_group)
        most, sat = self.plan(per_group)
        assert self.shared.last_launch_count() == most, (what, self.shared.last_launch_count(), most)
        got = self.shared.last_sweep()[:3]
        if want is not None:
            assert got == want, (what, "ran", got, "meant to run", want)
        assert got[2] == SEGMENTS, (what, got)
        self.finite(what)
        self.same(what)
        return most, sat


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
Cell = namedtuple("Cell", "name K variant form layout mutator tracking")


def _cell(K, variant, form, layout, mutator, tracking=False):
    return Cell(f"K{K}-{form}-{layout}-{mutator}{'-trk' if tracking else ''}", K, variant, form, layout, mutator, tracking)


def _table():
    cells = []
    # (no inter-robot factors: a topology pass would leave keyless connections, and a world that has them refuses mixed schedules;
    # the crowd: one robot out of range and the messages fit LDS again — the staged cells take the topology mutator)
    rest = tuple(m for m in MUTATORS if m != "topology")
    for i, (variant, K) in enumerate(FORM_K.items()):
        rot = lambda j, pool: pool[(i + j) % len(pool)]
        cells += [_cell(K, variant, "seg_none", "none", rot(0, rest)),
                  _cell(K, variant, "seg_staged", "near", rot(1, MUTATORS)),
                  _cell(K, variant, "seg_global", "dense", rot(2, rest))]
    cells += [_cell(3, 0, "seg_staged", "near", "topology"),
              _cell(4, 0, "seg_staged", "near", "spawn"),
              _cell(9, 0, "seg_staged", "near", "remove"),
              _cell(45, -1, "seg_staged", "line", "flags"),      # (three neighbours would not fit LDS any more)
              _cell(45, -1, "seg_global", "dense", "prior"),
              # inter-robot and tracking factors together
              _cell(12, 12, "seg_staged", "open", "spawn", tracking=True),
              _cell(16, 16, "seg_staged", "open", "topology", tracking=True)]  # (not spawn: there its oracle leaves the finite range)
    return cells


CELLS = _table()


def _mutate(p, mutator):
    if mutator == "prior":
        p.prior_changes()
    elif mutator == "topology":
        p.topology(far=(2,))
        assert p.deleted > 0
    elif mutator == "flags":
        p.flags(antenna_off=0, idle=1)
    elif mutator == "spawn":
        p.add(SPAWN_GROUP, PER_GROUP)
        if p.scs[0]["params"]["enable_mask"] & S.EN_IR:
            p.topology()                       # the newcomer meets its group
    elif mutator == "remove":
        p.remove(REMOVE_GROUP, 1)
    else:
        raise ValueError(mutator)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_mixed_schedules_on_every_instantiation(cell):
    sch = group_schedules()
    assert any(ext and n == 0 for ext, n in segments(sch[2])[:-1]), "internal 1 / external 4 has external-only segments in front of its last"
    assert len(segments(sch[3])) < min(len(segments(s)) for s in sch[:3]), "late-as-possible 2 / 2 sits the later launches out"
    ir_mode, form = FORMS[cell.form]
    want = (cell.variant, ir_mode, form)
    p = OraclePair(cell.layout, cell.K, tracking=cell.tracking, crowd=_crowd(cell.K) if cell.form == "seg_global" else 0)
    assert sum(len(x) for x in p.ids) <= _crowd(cell.K) + 9
    if ir_mode == IR_NONE:
        assert not p.scs[0]["params"]["enable_mask"] & S.EN_IR
    else:
        p.topology()
        assert p.created > 0
    launches = sat_out = 0
    # round 1: the four mixed schedules
    most, sat = p.mixed(sch, (cell.name, 1), want)
    launches, sat_out = launches + most, sat_out + sat
    if p.sizes[0] == p.sizes[1]:   # the same robots under two schedules: not the same beliefs
        differ = [not np.array_equal(b[p.ids[0]], b[p.ids[1]]) for b in p.beliefs()]
        # (three variables: the means do not move in one call, the precisions do)
        assert differ[2] if cell.K > 3 else differ[1], differ
    # round 2: one mutator, the schedules permuted, group 0 with no schedule at all.  Group 0 ran an internal iteration in the last
    # launch of round 1 that wrote snapshots, so its records in the two buffers differ — and it now sits out an ODD number of
    # launches that write: without the copy of the sits-out path the world would go on with the older ones
    _mutate(p, cell.mutator)
    per_group = [[], sch[3], sch[0], sch[2]]
    assert writing_launches(sch) % 2 == 1 and segments(sch[0])[2] == (True, 1) and writing_launches(per_group) % 2 == 1
    most, sat = p.mixed(per_group, (cell.name, 2), want)
    launches, sat_out = launches + most, sat_out + sat
    if cell.mutator == "spawn":
        assert p.shared.append_stats()[0] >= 1   # (in place)
    # round 3: equal schedules — the plain call, resident or posted where the world can — and, with no read in between, round 4:
    # the mixed schedules again, behind a launch that may still linger and on the buffer parity it left
    p.iterate([sch[1]] * 4)
    p.finite((cell.name, 3))
    most, sat = p.mixed(sch, (cell.name, 4), want)
    launches, sat_out = launches + most, sat_out + sat
    assert sat_out > 0
    assert p.shared.group_schedule_stats() == (3, launches, sat_out)


def test_groups_table_covers_every_instantiation():
    """Static: every launch-per-segment (variant, ir_mode) of mgx_sweep_inst.hip has a mixed-schedule cell, every cell's horizon
    runs the variant it claims, the crowds are crowds, and all five mutators occur."""
    src = open(INST).read()
    variants = []
    for m in re.finditer(r"#define MGX_K_LIST\(DO\)(.*)", src):
        variants += [int(v) for v in re.findall(r"DO\((-?\d+)\)", m.group(1))]
    assert sorted(variants) == sorted(FORM_K), variants
    triples = {(v, ir, SEGMENTS) for v in variants for ir in (IR_NONE, IR_UNSTAGED, IR_STAGED)}
    assert len(triples) == 36
    table = {(c.variant, *FORMS[c.form]) for c in CELLS}
    assert triples <= table, sorted(triples - table)
    for c in CELLS:
        assert FORMS[c.form][1] == SEGMENTS, c
        assert c.variant == (c.K if c.K in CONST_K else (0 if 2 * (c.K - 1) <= 64 else -1)), c
        if c.form == "seg_global":
            assert _seg_lds(c.K, (_crowd(c.K) - 1) * (c.K - 1)) > 64 * 1024, c
        if c.form == "seg_staged":   # ... and the groups of three, a fourth spawned in, are not (a line: two neighbours at most)
            assert _seg_lds(c.K, (2 if c.layout == "line" else 3) * (c.K - 1)) <= 64 * 1024, c
    assert {3, 4, 9, 10, 11, 12, 13, 16, 17, 20, 21, 32, 33, 34, 35, 45} <= {c.K for c in CELLS}
    assert {(c.K, c.form) for c in CELLS if c.tracking} == {(12, "seg_staged"), (16, "seg_staged")}
    assert {(45, "seg_staged", "line"), (45, "seg_global", "dense")} <= {(c.K, c.form, c.layout) for c in CELLS}
    assert len({c.name for c in CELLS}) == len(CELLS)
    assert {c.mutator for c in CELLS} == set(MUTATORS)
    assert max(_crowd(c.K) for c in CELLS if c.form == "seg_global") + 9 < 120


# ---- the plan's edges: K = 10, staged ----------------------------------------------------------------------------------------------
EDGE_K = 10
EDGE_WANT = (10, IR_STAGED, SEGMENTS)


def _edge_pair(seeds, **kw):
    p = OraclePair("near", EDGE_K, seeds=seeds, **kw)
    p.topology()
    assert p.created > 0
    return p


@pytest.mark.gpu
def test_more_segments_than_a_resident_plan_holds():
    """40 [E I] segments beside one: a mixed call is never resident, so MAX_SEGS = 32 does not cap it"""
    p = _edge_pair((805, 806))
    per_group = [[E, I] * 40, [I]]
    assert [len(segments(s)) for s in per_group] == [40, 1]
    most, sat = p.mixed(per_group, "40 segments", EDGE_WANT)
    assert (most, sat) == (40, 39 * PER_GROUP)
    assert p.shared.group_schedule_stats() == (1, 40, sat)


@pytest.mark.gpu
def test_more_internal_iterations_than_a_byte_counts():
    """300 internal iterations in ONE segment (GroupSeg::n_int has 32 bits, SegPlan's counts are bytes) beside a 3-step group"""
    p = _edge_pair((805, 806))
    per_group = [[I] * 300, [I, E, I]]
    assert segments(per_group[0]) == [(False, 300)] and len(segments(per_group[1])) == 2
    most, sat = p.mixed(per_group, "300 internal", EDGE_WANT)
    assert (most, sat) == (2, PER_GROUP)
    most, sat = p.mixed([[I, E, I], [I] * 300], "300 internal, the other way round", EDGE_WANT)
    assert p.shared.group_schedule_stats() == (2, 4, 2 * PER_GROUP)


@pytest.mark.gpu
def test_external_only_schedules():
    """every group external-only, of different lengths: no launch writes snapshots, the buffer parity stays, and the plain
    iterate behind it reads the right one"""
    p = _edge_pair((805, 806, 807))
    p.mixed([[I, E, I], [I, I], [I | E, I]], "warm-up", EDGE_WANT)   # (messages to exchange)
    per_group = [[E], [E, E], [E, E, E]]
    assert [segments(s) for s in per_group] == [[(True, 0)] * n for n in (1, 2, 3)]
    most, sat = p.mixed(per_group, "external only", EDGE_WANT)
    assert (most, sat) == (3, 3 * PER_GROUP)
    steps = [I, E | I, I]
    p.shared.iterate(steps)
    for w in p.alone:
        w.iterate(steps)
    p.finite("plain iterate behind external-only schedules")
    p.same("plain iterate behind external-only schedules")
    p.mixed(per_group[::-1], "external only again", EDGE_WANT)
    p.mixed([[I, E], [E, I], [I]], "mixed behind external only", EDGE_WANT)
    assert p.shared.group_schedule_stats()[0] == 4


@pytest.mark.gpu
def test_sparse_group_ids():
    """robots in groups 0, 5 and MGX_GROUPS_MAX - 1 of n_groups = MGX_GROUPS_MAX: a record table of n_launches x 4096"""
    top = hostlib.GROUPS_MAX
    p = _edge_pair((805, 806, 807), group_ids=(0, 5, top - 1), n_groups=top)
    sch = group_schedules()
    per_group = [sch[2], sch[0], sch[3]]
    assert len(p.per_group_of_world(per_group)) == top
    launches = sat_out = 0
    for n, pg in enumerate((per_group, per_group[::-1], [sch[1], [], sch[2]])):
        most, sat = p.mixed(pg, ("sparse ids", n), EDGE_WANT)
        launches, sat_out = launches + most, sat_out + sat
    assert p.shared.group_schedule_stats() == (3, launches, sat_out)


@pytest.mark.gpu
def test_an_emptied_group_keeps_its_schedule():
    """a group whose robots have all been removed: its schedule does not make a call mixed, and it sits nothing out"""
    p = _edge_pair((805, 806, 807))
    sch = group_schedules()
    for i in range(PER_GROUP):
        p.remove(2, i)
    p.iterate([sch[0], sch[0], sch[2]])                # equal among the groups that hold robots: the plain call
    assert p.shared.group_schedule_stats() == (0, 0, 0)
    p.finite("emptied group, equal")
    p.same("emptied group, equal")
    per_group = [[I], [I, E, I], sch[2]]                # ... the emptied group with the most segments of all
    counts = [len(segments(s)) for s in per_group]
    assert counts == [1, 2, 4]
    most, sat = p.mixed(per_group, "emptied group, mixed", EDGE_WANT)
    assert (most, sat) == (counts[2], PER_GROUP * (2 * counts[2] - counts[0] - counts[1]))
    assert p.shared.group_schedule_stats() == (1, most, sat)


@pytest.mark.gpu
def test_a_group_of_one():
    """a robot with no inter-robot edge at all in a kernel compiled with inter-robot messages, next to connected groups"""
    p = _edge_pair((805, 806, 807), sizes=(1, 3, 2))
    assert p.shared.connections(p.ids[0][0]) == []
    sch = group_schedules()
    launches = sat_out = 0
    for n, pg in enumerate(([sch[2], sch[0], sch[3]], [sch[3], sch[2], sch[1]], [[], sch[1], sch[2]])):
        most, sat = p.mixed(pg, ("group of one", n), EDGE_WANT)
        launches, sat_out = launches + most, sat_out + sat
    assert p.shared.group_schedule_stats() == (3, launches, sat_out)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [10, 20])
def test_mission_ticks_with_a_schedule_per_group(K):
    """mgx_mission_tick_begin_groups / mgx_mission_tick_end with one schedule per group: the prior updates do not ride in a mixed
    launch (they go as the kernel of their own).  The oracles are driven with update_topology and tick."""
    p = OraclePair("near", K, seeds=(805, 806, 807))
    sch = group_schedules()
    dt32 = F(1.0) / F(10.0)
    for g in range(p.n):
        for i, rid in enumerate(p.ids[g]):
            rb = p.robots(g)[i]
            r2, cur = float(F(rb["radius"]) * F(rb["radius"])), rb["mean0"][0]
            p.shared.mission_set(rid, np.asarray([tuple(rb["goal"])], dtype=np.float64), K - 1, 0, r2, r2, (F(cur[0]), F(0.5), F(cur[1])),
                                 float(dt32 / rb["t0"]))
    launches = sat_out = 0
    rounds = ([sch[0], sch[2], sch[3]], [sch[2], sch[3], sch[1]], [sch[1]] * 3, [sch[3], [], sch[2]])
    for n, per_group in enumerate(rounds):
        tr = np.asarray(p.shared.mission_read()[0], dtype=F).reshape(-1, 3)
        for g, w in enumerate(p.alone):
            p.nxt_alone[g], c, d = w.update_topology(tr[p.ids[g]], p.radius, p.nxt_alone[g])
            p.created += c
        p.nxt, stats, fin = p.shared.mission_tick_begin_groups(p.radius, p.nxt, despawn_finished=True)
        assert not len(fin) and [int(x) for x in p.nxt] == p.nxt_alone, (n, fin, p.nxt, p.nxt_alone)
        p.shared.mission_tick_end(per_group, float(F(p.scs[0]["target_speed"])), float(dt32))
        for g, w in enumerate(p.alone):
            tick = S.tick_inputs({"robots": p.robots(g), "target_speed": p.scs[g]["target_speed"]})
            if len(per_group[g]):
                w.tick(steps=per_group[g], **tick)
            else:
                w.update_priors(**tick)
        if len({tuple(s) for s in per_group}) > 1:
            most, sat = p.plan(per_group)
            assert p.shared.last_launch_count() == most, n
            assert p.shared.last_sweep()[:3] == (K, IR_STAGED, SEGMENTS), (n, p.shared.last_sweep())
            launches, sat_out = launches + most, sat_out + sat
        p.finite(("mission tick", n))
        p.same(("mission tick", n))
    assert p.created > 0
    assert p.shared.group_schedule_stats() == (3, launches, sat_out)
