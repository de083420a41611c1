"""Enabled factor kinds per robot GROUP (include/mgx.h, ROBOT GROUPS: mgx_set_group_enabled): a world of 4 groups x 3 robots, K = 8,
every group with its own gbp.factors-enabled — against four worlds of their own, each created with that group's mask in mgx_params
and driven with the plain calls.  After every round each group's beliefs (as bit patterns), message counts and connections have to
be the solo world's.

World A: the open grid of tests/test_gpu_groups_schedules.py (pitch 4, comms radius 12, a blank obstacle image, tracking paths),
world mask 15, group masks 15, 7, 15, 14 — tracking off in group 1, dynamic off in group 3.  The blank image makes the obstacle
bit show in the message counts only, so it is tested in world B: the same grid at pitch 2.5 / radius 6 with obstacles and without
tracking, world mask 7, group masks 7, 3, 7, 6.  Seeds 805, 805, 806, 807 in both: groups 0 and 1 hold the SAME robots, so that
they end with different beliefs is what their masks do — the comparison cannot pass with the masks ignored.

The rounds: EQUAL schedules, which on a masked world run as a group plan (launch by launch, never resident:
mgx_group_enabled_stats), MIXED schedules together with the masks, the world-wide and the per-robot fine-grained calls; in between
prior changes, one antenna off and one idle robot per group, a topology pass that makes and breaks connections, and a robot spawned
in place into group 1 after the world has iterated.  Mission ticks on world A.  The refusals, each leaving the beliefs untouched.
The unmasked control: every group set to the world's own mask is a world that never heard of the call.

Finiteness of every solo world is asserted as a condition on the inputs."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S
from test_gpu_groups_schedules import GROUPS, HZ, K, PER_GROUP, SEEDS, SEGMENTS_FORM, SPAWN_GROUP, Pair, _drive, _same_bits, schedules, segments
from test_gpu_kernel_matrix import _grid

pytestmark = pytest.mark.gpu

F = np.float32
WORLDS = {"A": dict(masks=(15, 7, 15, 14), grid=dict(pitch=4.0, comm_radius=12.0, obstacles=False, tracking=True), radius=12.0),
          "B": dict(masks=(7, 3, 7, 6), grid=dict(pitch=2.5, comm_radius=6.0, obstacles=True, tracking=False), radius=6.0)}


def group_scenarios(world, masks=None):
    """one scenario per group: the world's grid under the group's seed, the group's mask in its params (the shared world is made
    from group 0's, whose mask is the world's)"""
    spec = WORLDS[world]
    masks = spec["masks"] if masks is None else masks
    scs = []
    for g in range(GROUPS):
        sc = _grid(PER_GROUP + 1, K, interrobot=True, seed=SEEDS[g], **spec["grid"])
        assert sc["params"]["enable_mask"] == masks[0], "group 0 has the world's mask"
        sc["params"] = dict(sc["params"], enable_mask=masks[g])
        scs.append(sc)
    return scs


class MaskedPair(Pair):
    """Pair whose shared world gives every group its mask before the first robot goes in; the groups' own worlds have theirs from
    their params.  set_masks=False: a world that is never told"""

    def __init__(self, world="A", masks=None, set_masks=True, **kw):
        self.masks = tuple(WORLDS[world]["masks"] if masks is None else masks)
        self._masks_pending = set_masks
        super().__init__(scs=group_scenarios(world, self.masks), radius=WORLDS[world]["radius"], **kw)

    def add(self, g, i):
        if self._masks_pending:
            self._masks_pending = False
            for q, mask in enumerate(self.masks):
                self.shared.set_group_enabled(self.gid[q], mask)
                assert self.shared.group_enabled(self.gid[q]) == mask
        super().add(g, i)

    def finite(self, what):
        """a condition on the chosen inputs: every solo world's beliefs are numbers"""
        for g, w in enumerate(self.alone):
            for name, a in zip(("eta", "lam", "mean"), w.read_beliefs()):
                assert np.isfinite(a).all(), (what, "the solo world of group", g, "left the finite range in", name)

    def check(self, what):
        self.finite(what)
        self.same(what)

    def groups_0_and_1_differ(self):
        means = self.beliefs()[2]
        return not np.array_equal(means[self.ids[0]], means[self.ids[1]])


def _equal(p, steps, what, as_groups):
    """one EQUAL schedule on the masked world: a group plan of the schedule's segments, not resident, counted by the new statistic"""
    plans0, launches0 = p.shared.group_enabled_stats()
    mixed0, resident0 = p.shared.group_schedule_stats(), p.shared.resident_stats()[0]
    if as_groups:
        p.iterate([steps] * p.n)
    else:
        p.shared.iterate(steps)
        for w in p.alone:
            w.iterate(steps)
    n = len(segments(steps))
    assert p.shared.last_launch_count() == n, what
    assert p.shared.last_sweep()[2] == SEGMENTS_FORM, (what, p.shared.last_sweep())
    assert p.shared.group_enabled_stats() == (plans0 + 1, launches0 + n), what
    assert p.shared.group_schedule_stats() == mixed0 and p.shared.resident_stats()[0] == resident0, what
    p.check(what)


def _mixed(p, per_group, what):
    plans0 = p.shared.group_enabled_stats()
    calls0, launches0, _ = p.shared.group_schedule_stats()
    p.iterate(per_group)
    most = max(len(segments(s)) for s in per_group)
    assert p.shared.last_launch_count() == most, what
    assert p.shared.last_sweep()[2] == SEGMENTS_FORM, what
    assert p.shared.group_schedule_stats()[:2] == (calls0 + 1, launches0 + most), what
    assert p.shared.group_enabled_stats() == plans0, what             # (a mixed call is a mixed call, masks or none)
    p.check(what)


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_every_group_runs_under_its_own_kinds(world):
    p = MaskedPair(world, reserve=1)
    sch = schedules()
    assert p.shared.group_enabled_stats() == (0, 0)
    p.topology()
    assert p.created > 0
    p.check((world, "topology"))                                       # (the robots' counts at creation are per mask already)
    _equal(p, sch[0], (world, 0, "equal"), as_groups=True)
    p.prior_changes()
    p.flags(antenna_off=0, idle=1)
    _mixed(p, [sch[0], sch[0], sch[2], sch[3]], (world, 1, "mixed"))   # (groups 0 and 1 alike: what tells them apart is their masks)
    p.flags()
    p.topology(far=(2,))
    assert p.deleted > 0
    _equal(p, sch[1], (world, 2, "equal"), as_groups=False)
    # the same robots under the same schedules so far (the tracking factors of world A start at the tenth factor iteration)
    assert p.groups_0_and_1_differ(), "their masks make the difference"
    p.topology()
    p.add(SPAWN_GROUP, PER_GROUP)                                      # into the group whose mask lacks a kind, after the world has iterated
    p.prior_changes()
    _mixed(p, [sch[1], sch[2], sch[3], sch[0]], (world, 3, "mixed"))
    assert p.shared.append_stats()[0] >= 1                             # the spawn went in place
    p.topology()                                                       # the newcomer meets its group
    _equal(p, sch[3], (world, 4, "equal"), as_groups=True)
    # the fine-grained calls: world-wide ones are group plans of one launch, per-robot ones carry their robot's kinds
    plans0, launches0 = p.shared.group_enabled_stats()
    for w in [p.shared] + p.alone:
        w.sweep(3, 3, 1)
        w.external_factor_iteration()
        w.internal_factor_iteration()
        w.internal_variable_iteration()
    assert p.shared.group_enabled_stats() == (plans0 + 4, launches0 + 4)
    assert p.shared.last_sweep()[2] == SEGMENTS_FORM
    p.check((world, "world-wide fine-grained"))
    for g in range(p.n):
        for world_, r in ((p.shared, p.ids[g][1]), (p.alone[g], 1)):
            world_.internal_factor_iteration(r)
            world_.internal_variable_iteration(r)
            world_.sweep(0, 3, 2, robot=r)
    assert p.shared.group_enabled_stats() == (plans0 + 4, launches0 + 4)
    p.check((world, "per-robot fine-grained"))
    assert p.groups_0_and_1_differ()
    assert p.shared.resident_stats()[0] == 0                           # never resident
    for w in p.alone:
        assert w.group_enabled_stats() == (0, 0)


def test_mission_ticks_on_a_masked_world():
    """mgx_mission_tick_begin_groups / mgx_mission_tick_end on world A: the prior updates go as the kernel of their own, the
    schedule — mixed in the first tick, equal in the second — as a group plan.  The solo worlds are driven with update_topology
    and tick."""
    p = MaskedPair("A")
    sch = schedules()
    dt32 = F(1.0) / F(HZ)
    for g in range(p.n):
        for i, rid in enumerate(p.ids[g]):
            rb = p.robots(g)[i]
            r2, cur = float(F(rb["radius"]) * F(rb["radius"])), rb["mean0"][0]
            p.shared.mission_set(rid, np.asarray([tuple(rb["goal"])], dtype=np.float64), K - 1, 0, r2, r2, (F(cur[0]), F(0.5), F(cur[1])),
                                 float(dt32 / rb["t0"]))
    for n, per_group in enumerate((sch, [sch[0]] * GROUPS)):
        tr = np.asarray(p.shared.mission_read()[0], dtype=F).reshape(-1, 3)
        for g, w in enumerate(p.alone):
            p.nxt_alone[g], c, d = w.update_topology(tr[p.ids[g]], p.radius, p.nxt_alone[g])
            p.created += c
        p.nxt, stats, fin = p.shared.mission_tick_begin_groups(p.radius, p.nxt, despawn_finished=True)
        assert not len(fin) and [int(x) for x in p.nxt] == p.nxt_alone, (n, fin, p.nxt, p.nxt_alone)
        before = p.shared.group_enabled_stats(), p.shared.group_schedule_stats()[0]
        p.shared.mission_tick_end(per_group, float(F(p.scs[0]["target_speed"])), float(dt32))
        for g, w in enumerate(p.alone):
            w.tick(steps=per_group[g], **S.tick_inputs({"robots": p.robots(g), "target_speed": p.scs[g]["target_speed"]}, HZ))
        most = max(len(segments(s)) for s in per_group)
        assert p.shared.last_launch_count() == most and p.shared.last_sweep()[2] == SEGMENTS_FORM, n
        if n == 0:
            assert (p.shared.group_enabled_stats(), p.shared.group_schedule_stats()[0]) == (before[0], before[1] + 1)
        else:
            assert (p.shared.group_enabled_stats(), p.shared.group_schedule_stats()[0]) == ((before[0][0] + 1, before[0][1] + most), before[1])
        p.check(("mission tick", n))
    assert p.created > 0
    assert p.groups_0_and_1_differ()
    assert p.shared.resident_stats()[0] == 0


def _untouched(world, before, what):
    for x, y in zip(before, world.read_beliefs()):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), what


def test_refusals_leave_the_world_as_it_was():
    p = MaskedPair("A")
    p.topology()
    p.iterate(schedules())
    w = p.shared
    before = w.read_beliefs()
    stats = w.group_enabled_stats(), w.group_schedule_stats()
    with pytest.raises(hostlib.MgxError, match="fixed before its first robot"):          # a group that has a robot (group 0 like any other)
        w.set_group_enabled(0, 7)
    with pytest.raises(hostlib.MgxError, match="fixed before its first robot"):
        w.set_group_enabled(1, 15)
    with pytest.raises(hostlib.MgxError, match="inter-robot kind"):                      # a group without robots, but the world's bit 2 is on
        w.set_group_enabled(GROUPS, 13)
    with pytest.raises(hostlib.MgxError, match="mgx_set_group_enabled"):                  # freeze and thaw stay world-wide
        w.set_enabled(7)
    w.set_enabled(15)                                                                    # (the world's own mask: nothing to do)
    with pytest.raises(hostlib.MgxError, match="mgx_mission_run"):
        w.mission_run(2, p.radius, 1, schedules()[0], 1.0, 0.1)
    with pytest.raises(hostlib.MgxError, match="unknown factor kind"):
        w.set_group_enabled(GROUPS, 16)
    with pytest.raises(hostlib.MgxError, match="MGX_GROUPS_MAX"):
        w.set_group_enabled(hostlib.GROUPS_MAX, 15)
    assert [w.group_enabled(g) for g in range(GROUPS + 1)] == list(p.masks) + [15]
    _untouched(w, before, "refusals on a masked world")
    assert (w.group_enabled_stats(), w.group_schedule_stats()) == stats
    w.set_group_enabled(GROUPS, 5 | 2)                                                   # a group still without robots takes a mask
    assert w.group_enabled(GROUPS) == 7
    p.iterate(schedules())
    p.check("behind the refusals")
    # a world that has switched a kind at run time takes no masks: the thaw kernels are world-wide
    q = Pair()
    q.topology()
    q.iterate(schedules())
    q.shared.set_enabled(S.EN_DYN | S.EN_OBS | S.EN_IR)
    before = q.shared.read_beliefs()
    with pytest.raises(hostlib.MgxError, match="mgx_set_enabled"):
        q.shared.set_group_enabled(GROUPS, 3)
    assert q.shared.group_enabled(GROUPS) == 7
    _untouched(q.shared, before, "set_group_enabled behind set_enabled")
    # ... and neither does a world with a ghost
    sc = group_scenarios("A")[0]
    g = World(sc["params"])
    g.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    for i, rb in enumerate(sc["robots"][:3]):
        g.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=i, ghost=(i == 2))
    with pytest.raises(hostlib.MgxError, match="ghosts"):
        g.set_group_enabled(3, 7)


def test_every_group_at_the_worlds_mask_is_an_unmasked_world():
    """the control: the same world with every group SET to the world's mask makes the launches, the last_sweep answers and the
    group_schedule_stats of a world that never heard of the call — resident launches and posts included"""
    same = (15,) * GROUPS
    a, b = MaskedPair("A", masks=same), MaskedPair("A", masks=same, set_masks=False)
    for q in (a, b):
        q.topology()
    sch = schedules()
    ran_a, bel_a, res_a, linger_a, mixed_a = _drive(a.shared, [sch[0]] * GROUPS)
    ran_b, bel_b, res_b, linger_b, mixed_b = _drive(b.shared, [sch[0]] * GROUPS)
    assert ran_a == ran_b and _same_bits(bel_a, bel_b)
    assert res_a == res_b and linger_a == linger_b and mixed_a == mixed_b == (0, 0, 0)
    for q in (a, b):
        q.prior_changes()
        q.iterate(sch)
    assert (a.shared.last_launch_count(), a.shared.last_sweep()) == (b.shared.last_launch_count(), b.shared.last_sweep())
    assert a.shared.group_schedule_stats() == b.shared.group_schedule_stats() and a.shared.group_schedule_stats()[0] == 1
    assert _same_bits(a.shared.read_beliefs(), b.shared.read_beliefs())
    assert a.shared.group_enabled_stats() == b.shared.group_enabled_stats() == (0, 0)
    a.shared.set_enabled(7)                                            # ... and freeze and thaw are still its own
    assert a.shared.group_enabled(0) == 7
