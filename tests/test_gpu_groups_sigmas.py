"""Factor sigmas per robot GROUP (include/mgx.h, ROBOT GROUPS: mgx_set_group_sigmas): the two worlds of
tests/test_gpu_groups_factors.py — 4 groups x 3 robots, K = 8 — every group with its own gbp.sigma-factor-*, against four worlds of
their own, each created with that group's sigmas in mgx_params and driven with the plain calls.  After every round each group's
beliefs (as bit patterns), message counts and connections have to be the solo world's.

World A (pitch 4, comms radius 12, a blank obstacle image, tracking on): sigma_tracking and sigma_dynamics change the beliefs
there — the image is blank and the robots keep outside the safety distance, so sigma_obstacle and sigma_interrobot do not.  Groups:
the world's; tracking 0.15; tracking 0.5; dynamics 0.05 together with the mask without tracking (a group with a mask AND sigmas).
World B (pitch 2.5, radius 6, obstacles, tracking off): obstacle, inter-robot and dynamics change the beliefs.  Groups: the
world's; obstacle 0.05; inter-robot 0.05; dynamics 0.05.  The world's sigmas are 0.1 / 0.01 / 0.01 / 0.01 in both.
Seeds 805, 805, 806, 807: groups 0 and 1 hold the SAME robots, so that they end with different beliefs is what their sigmas do —
the comparison cannot pass with the sigmas ignored.

Such a world is run as a masked world is: equal schedules as group plans (mgx_group_enabled_stats), with
mgx_set_group_resident as resident launches and posts of the masked form (mgx_group_resident_stats).  The rounds are those of
tests/test_gpu_groups_factors.py and tests/test_gpu_groups_factors_resident.py; then the refusals, each leaving the beliefs
untouched, and the control: every group SET to the world's own sigmas is a world that never heard of the call.

Finiteness of every solo world is asserted as a condition on the inputs, on the solo side alone."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S
from test_gpu_groups_factors import WORLDS, MaskedPair, _equal, _mixed, _untouched, group_scenarios
from test_gpu_groups_schedules import GROUPS, HZ, K, PER_GROUP, SEGMENTS_FORM, SPAWN_GROUP, Pair, _drive, _same_bits, schedules, segments

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("dynamics", "interrobot", "obstacle", "tracking")
WORLD_SIGMAS = dict(dynamics=S.f32w(0.1), interrobot=S.f32w(0.01), obstacle=S.f32w(0.01), tracking=S.f32w(0.01))
SETS = {"A": dict(masks=(15, 15, 15, 7), own=({}, {"tracking": 0.15}, {"tracking": 0.5}, {"dynamics": 0.05})),
        "B": dict(masks=(7, 7, 7, 7), own=({}, {"obstacle": 0.05}, {"interrobot": 0.05}, {"dynamics": 0.05}))}
RESIDENT_FORM, POSTED_FORM = 1, 2      # MGX_SWEEP_FORM_RESIDENT, MGX_SWEEP_FORM_POSTED
MASKED_FORM = 7                        # MGX_SWEEP_F_GROUP_KINDS | MGX_SWEEP_F_TRACKING | MGX_SWEEP_F_UPDATES


def group_sigmas(world, own=None):
    """every group's four sigmas: the world's with the group's own in place, widened from f32 as a config file's are"""
    own = SETS[world]["own"] if own is None else own
    return [dict(WORLD_SIGMAS, **{k: S.f32w(v) for k, v in o.items()}) for o in own]


class SigmaPair(MaskedPair):
    """Pair whose shared world gives every group its sigmas (and its mask, where it has one) before the first robot goes in; the
    groups' own worlds have both from their params.  tell=False: a world that is never told; resident: mgx_set_group_resident
    before the first robot as well"""

    def __init__(self, world="A", own=None, tell=True, resident=False, **kw):
        self.masks = SETS[world]["masks"]
        self.sigmas = group_sigmas(world, own)
        self._masks_pending = False           # (MaskedPair.add: the masks go in below, with the sigmas)
        self._pending, self._resident = tell, resident
        scs = group_scenarios(world, self.masks)
        for sc, s in zip(scs, self.sigmas):
            assert {k: sc["params"]["sigma_" + k] for k in NAMES} == WORLD_SIGMAS, "the scenario's sigmas are the world's"
            sc["params"] = dict(sc["params"], **{"sigma_" + k: v for k, v in s.items()})
        Pair.__init__(self, scs=scs, radius=WORLDS[world]["radius"], **kw)
        if resident:
            # (which form a schedule takes must not hang on how fast the host issues it: the launch waits a long time for the
            # next one, and every schedule is its own post)
            self.shared.set_linger(200000)
            self.shared.set_post_merge(0)

    def add(self, g, i):
        if self._pending:
            self._pending = False
            w = self.shared
            if self._resident:
                w.set_group_resident(True)
            for q in range(self.n):
                assert w.group_sigmas(self.gid[q]) == WORLD_SIGMAS                     # never given any: the world's
                if self.masks[q] != self.masks[0]:
                    w.set_group_enabled(self.gid[q], self.masks[q])
                w.set_group_sigmas(self.gid[q], **self.sigmas[q])
                assert w.group_sigmas(self.gid[q]) == self.sigmas[q] and w.group_enabled(self.gid[q]) == self.masks[q]
        super().add(g, i)

    # (the shared world first, the solo worlds behind a flush: a launch that lingers would hold the other worlds' up)
    def tick_shared(self, steps):
        by_id = {self.ids[g][i]: rb for g in range(self.n) for i, rb in enumerate(self.robots(g))}
        every = {"robots": [by_id[r] for r in sorted(by_id)], "target_speed": self.scs[0]["target_speed"]}
        self.shared.tick(steps=steps, **dict(S.tick_inputs(every, HZ), robots=np.array(sorted(by_id), dtype=np.int32)))

    def tick_alone(self, steps):
        self.shared.flush()
        for g, w in enumerate(self.alone):
            w.tick(steps=steps, **S.tick_inputs({"robots": self.robots(g), "target_speed": self.scs[g]["target_speed"]}, HZ))

    def iterate_alone(self, steps):
        self.shared.flush()
        for w in self.alone:
            w.iterate(steps)

    def set_missions(self):
        dt32 = F(1.0) / F(HZ)
        for g in range(self.n):
            for i, rid in enumerate(self.ids[g]):
                rb = self.robots(g)[i]
                r2, cur = float(F(rb["radius"]) * F(rb["radius"])), rb["mean0"][0]
                self.shared.mission_set(rid, np.asarray([tuple(rb["goal"])], dtype=np.float64), K - 1, 0, r2, r2, (F(cur[0]), F(0.5), F(cur[1])),
                                        float(dt32 / rb["t0"]))
        return dt32

    def mission_tick_begin(self, n):
        tr = np.asarray(self.shared.mission_read()[0], dtype=F).reshape(-1, 3)
        for g, solo in enumerate(self.alone):
            self.nxt_alone[g], c, d = solo.update_topology(tr[self.ids[g]], self.radius, self.nxt_alone[g])
            self.created += c
        self.nxt, stats, fin = self.shared.mission_tick_begin_groups(self.radius, self.nxt, despawn_finished=True)
        assert not len(fin) and [int(x) for x in self.nxt] == self.nxt_alone, (n, fin, self.nxt, self.nxt_alone)


@pytest.mark.parametrize("world", sorted(SETS))
def test_every_group_runs_under_its_own_sigmas(world):
    p = SigmaPair(world, reserve=1)
    w, sch = p.shared, schedules()
    assert w.group_enabled_stats() == (0, 0)
    p.topology()
    assert p.created > 0
    p.check((world, "topology"))
    _equal(p, sch[0], (world, 0, "equal"), as_groups=True)             # a group plan, counted; resident_stats unmoved
    p.prior_changes()
    p.flags(antenna_off=0, idle=1)
    _mixed(p, [sch[0], sch[0], sch[2], sch[3]], (world, 1, "mixed"))   # (groups 0 and 1 alike: what tells them apart is their sigmas)
    p.flags()
    p.topology(far=(2,))
    assert p.deleted > 0
    _equal(p, sch[1], (world, 2, "equal"), as_groups=False)
    assert p.groups_0_and_1_differ(), "their sigmas make the difference"
    # the fine-grained calls: world-wide ones are group plans of one launch, per-robot ones carry their robot's group's sigmas
    p.topology()
    plans0, launches0 = w.group_enabled_stats()
    for q in [w] + p.alone:
        q.sweep(3, 3, 1)
        q.external_factor_iteration()
        q.internal_factor_iteration()
        q.internal_variable_iteration()
    assert w.group_enabled_stats() == (plans0 + 4, launches0 + 4) and w.last_sweep()[2] == SEGMENTS_FORM
    p.check((world, "world-wide fine-grained"))
    for g in range(p.n):
        for world_, r in ((w, p.ids[g][1]), (p.alone[g], 1)):
            world_.internal_factor_iteration(r)
            world_.internal_variable_iteration(r)
            world_.sweep(0, 3, 2, robot=r)
    assert w.group_enabled_stats() == (plans0 + 4, launches0 + 4)
    p.check((world, "per-robot fine-grained"))
    # a robot spawned in place into group 1 after the world has iterated: its dyn_m and its table row are its group's
    appended0, layouts0 = w.append_stats()[0], w.layout_stats()[0]
    p.add(SPAWN_GROUP, PER_GROUP)
    p.prior_changes()
    _mixed(p, [sch[1], sch[2], sch[3], sch[0]], (world, 3, "mixed"))
    assert w.append_stats()[0] == appended0 + 1 and w.layout_stats()[0] == layouts0
    p.topology()                                                       # the newcomer meets its group
    _equal(p, sch[3], (world, 4, "equal"), as_groups=True)
    assert p.groups_0_and_1_differ()
    assert w.resident_stats()[0] == 0 and w.group_resident_stats() == (0, 0, 0)   # never resident: nobody asked
    for solo in p.alone:
        assert solo.group_enabled_stats() == (0, 0)


def test_mission_ticks_under_group_sigmas():
    """mgx_mission_tick_begin_groups / mgx_mission_tick_end on world A: the prior updates go as the kernel of their own, the
    schedule — mixed in the first tick, equal in the second and third — as a group plan.  The solo worlds are driven with
    update_topology and tick."""
    p = SigmaPair("A")
    w, sch = p.shared, schedules()
    dt32 = p.set_missions()
    for n, per_group in enumerate((sch, [sch[0]] * GROUPS, [sch[1]] * GROUPS)):
        p.mission_tick_begin(n)
        before = w.group_enabled_stats(), w.group_schedule_stats()[0]
        w.mission_tick_end(per_group, float(F(p.scs[0]["target_speed"])), float(dt32))
        for g, solo in enumerate(p.alone):
            solo.tick(steps=per_group[g], **S.tick_inputs({"robots": p.robots(g), "target_speed": p.scs[g]["target_speed"]}, HZ))
        most = max(len(segments(s)) for s in per_group)
        assert w.last_launch_count() == most and w.last_sweep()[2] == SEGMENTS_FORM, n
        if n == 0:
            assert (w.group_enabled_stats(), w.group_schedule_stats()[0]) == (before[0], before[1] + 1)
        else:
            assert (w.group_enabled_stats(), w.group_schedule_stats()[0]) == ((before[0][0] + 1, before[0][1] + most), before[1])
        p.check(("mission tick", n))
    assert p.created > 0
    assert p.groups_0_and_1_differ()
    assert w.resident_stats()[0] == 0


def _ran_masked(w, what, form):
    """one launch of the run-time-K kernel's masked form (or one post into it), messages staged in LDS"""
    assert w.last_launch_count() == 1, (what, w.last_launch_count())
    assert w.last_sweep()[:3] == (0, 2, form), (what, w.last_sweep())
    assert w.last_sweep_features() == MASKED_FORM, (what, w.last_sweep_features())


@pytest.mark.parametrize("world", sorted(SETS))
def test_equal_schedules_run_resident_under_group_sigmas(world):
    p = SigmaPair(world, resident=True)
    w, sch = p.shared, schedules()
    assert w.group_resident_stats() == (0, 0, 0) and w.group_enabled_stats() == (0, 0)
    p.topology()
    assert p.created > 0
    # one equal schedule is one resident launch of the masked form, a second one right behind it a post into it
    res0 = w.resident_stats()[0]
    w.iterate([sch[0]] * p.n)
    _ran_masked(w, (world, "launch"), RESIDENT_FORM)
    assert w.resident_stats()[0] == res0 + 1 and w.group_resident_stats() == (1, 0, 0)
    w.iterate(sch[1])
    _ran_masked(w, (world, "post"), POSTED_FORM)
    assert w.group_resident_stats() == (1, 1, 0) and w.linger_stats()[1] == 1
    p.iterate_alone(sch[0])
    p.iterate_alone(sch[1])
    p.check((world, "launch + post"))
    assert w.linger_stats()[2] == 0                                    # (the post was taken, not taken back)
    # a tick — the prior updates ride — is one launch, and the tick behind it one post
    p.tick_shared(sch[3])
    _ran_masked(w, (world, "tick, launch"), RESIDENT_FORM)
    p.tick_shared(sch[0])
    _ran_masked(w, (world, "tick, post"), POSTED_FORM)
    assert w.group_resident_stats() == (2, 2, 0) and w.group_enabled_stats() == (0, 0)
    p.tick_alone(sch[3])
    p.tick_alone(sch[0])
    p.check((world, "ticks"))
    assert p.groups_0_and_1_differ(), "their sigmas make the difference"
    # a mixed call stays a group plan
    calls0, launches0, _ = w.group_schedule_stats()
    per_group = [sch[0], sch[0], sch[2], sch[3]]
    w.iterate(per_group)
    most = max(len(segments(x)) for x in per_group)
    assert w.last_launch_count() == most and w.last_sweep()[2] == SEGMENTS_FORM
    assert w.group_schedule_stats()[:2] == (calls0 + 1, launches0 + most) and w.group_enabled_stats() == (0, 0)
    for g, solo in enumerate(p.alone):
        solo.iterate(per_group[g])
    p.check((world, "mixed"))
    for solo in p.alone:
        assert solo.group_resident_stats() == (0, 0, 0)


def test_mission_ticks_run_resident_under_group_sigmas():
    """equal schedules on world A with the switch on: the prior updates ride, each tick is ONE launch of the masked form — a
    group plan only while no connection exists"""
    p = SigmaPair("A", resident=True)
    w, sch = p.shared, schedules()
    dt32 = p.set_missions()
    resident = 0
    for n, steps in enumerate((sch[0], sch[3], sch[1])):
        p.mission_tick_begin(n)
        connected = p.created > 0                                      # (nobody moves out of range in three ticks)
        before = w.group_resident_stats(), w.group_enabled_stats()
        w.mission_tick_end([steps] * GROUPS if n % 2 == 0 else steps, float(F(p.scs[0]["target_speed"])), float(dt32))
        if connected:
            _ran_masked(w, ("mission tick", n), RESIDENT_FORM)
            assert (w.group_resident_stats(), w.group_enabled_stats()) == ((before[0][0] + 1, before[0][1], before[0][2]), before[1]), n
            resident += 1
        else:
            assert w.last_sweep()[2] == SEGMENTS_FORM and w.group_enabled_stats()[0] == before[1][0] + 1, n
            assert w.group_resident_stats() == (before[0][0], before[0][1], before[0][2] + 1), n
        p.tick_alone(steps)
        p.check(("mission tick", n))
    assert p.created > 0 and resident >= 2
    assert p.groups_0_and_1_differ()


def test_refusals_leave_the_world_as_it_was():
    p = SigmaPair("A")
    p.topology()
    p.iterate(schedules())
    w = p.shared
    before = w.read_beliefs()
    stats = w.group_enabled_stats(), w.group_schedule_stats(), w.group_resident_stats()
    with pytest.raises(hostlib.MgxError, match="fixed before its first robot"):          # a group that has robots (group 0 like any other)
        w.set_group_sigmas(0, tracking=0.2)
    with pytest.raises(hostlib.MgxError, match="fixed before its first robot"):
        w.set_group_sigmas(1, **WORLD_SIGMAS)
    for name in NAMES:                                                                   # a group without robots, bad values
        for bad in (0.0, -0.01, float("nan"), float("inf")):
            with pytest.raises(hostlib.MgxError, match="finite and positive"):
                w.set_group_sigmas(GROUPS, **{name: bad})
    with pytest.raises(hostlib.MgxError, match="MGX_GROUPS_MAX"):
        w.set_group_sigmas(hostlib.GROUPS_MAX, **WORLD_SIGMAS)
    with pytest.raises(hostlib.MgxError, match="mgx_set_group_sigmas"):                   # freeze and thaw stay world-wide
        w.set_enabled(7)
    w.set_enabled(15)                                                                    # (the world's own mask: nothing to do)
    with pytest.raises(hostlib.MgxError, match="mgx_mission_run"):
        w.mission_run(2, p.radius, 1, schedules()[0], 1.0, 0.1)
    assert [w.group_sigmas(g) for g in range(GROUPS + 1)] == p.sigmas + [WORLD_SIGMAS]
    _untouched(w, before, "refusals on a world with sigmas per group")
    assert (w.group_enabled_stats(), w.group_schedule_stats(), w.group_resident_stats()) == stats
    w.set_group_sigmas(GROUPS, obstacle=S.f32w(0.02))                                    # a group still without robots takes sigmas,
    assert w.group_sigmas(GROUPS) == dict(WORLD_SIGMAS, obstacle=S.f32w(0.02))
    w.set_group_sigmas(GROUPS, **WORLD_SIGMAS)                                           # ... and gives them back
    assert w.group_sigmas(GROUPS) == WORLD_SIGMAS
    p.iterate(schedules())
    p.check("behind the refusals")
    # a world that has switched a kind at run time takes no sigmas: the thaw kernels evaluate factors with the world's
    q = Pair()
    q.topology()
    q.iterate(schedules())
    q.shared.set_enabled(S.EN_DYN | S.EN_OBS | S.EN_IR)
    before = q.shared.read_beliefs()
    with pytest.raises(hostlib.MgxError, match="mgx_set_enabled"):
        q.shared.set_group_sigmas(GROUPS, tracking=0.5)
    assert q.shared.group_sigmas(GROUPS) == WORLD_SIGMAS
    _untouched(q.shared, before, "set_group_sigmas behind set_enabled")
    # ... and neither does a world with a ghost
    sc = group_scenarios("A")[0]
    g = World(sc["params"])
    g.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    for i, rb in enumerate(sc["robots"][:3]):
        g.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=i, ghost=(i == 2))
    with pytest.raises(hostlib.MgxError, match="ghosts"):
        g.set_group_sigmas(3, tracking=0.5)


def test_every_group_at_the_worlds_sigmas_is_a_world_never_told():
    """the control: every group SET to the world's own sigmas makes the launches, the last_sweep answers and the stats of a world
    that never heard of the call — resident launches and posts included"""
    same = ({},) * GROUPS
    a, b = SigmaPair("B", own=same), SigmaPair("B", own=same, tell=False)
    for q in (a, b):
        q.topology()
    sch = schedules()
    ran_a, bel_a, res_a, linger_a, mixed_a = _drive(a.shared, [sch[0]] * GROUPS)
    ran_b, bel_b, res_b, linger_b, mixed_b = _drive(b.shared, [sch[0]] * GROUPS)
    assert ran_a == ran_b and _same_bits(bel_a, bel_b)
    assert res_a == res_b and res_a[0] >= 1 and linger_a == linger_b and mixed_a == mixed_b == (0, 0, 0)
    assert a.shared.last_sweep_features() == b.shared.last_sweep_features() and not a.shared.last_sweep_features() & 4
    for q in (a, b):
        q.prior_changes()
        q.iterate(sch)
    assert (a.shared.last_launch_count(), a.shared.last_sweep()) == (b.shared.last_launch_count(), b.shared.last_sweep())
    assert a.shared.group_schedule_stats() == b.shared.group_schedule_stats() and a.shared.group_schedule_stats()[0] == 1
    assert _same_bits(a.shared.read_beliefs(), b.shared.read_beliefs())
    assert a.shared.group_enabled_stats() == b.shared.group_enabled_stats() == (0, 0)
    assert a.shared.group_resident_stats() == b.shared.group_resident_stats() == (0, 0, 0)
    a.shared.set_enabled(3)                                            # ... and freeze and thaw are still its own
    assert a.shared.group_enabled(0) == 3
