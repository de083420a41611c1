"""Resident and lingering launches on a MASKED world (include/mgx.h, ROBOT GROUPS: mgx_set_group_resident): worlds A and B of
tests/test_gpu_groups_factors.py — 4 groups x 3 robots, K = 8 (the run-time-K kernel's masked form), every group with its own
gbp.factors-enabled, groups 0 and 1 the same robots under different masks — with the switch on before the first robot.

Equal schedules, ticks and mission ticks have to run as ONE resident launch of the masked form (mgx_last_sweep_features: 7) or as
one post into it, and every group's beliefs (as bit patterns), message counts and connections have to be those of the group's own
world, created with that mask and driven with the plain calls.  Mixed schedules stay group plans.  Every fall-back — a tick before
any connection exists, resident launches switched off — sends the riding prior updates once and runs as ONE group plan.

The shared world is driven first and read afterwards: worlds share the stream, and a launch that lingers holds up whatever another
world puts behind it (the first read of the shared world ends the launch).

Controls: with the switch off the same script takes the counts tests/test_gpu_groups_factors.py pins; with the switch on and
every group at the world's mask the world is an unmasked world.

Finiteness of every solo world is asserted as a condition on the inputs."""
import numpy as np
import pytest

from magics_amd import hostlib, scenarios as S
from test_gpu_groups_factors import WORLDS, MaskedPair, _equal
from test_gpu_groups_schedules import GROUPS, HZ, K, PER_GROUP, SEGMENTS_FORM, SPAWN_GROUP, _drive, _same_bits, schedules, segments

pytestmark = pytest.mark.gpu

F = np.float32
RESIDENT_FORM, POSTED_FORM = 1, 2      # MGX_SWEEP_FORM_RESIDENT, MGX_SWEEP_FORM_POSTED
MASKED_FORM = 7                        # MGX_SWEEP_F_GROUP_KINDS | MGX_SWEEP_F_TRACKING | MGX_SWEEP_F_UPDATES
MAX_SEGS = 32                          # segments of one resident launch (mgx_dev.h)


class ResidentPair(MaskedPair):
    """MaskedPair whose shared world is told mgx_set_group_resident before its first robot (knob=False: never told)"""

    def __init__(self, world="A", knob=True, **kw):
        self.knob = knob
        super().__init__(world, **kw)
        # (which form a schedule takes must not hang on how fast the host issues it: the launch waits a long time for the next
        # one, and every schedule is its own post)
        self.shared.set_linger(200000)
        self.shared.set_post_merge(0)

    def add(self, g, i):
        if self.knob:
            self.knob = False
            self.shared.set_group_resident(True)
        super().add(g, i)

    def tick_shared(self, steps):
        by_id = {self.ids[g][i]: rb for g in range(self.n) for i, rb in enumerate(self.robots(g))}
        every = {"robots": [by_id[r] for r in sorted(by_id)], "target_speed": self.scs[0]["target_speed"]}
        self.shared.tick(steps=steps, **dict(S.tick_inputs(every, HZ), robots=np.array(sorted(by_id), dtype=np.int32)))

    def tick_alone(self, steps):
        self.shared.flush()                                            # (a launch that lingers would hold the other worlds' up)
        for g, w in enumerate(self.alone):
            w.tick(steps=steps, **S.tick_inputs({"robots": self.robots(g), "target_speed": self.scs[g]["target_speed"]}, HZ))

    def iterate_alone(self, steps):
        self.shared.flush()
        for w in self.alone:
            w.iterate(steps)


def _ran_resident(w, what, forms=(RESIDENT_FORM,), launches=1):
    assert w.last_launch_count() == launches, (what, w.last_launch_count())
    variant, ir_mode, form, _ = w.last_sweep()
    assert (variant, ir_mode) == (0, 2) and form in forms, (what, w.last_sweep())   # the run-time-K kernel, messages staged in LDS
    assert w.last_sweep_features() == MASKED_FORM, (what, w.last_sweep_features())


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_equal_schedules_run_resident_on_a_masked_world(world):
    p = ResidentPair(world, reserve=1)
    w, sch = p.shared, schedules()
    assert w.group_resident_stats() == (0, 0, 0) and w.group_enabled_stats() == (0, 0)
    p.topology()
    assert p.created > 0
    # 1: one equal schedule is one resident launch of the masked form
    res0 = w.resident_stats()[0]
    w.iterate([sch[0]] * p.n)
    _ran_resident(w, (world, 1))
    assert w.resident_stats()[0] == res0 + 1 and w.group_enabled_stats() == (0, 0)
    assert w.group_resident_stats() == (1, 0, 0)
    # 2: a second one right behind it is posted into the launch that lingers
    w.iterate(sch[1])
    _ran_resident(w, (world, 2), forms=(POSTED_FORM,))
    assert w.group_resident_stats() == (1, 1, 0) and w.linger_stats()[1] == 1
    p.iterate_alone(sch[0])
    p.iterate_alone(sch[1])
    p.check((world, "launch + post"))
    assert p.groups_0_and_1_differ(), "their masks make the difference"
    assert w.linger_stats()[2] == 0                                    # (the post was taken, not taken back)
    # 3: a tick — the prior updates ride — is one launch, and the tick behind it one post
    p.tick_shared(sch[3])
    _ran_resident(w, (world, 3, "launch"))
    p.tick_shared(sch[0])
    _ran_resident(w, (world, 3, "post"), forms=(POSTED_FORM,))
    assert w.group_resident_stats() == (2, 2, 0) and w.group_enabled_stats() == (0, 0)
    p.tick_alone(sch[3])
    p.tick_alone(sch[0])
    p.check((world, "ticks"))
    # 4: more segments than one launch holds: parts
    long = [hostlib.STEP_EXTERNAL, hostlib.STEP_INTERNAL] * (MAX_SEGS + 3)
    assert len(segments(long)) == MAX_SEGS + 3
    w.iterate(long)
    _ran_resident(w, (world, 4), launches=2)
    assert w.group_resident_stats() == (4, 2, 0)
    p.iterate_alone(long)
    p.check((world, "parts"))
    # 5: a mixed call behind a launch that lingers: the launch is ended, the call is a group plan
    p.flags(antenna_off=0, idle=1)
    calls0, launches0, _ = w.group_schedule_stats()
    w.iterate(sch[2])
    _ran_resident(w, (world, 5))
    per_group = [sch[0], sch[0], sch[2], sch[3]]                       # (groups 0 and 1 alike: what tells them apart is their masks)
    w.iterate(per_group)
    most = max(len(segments(x)) for x in per_group)
    assert w.last_launch_count() == most and w.last_sweep()[2] == SEGMENTS_FORM, (world, 5, w.last_sweep())
    assert w.group_schedule_stats()[:2] == (calls0 + 1, launches0 + most)
    assert w.group_resident_stats() == (5, 2, 0) and w.group_enabled_stats() == (0, 0)
    p.iterate_alone(sch[2])
    for g, solo in enumerate(p.alone):
        solo.iterate(per_group[g])
    p.check((world, "mixed behind a lingering launch"))
    # 6: a robot spawned in place into the group whose mask lacks a kind: a new launch, and a table that is still right
    p.flags()
    p.topology(far=(2,))
    assert p.deleted > 0
    p.add(SPAWN_GROUP, PER_GROUP)
    p.topology()                                                       # the newcomer meets its group
    p.prior_changes()
    w.iterate([sch[1]] * p.n)
    _ran_resident(w, (world, 6))
    assert w.append_stats()[0] >= 1                                    # the spawn went in place
    assert w.group_resident_stats() == (6, 2, 0)
    p.iterate_alone(sch[1])
    p.check((world, "spawn"))
    assert p.groups_0_and_1_differ()
    assert w.group_enabled_stats() == (0, 0)                           # no schedule ran as a group plan because of the masks
    for solo in p.alone:
        assert solo.group_resident_stats() == (0, 0, 0)


def test_mission_ticks_run_resident_on_a_masked_world():
    """mgx_mission_tick_begin_groups / mgx_mission_tick_end with equal schedules on world A (the pattern of
    test_mission_ticks_on_a_masked_world): the prior updates ride, each tick is ONE launch — a group plan only while no connection
    exists.  The solo worlds are driven with update_topology and tick."""
    p = ResidentPair("A")
    w, sch = p.shared, schedules()
    dt32 = F(1.0) / F(HZ)
    for g in range(p.n):
        for i, rid in enumerate(p.ids[g]):
            rb = p.robots(g)[i]
            r2, cur = float(F(rb["radius"]) * F(rb["radius"])), rb["mean0"][0]
            w.mission_set(rid, np.asarray([tuple(rb["goal"])], dtype=np.float64), K - 1, 0, r2, r2, (F(cur[0]), F(0.5), F(cur[1])), float(dt32 / rb["t0"]))
    resident = 0
    for n, steps in enumerate((sch[0], sch[3], sch[1])):
        tr = np.asarray(w.mission_read()[0], dtype=F).reshape(-1, 3)
        for g, solo in enumerate(p.alone):
            p.nxt_alone[g], c, d = solo.update_topology(tr[p.ids[g]], p.radius, p.nxt_alone[g])
            p.created += c
        p.nxt, stats, fin = w.mission_tick_begin_groups(p.radius, p.nxt, despawn_finished=True)
        assert not len(fin) and [int(x) for x in p.nxt] == p.nxt_alone, (n, fin, p.nxt, p.nxt_alone)
        connected = p.created > 0                                      # (nobody moves out of range in three ticks)
        before = w.group_resident_stats(), w.group_enabled_stats()
        w.mission_tick_end([steps] * GROUPS if n % 2 == 0 else steps, float(F(p.scs[0]["target_speed"])), float(dt32))
        if connected:
            _ran_resident(w, ("mission tick", n))
            assert (w.group_resident_stats(), w.group_enabled_stats()) == ((before[0][0] + 1, before[0][1], before[0][2]), before[1]), n
            resident += 1
        else:
            assert w.last_sweep()[2] == SEGMENTS_FORM and w.group_enabled_stats()[0] == before[1][0] + 1, n
            assert w.group_resident_stats() == (before[0][0], before[0][1], before[0][2] + 1), n
        p.tick_alone(steps)
        p.check(("mission tick", n))
    assert p.created > 0 and resident >= 2
    assert p.groups_0_and_1_differ()


def test_a_tick_before_any_connection_falls_back_with_its_updates():
    """no connection yet: the world cannot launch resident now, the tick's prior updates — riding — go as the kernel of their own,
    once, and the schedule is ONE group plan"""
    p = ResidentPair("A")
    w, steps = p.shared, schedules()[0]
    p.tick_shared(steps)
    n = len(segments(steps))
    assert w.last_launch_count() == n and w.last_sweep()[2] == SEGMENTS_FORM, w.last_sweep()
    assert w.group_resident_stats() == (0, 0, 1) and w.group_enabled_stats() == (1, n) and w.resident_stats()[0] == 0
    p.tick_alone(steps)
    p.check("tick without connections")
    # ... and once they exist the next tick is a launch
    p.topology()
    assert p.created > 0
    p.tick_shared(steps)
    _ran_resident(w, "tick with connections")
    assert w.group_resident_stats() == (1, 0, 1) and w.group_enabled_stats() == (1, n)
    p.tick_alone(steps)
    p.check("tick with connections")
    assert p.groups_0_and_1_differ()


def test_resident_launches_off_falls_back_to_one_group_plan():
    p = ResidentPair("B")
    w, sch = p.shared, schedules()
    p.topology()
    assert p.created > 0
    w.set_resident_launches(False)
    for k, steps in enumerate((sch[0], sch[1])):
        w.iterate([steps] * p.n)
        n = len(segments(steps))
        assert w.last_launch_count() == n and w.last_sweep()[2] == SEGMENTS_FORM, (k, w.last_sweep())
        assert w.group_resident_stats() == (0, 0, k + 1) and w.group_enabled_stats()[0] == k + 1 and w.resident_stats()[0] == 0
        p.iterate_alone(steps)
        p.check(("resident launches off", k))
    p.tick_shared(sch[3])                                              # (updates riding into the fall-back)
    assert w.last_sweep()[2] == SEGMENTS_FORM and w.group_resident_stats() == (0, 0, 3) and w.group_enabled_stats()[0] == 3
    p.tick_alone(sch[3])
    p.check("resident launches off, tick")
    w.set_resident_launches(True)
    w.iterate(sch[0])
    _ran_resident(w, "resident launches on again")
    assert w.group_resident_stats() == (1, 0, 3)
    p.iterate_alone(sch[0])
    p.check("resident launches on again")
    assert p.groups_0_and_1_differ()


def test_with_the_switch_off_nothing_changes():
    """the control: the same world never told (and one told and untold again) takes the counts of test_gpu_groups_factors.py"""
    for told in (False, True):
        p = ResidentPair("A", knob=told)
        if told:
            p.shared.set_group_resident(False)
        sch = schedules()
        p.topology()
        _equal(p, sch[0], ("switch off", told, "equal"), as_groups=True)
        _equal(p, sch[1], ("switch off", told, "equal again"), as_groups=False)
        plans0, launches0 = p.shared.group_enabled_stats()
        p.tick_shared(sch[3])                                          # (the updates as the kernel of their own, the schedule a group plan)
        assert p.shared.last_sweep()[2] == SEGMENTS_FORM
        assert p.shared.group_enabled_stats() == (plans0 + 1, launches0 + len(segments(sch[3])))
        p.tick_alone(sch[3])
        p.check(("switch off", told, "tick"))
        assert p.shared.group_resident_stats() == (0, 0, 0) and p.shared.resident_stats()[0] == 0


def test_the_switch_on_an_unmasked_world_does_nothing():
    """every group at the world's mask, the switch on: the launches, forms and stats of a world that never heard of either call"""
    same = (15,) * GROUPS
    a, b = ResidentPair("A", masks=same), MaskedPair("A", masks=same, set_masks=False)
    for q in (a, b):
        q.topology()
    sch = schedules()
    ran_a, bel_a, res_a, linger_a, mixed_a = _drive(a.shared, [sch[0]] * GROUPS)
    ran_b, bel_b, res_b, linger_b, mixed_b = _drive(b.shared, [sch[0]] * GROUPS)
    assert ran_a == ran_b and _same_bits(bel_a, bel_b)
    assert res_a == res_b and res_a[0] >= 1 and linger_a == linger_b and mixed_a == mixed_b == (0, 0, 0)
    a.shared.iterate(sch[1])
    a.shared.flush()
    b.shared.iterate(sch[1])
    assert a.shared.last_sweep() == b.shared.last_sweep() and a.shared.last_sweep()[2] == RESIDENT_FORM
    assert a.shared.last_sweep_features() == b.shared.last_sweep_features() and not a.shared.last_sweep_features() & 4
    assert _same_bits(a.shared.read_beliefs(), b.shared.read_beliefs())
    assert a.shared.group_resident_stats() == (0, 0, 0) and a.shared.group_enabled_stats() == (0, 0)
