"""One GBP iteration schedule per robot GROUP (include/mgx.h, ROBOT GROUPS: mgx_iterate_groups): a world of 4 groups x 3 robots,
K = 8 (the smallest horizon the group tests use), the robots of a group within comms range, inter-robot and tracking factors on,
every group driven with its OWN schedule — against four worlds of their own, each holding one group's robots and driven with plain
iterate.  After every round each group's beliefs (as bit patterns), message counts and connections have to be the solo world's.

The schedules: interleave-evenly 3 / 3; internal 5 / external 2; internal 1 / external 4 — more external than internal iterations,
so some of its segments are an external iteration ALONE in launches that write snapshots for the other groups (the robot has to end
with its unchanged record in the launch's output buffer); late-as-possible 2 / 2; and, in two rounds, one group with no schedule at
all.  Between the rounds: prior changes, one antenna off and one idle robot per group, connections made and broken by
update_topology_groups, a robot spawned in place into one group.

Groups 0 and 1 hold the SAME robots (one scenario, one seed): that they end with different beliefs is what their different schedules
do, so the comparison cannot pass with the schedules ignored.

Same file: equal schedules ARE the plain call (same beliefs, same launches, no mixed call counted), and the two refusals of a mixed
schedule — a sharded world, a world that has switched a factor kind — leave the beliefs untouched."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S

pytestmark = pytest.mark.gpu

GROUPS, PER_GROUP, K, RADIUS, HZ = 4, 3, 8, 12.0, 10.0
SEEDS = (805, 805, 806, 807)          # (groups 0 and 1: the same robots)
SPAWN_GROUP = 1
F = np.float32
I, E = hostlib.STEP_INTERNAL, hostlib.STEP_EXTERNAL
SEGMENTS_FORM = 0                      # MGX_SWEEP_FORM_SEGMENTS


def schedules():
    s = [hostlib.schedule(hostlib.SCHEDULE_INTERLEAVE_EVENLY, 3, 3), hostlib.schedule(hostlib.SCHEDULE_INTERLEAVE_EVENLY, 5, 2),
         hostlib.schedule(hostlib.SCHEDULE_INTERLEAVE_EVENLY, 1, 4), hostlib.schedule(hostlib.SCHEDULE_LATE_AS_POSSIBLE, 2, 2)]
    assert len({tuple(x) for x in s}) == GROUPS
    return s


def segments(steps):
    """the [external] internal* segments of a schedule as (external?, internal iterations) — plan_launches, restated"""
    phases = [p for s in steps for p in (("I",) if s & I else ()) + (("E",) if s & E else ())]
    out, i = [], 0
    while i < len(phases):
        ext = phases[i] == "E"
        i += 1 if ext else 0
        n = 0
        while i < len(phases) and phases[i] == "I":
            n, i = n + 1, i + 1
        out.append((ext, n))
    return out


def scenario_of(g):
    """group g's robots: a grid scenario of PER_GROUP + 1 (the last one is the robot that may be spawned later)"""
    added = K not in S.HORIZON_FOR_K     # (the table of horizons has no entry for 8 variables: one for the time being, as other tests do)
    if added:
        S.HORIZON_FOR_K[K] = next(h for h in range(1, 200) if len(hostlib.variable_timesteps(h, 3)) == K)
    try:
        return S.grid_scenario(PER_GROUP + 1, K, interrobot=True, comm_radius=RADIUS, obstacles=False, seed=SEEDS[g], pitch=4.0, tracking=True)
    finally:
        if added:
            del S.HORIZON_FOR_K[K]


class Pair:
    """the shared world and the groups' own worlds, driven alike; ids[g][i]: the shared world's id of robot i of group g.

    The defaults are this file's world.  scs: one scenario per group (its last robot is held back for a spawn where sizes[g] leaves
    it out); sizes: robots per group; alone: what makes a group's own world from the scenario's params (tests/
    test_gpu_groups_kernel_matrix.py hands in the CPU oracle); radius: the comms radius of topology(); group_ids: the shared
    world's group id of every group here, n_groups: how many groups the per-group calls name (the ones in between hold no robot)"""

    def __init__(self, reserve=0, scs=None, sizes=None, alone=World, radius=RADIUS, spawn_group=SPAWN_GROUP, group_ids=None, n_groups=None):
        self.scs = scs if scs is not None else [scenario_of(g) for g in range(GROUPS)]
        self.n, self.K, self.radius = len(self.scs), self.scs[0]["K"], radius
        self.sizes = list(sizes) if sizes is not None else [PER_GROUP] * self.n
        self.gid = list(group_ids) if group_ids is not None else list(range(self.n))
        self.n_groups = n_groups if n_groups is not None else max(self.gid) + 1
        sdf = self.scs[0]["sdf"]
        self.shared, self.alone = World(self.scs[0]["params"]), [alone(sc["params"]) for sc in self.scs]
        for w in [self.shared] + self.alone:
            w.set_sdf(sdf["rgb"], sdf["world_w"], sdf["world_h"])
        if reserve:
            self.shared.reserve(sum(self.sizes) + reserve)
            if hasattr(self.alone[spawn_group], "reserve"):
                self.alone[spawn_group].reserve(self.sizes[spawn_group] + reserve)
        self.ids = [[] for _ in range(self.n)]
        self.gone = set()                     # (g, i) of the robots that have been removed
        self.key = 0
        for i in range(max(self.sizes)):      # ids interleaved across the groups
            for g in range(self.n):
                if i < self.sizes[g]:
                    self.add(g, i)
        self.nxt, self.nxt_alone = np.ones(self.n_groups, np.uint64), [1] * self.n
        self.created = self.deleted = 0

    def add(self, g, i):
        rb = self.scs[g]["robots"][i]
        self.ids[g].append(self.shared.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=self.key, group=self.gid[g]))
        assert self.alone[g].add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=self.key) == i
        self.key += 1

    def robots(self, g):
        return self.scs[g]["robots"][:len(self.ids[g])]

    def topology(self, far=()):
        """one pass over the robots' start positions; robot i of every group with i in `far` is out of everybody's range"""
        n = sum(len(x) for x in self.ids)
        pos_shared = np.zeros((n, 3), dtype=F)
        for g in range(self.n):
            pos = np.array([[rb["pos"][0] + (5000.0 * (i + 1) if i in far else 0.0), 0.5, rb["pos"][1]] for i, rb in enumerate(self.robots(g))], dtype=F)
            pos_shared[self.ids[g]] = pos
            self.nxt_alone[g], c, d = self.alone[g].update_topology(pos, self.radius, self.nxt_alone[g])
            self.created, self.deleted = self.created + c, self.deleted + d
        self.nxt, stats = self.shared.update_topology_groups(pos_shared, self.radius, self.nxt)
        assert [int(self.nxt[q]) for q in self.gid] == self.nxt_alone

    def prior_changes(self):
        by_id = {self.ids[g][i]: rb for g in range(self.n) for i, rb in enumerate(self.robots(g)) if (g, i) not in self.gone}
        every = {"robots": [by_id[r] for r in sorted(by_id)], "target_speed": self.scs[0]["target_speed"]}
        self.shared.update_priors(**dict(S.tick_inputs(every, HZ), robots=np.array(sorted(by_id), dtype=np.int32)))
        for g, w in enumerate(self.alone):
            live = [i for i in range(len(self.ids[g])) if (g, i) not in self.gone]
            if live:
                w.update_priors(**dict(S.tick_inputs({"robots": [self.robots(g)[i] for i in live], "target_speed": self.scs[g]["target_speed"]}, HZ),
                                       robots=np.array(live, dtype=np.int32)))

    def flags(self, antenna_off=None, idle=None):
        for g, w in enumerate(self.alone):
            for i, rid in enumerate(self.ids[g]):
                if (g, i) in self.gone:
                    continue
                for world, r in ((self.shared, rid), (w, i)):
                    world.set_antenna(r, i != antenna_off)
                    world.set_idle(r, i == idle)

    def per_group_of_world(self, per_group):
        """one schedule per group of the SHARED world: the groups here by their group id there, an empty one for every other id"""
        if self.gid == list(range(self.n_groups)):
            return per_group
        out = [[] for _ in range(self.n_groups)]
        for g, steps in enumerate(per_group):
            out[self.gid[g]] = steps
        return out

    def iterate(self, per_group):
        self.shared.iterate(self.per_group_of_world(per_group))
        for g, w in enumerate(self.alone):
            if len(per_group[g]) and len(self.gone & {(g, i) for i in range(len(self.ids[g]))}) < len(self.ids[g]):
                w.iterate(per_group[g])

    def beliefs(self):
        n = sum(len(x) for x in self.ids)
        return [a.reshape((n, self.K) + a.shape[1:]) for a in self.shared.read_beliefs()]

    def same(self, what):
        bs = self.beliefs()
        for g, w in enumerate(self.alone):
            sel = np.array(self.ids[g])
            for name, a, b in zip(("eta", "lam", "mean"), bs, w.read_beliefs()):
                b = b.reshape((len(sel), self.K) + b.shape[1:])
                assert np.array_equal(a[sel].view(np.uint64), b.view(np.uint64)), (what, g, name)
            for i, rid in enumerate(self.ids[g]):
                if (g, i) in self.gone:
                    continue
                assert self.shared.message_counts(rid) == w.message_counts(i), (what, g, i)
                assert self.shared.connections(rid) == [self.ids[g][j] for j in w.connections(i)], (what, g, i)


def test_every_group_runs_its_own_schedule():
    p = Pair(reserve=1)
    sch = schedules()
    counts = [len(segments(s)) for s in sch]
    assert any(ext and n == 0 for ext, n in segments(sch[2])[:-1]), "internal 1 / external 4 has external-only segments in front of its last"
    assert len(set(counts)) > 1, "ragged segment counts"
    launches = sat_floor = 0
    rounds = [                                                     # (what happens in front of the round's schedules, who runs what)
        (lambda: p.topology(), sch),
        (lambda: (p.prior_changes(), p.flags(antenna_off=0, idle=1)), sch),
        (lambda: (p.flags(), p.topology(far=(2,))), sch[:3] + [[]]),                       # group 3 sits the call out
        (lambda: (p.topology(), p.add(SPAWN_GROUP, PER_GROUP), p.prior_changes()), [sch[1], sch[2], sch[3], sch[0]]),
        (lambda: (p.topology(), p.flags(antenna_off=2)), [[], sch[0], sch[2], sch[2]]),    # group 0 sits out; two groups alike, two not
        (lambda: p.prior_changes(), sch),
    ]
    for n, (before, per_group) in enumerate(rounds):
        before()
        p.iterate(per_group)
        most = max(len(segments(s)) for s in per_group)
        assert p.shared.last_launch_count() == most, n
        assert p.shared.last_sweep()[2] == SEGMENTS_FORM, n
        launches += most
        sat_floor += sum(len(p.ids[g]) * (most - len(segments(s))) for g, s in enumerate(per_group))
        p.same(n)
        if n == 0:    # the same robots under two schedules: not the same beliefs
            means = p.beliefs()[2]
            assert not np.array_equal(means[p.ids[0]], means[p.ids[1]])
            assert np.isfinite(means).all()
    assert p.created > 0 and p.deleted > 0                          # connections came and went
    assert p.shared.append_stats()[0] >= 1                          # the spawn went in place
    calls, mixed_launches, sat_out = p.shared.group_schedule_stats()
    assert (calls, mixed_launches) == (len(rounds), launches)
    assert sat_out == sat_floor > 0
    for w in p.alone:
        assert w.group_schedule_stats() == (0, 0, 0)


def _drive(world, schedule, rounds=3):
    """`rounds` schedules back to back (a launch, then posts into the launch that lingers), then the reads that end it: how each
    ran, the beliefs, the launches' counters.  One world at a time — worlds share the stream, and a launch that lingers holds up
    whatever another world puts behind it"""
    # (which form a schedule takes must not hang on how fast the host issues it: the launch waits a long time for the next one,
    # and every schedule is its own post)
    world.set_linger(200000)
    world.set_post_merge(0)
    ran = []
    for _ in range(rounds):
        world.iterate(schedule)
        ran.append((world.last_launch_count(), world.last_sweep()))
    return ran, world.read_beliefs(), world.resident_stats(), world.linger_stats(), world.group_schedule_stats()


def _same_bits(xs, ys):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(xs, ys))


def test_equal_schedules_are_the_plain_call():
    a, b = Pair(), Pair()
    for q in (a, b):
        q.topology()
    steps = schedules()[0]
    ran_a, bel_a, res_a, linger_a, mixed_a = _drive(a.shared, [steps] * GROUPS)
    ran_b, bel_b, res_b, linger_b, _ = _drive(b.shared, steps)
    assert ran_a == ran_b and _same_bits(bel_a, bel_b)
    assert res_a == res_b and linger_a == linger_b
    assert mixed_a == (0, 0, 0)
    # only the groups that hold live robots count: an empty group's steps do not make the call mixed
    ran_a, bel_a, *_, mixed_a = _drive(a.shared, [steps] * GROUPS + [[I, E, I]], rounds=1)
    ran_b, bel_b, *_ = _drive(b.shared, steps, rounds=1)
    assert ran_a == ran_b and _same_bits(bel_a, bel_b) and mixed_a == (0, 0, 0)
    # ... and an ungrouped world: one group
    ran_a, bel_a, res_a, linger_a, mixed_a = _drive(a.alone[0], [steps])
    ran_b, bel_b, res_b, linger_b, _ = _drive(b.alone[0], steps)
    assert ran_a == ran_b and _same_bits(bel_a, bel_b)
    assert res_a == res_b and linger_a == linger_b and mixed_a == (0, 0, 0)


def test_mixed_schedules_are_refused_where_they_cannot_run():
    sch = schedules()
    # a sharded world (one ghost): ghosts have no group
    sc = scenario_of(0)
    w = World(sc["params"])
    w.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    for i, rb in enumerate(sc["robots"][:3]):
        w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=i, ghost=(i == 2))
    before = w.read_beliefs()
    with pytest.raises(hostlib.MgxError, match="sharded"):
        w.iterate([sch[0], sch[1]])
    for x, y in zip(before, w.read_beliefs()):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert w.group_schedule_stats() == (0, 0, 0)
    # a world that has switched a factor kind at run time
    p = Pair()
    p.topology()
    p.iterate(sch)
    p.shared.set_enabled(S.EN_DYN | S.EN_OBS | S.EN_IR)
    before = p.shared.read_beliefs()
    with pytest.raises(hostlib.MgxError, match="mgx_set_enabled"):
        p.shared.iterate(sch)
    for x, y in zip(before, p.shared.read_beliefs()):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert p.shared.group_schedule_stats()[0] == 1
    # a live robot whose group is not below n_groups
    with pytest.raises(hostlib.MgxError, match="n_groups"):
        p.shared.iterate(sch[:GROUPS - 1])
    for x, y in zip(before, p.shared.read_beliefs()):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    p.shared.iterate([sch[0]] * GROUPS)                              # equal schedules still run: the plain call
