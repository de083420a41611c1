"""One comms radius per group through the topology pass and the mission tick (mgx_update_topology_groups_radii,
mgx_mission_tick_begin_groups_radii; include/mgx.h, ROBOT GROUPS): ONE world of three groups with radii 2, 4 and 8 against three
worlds of their own, each through the scalar calls at its own radius — connections, robot numbers, per-group stats and beliefs
(bit patterns) are equal.  3 x 6 robots, K = 8, ids interleaved, all three groups along the same line.

Scripted positions: every group's robots on a line whose spacing is its radius times 0.9, 1.1, 0.45, 1.2, 0.8, 0.3 over six
steps, so pairs cross their group's radius in both directions (checked with the numpy predicate before anything runs).  Mission
ticks: from the second tick on the rows are the ones the tick before searched ahead; at tick 4 group 1's radius becomes 8, and
that tick's connections have to be the new radius's — rows searched ahead with the old one must not be used."""
import ctypes as C

import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S

SIZES, K, STEPS, HZ = (6, 6, 6), 8, 6, 10.0
RADII = np.array([2.0, 4.0, 8.0], dtype=np.float32)
SPACING = (0.9, 1.1, 0.45, 1.2, 0.8, 0.3)      # of the group's radius
CHANGE_AT, CHANGED = 4, np.array([2.0, 8.0, 8.0], dtype=np.float32)
F = np.float32


def in_range(pos, radius):
    """the predicate in f32, every operation rounded on its own: [n, n] bool, the diagonal False"""
    pos = np.asarray(pos, dtype=F)
    d = pos[:, None, :] - pos[None, :, :]
    s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    out = ~(F(radius) < np.sqrt(s))
    np.fill_diagonal(out, False)
    return out


def scripted(t):
    """per group [n, 3] f32: a line along x from the same origin for every group"""
    return [np.array([[SPACING[t] * float(r) * i, 0.5, 0.0] for i in range(n)], dtype=F) for n, r in zip(SIZES, RADII)]


def transforms():
    """the missions' first Transforms, per group: a line of pitch 0.65 radius — neighbours at 0.65, 1.3, 1.95 .. radii"""
    return [np.array([[0.65 * float(r) * i, -1.5, 0.0] for i in range(n)], dtype=F) for n, r in zip(SIZES, RADII)]


def test_the_script_crosses_every_radius_both_ways():
    for g, r in enumerate(RADII):
        before = in_range(scripted(0)[g], r)
        assert before.any() and not before.all()
        came = went = 0
        for t in range(1, STEPS):
            now = in_range(scripted(t)[g], r)
            came, went = came + int((now & ~before).sum()), went + int((before & ~now).sum())
            before = now
        assert came > 0 and went > 0, g
    # the radius that changes: group 1 has pairs between the old and the new radius — the second neighbours, 5.2 apart — with more
    # room than the robots travel in four ticks (0.1 a tick each at target speed 1: 0.8 between two of them)
    tr = transforms()[1]
    d = np.abs(tr[:, None, 0] - tr[None, :, 0])
    assert ((d > RADII[1] + 1.0) & (d < CHANGED[1] - 1.0)).sum() == 8
    assert CHANGED[1] != RADII[1] and CHANGED[0] == RADII[0] and CHANGED[2] == RADII[2]


def scenarios():
    added = K not in S.HORIZON_FOR_K     # (the table of horizons has no entry for 8 variables: one for the time being, as other tests do)
    if added:
        S.HORIZON_FOR_K[K] = next(h for h in range(1, 200) if len(hostlib.variable_timesteps(h, 3)) == K)
    try:
        scs = [S.grid_scenario(n, K, interrobot=True, comm_radius=float(RADII[g]), obstacles=False, seed=805 + g, pitch=4.0, target_speed=1.0)
               for g, n in enumerate(SIZES)]
    finally:
        if added:
            del S.HORIZON_FOR_K[K]
    order = [(g, i) for i in range(max(SIZES)) for g in range(len(SIZES)) if i < SIZES[g]]
    return scs, order


def build(scs, order, missions=False):
    """the shared world and the groups' own worlds; ids[g][i]: the shared world's id of robot i of group g"""
    sdf = scs[0]["sdf"]
    shared, alone = World(scs[0]["params"]), [World(sc["params"]) for sc in scs]
    for w in [shared] + alone:
        w.set_sdf(sdf["rgb"], sdf["world_w"], sdf["world_h"])
    ids = [[None] * n for n in SIZES]
    for key, (g, i) in enumerate(order):
        rb = scs[g]["robots"][i]
        ids[g][i] = shared.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=key, group=g)
    for g, sc in enumerate(scs):
        for i, rb in enumerate(sc["robots"]):
            assert alone[g].add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=i) == i
    if missions:
        dt32 = F(1.0) / F(HZ)
        tr = transforms()
        for g, sc in enumerate(scs):
            for i, rb in enumerate(sc["robots"]):
                heading = (rb["goal"] - rb["pos"]) / np.linalg.norm(rb["goal"] - rb["pos"])
                wp = np.array([rb["pos"] + 50.0 * heading])
                for w, rid in ((shared, ids[g][i]), (alone[g], i)):
                    w.mission_set(rid, wp, 0, 0, 1.0, 1.0, tr[g][i], float(dt32 / rb["t0"]))
    return shared, alone, ids


def same_beliefs(shared, alone, ids, what):
    bs = shared.read_beliefs()
    for g, w in enumerate(alone):
        sel = np.array(ids[g])
        for name, a, b in zip(("eta", "lam", "mean"), bs, w.read_beliefs()):
            a, b = a.reshape((sum(SIZES), K) + a.shape[1:]), b.reshape((SIZES[g], K) + b.shape[1:])
            assert np.array_equal(a[sel], b), (what, g, name)


def same_connections(shared, alone, ids, what):
    for g, w in enumerate(alone):
        for i, rid in enumerate(ids[g]):
            assert shared.connections(rid) == [ids[g][j] for j in w.connections(i)], (what, g, i)


@pytest.mark.gpu
def test_update_topology_with_one_radius_per_group():
    scs, order = scenarios()
    shared, alone, ids = build(scs, order)
    steps = scs[0]["steps"]
    nxt, nxt_alone = np.ones(len(SIZES), np.uint64), [1] * len(SIZES)
    created, deleted = np.zeros(3, int), np.zeros(3, int)
    for t in range(STEPS):
        pos = scripted(t)
        pos_shared = np.zeros((len(order), 3), dtype=F)
        for g in range(len(SIZES)):
            pos_shared[ids[g]] = pos[g]
        nxt, stats = shared.update_topology_groups(pos_shared, RADII, nxt)
        assert shared.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS and shared.last_search()[2] == 1
        for g, w in enumerate(alone):
            nxt_alone[g], c, d = w.update_topology(pos[g], float(RADII[g]), nxt_alone[g])
            assert (int(nxt[g]), int(stats[g, 0]), int(stats[g, 1])) == (nxt_alone[g], c, d), (t, g)
            created[g], deleted[g] = created[g] + c, deleted[g] + d
        same_connections(shared, alone, ids, t)
        for w in [shared] + alone:
            w.iterate(steps)
        same_beliefs(shared, alone, ids, t)
    assert (created > 0).all() and (deleted > 0).all()      # in every group connections came and went


@pytest.mark.gpu
def test_mission_ticks_with_a_radius_that_changes():
    scs, order = scenarios()
    shared, alone, ids = build(scs, order, missions=True)
    steps = scs[0]["steps"]
    speed, dt = S.f32w(scs[0]["target_speed"]), float(F(1.0) / F(HZ))
    nxt, nxt_alone = np.ones(len(SIZES), np.uint64), [1] * len(SIZES)
    at_change = None
    for t in range(STEPS):
        radii = CHANGED if t >= CHANGE_AT else RADII
        nxt, stats, fin = shared.mission_tick_begin_groups(radii, nxt, despawn_finished=True)
        assert shared.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS and len(fin) == 0
        for g, w in enumerate(alone):
            nxt_alone[g], c, d, f = w.mission_tick_begin(float(radii[g]), nxt_alone[g], despawn_finished=True)
            assert (int(nxt[g]), int(stats[g, 0]), int(stats[g, 1]), int(stats[g, 2])) == (nxt_alone[g], c, d, len(f)), (t, g)
        same_connections(shared, alone, ids, t)
        if t == CHANGE_AT:
            at_change = stats.copy()
        shared.mission_tick_end(steps, speed, dt)
        for w in alone:
            w.mission_tick_end(steps, speed, dt)
        same_beliefs(shared, alone, ids, t)
        tr = shared.mission_read()[0]
        for g, w in enumerate(alone):
            assert np.array_equal(tr[ids[g]].view(np.uint32), w.mission_read()[0].view(np.uint32)), (t, g)
    # the tick of the change connected group 1's second neighbours: the NEW radius's rows (the ones searched ahead were the old radius's)
    assert at_change[1, 0] >= 8


@pytest.mark.gpu
def test_argument_errors_leave_the_world_unchanged():
    scs, order = scenarios()
    shared, alone, ids = build(scs, order, missions=True)
    pos = scripted(0)
    pos_shared = np.zeros((len(order), 3), dtype=F)
    for g in range(len(SIZES)):
        pos_shared[ids[g]] = pos[g]
    L, numbers, stats = hostlib.lib(), np.ones(3, np.uint64), np.zeros((3, 3), np.uint32)
    INVALID = -1
    for n_groups, radii in ((2, RADII[:2]), (3, None), (0, RADII), (hostlib.GROUPS_MAX + 1, RADII)):
        rp = None if radii is None else radii.ctypes.data
        assert L.mgx_update_topology_groups_radii(shared._w, pos_shared.ctypes.data, rp, 0, n_groups, numbers.ctypes.data, stats.ctypes.data) == INVALID
        assert L.mgx_mission_tick_begin_groups_radii(shared._w, rp, 0, n_groups, numbers.ctypes.data, 1, stats.ctypes.data) == INVALID
        ptr = np.zeros(len(order) + 1, np.int32)
        assert L.mgx_neighbours_groups(shared._w, pos_shared.ctypes.data, rp, n_groups, 0, ptr.ctypes.data, None, 0, C.byref(C.c_uint64())) == INVALID
    with pytest.raises(hostlib.MgxError, match="n_groups"):
        shared.update_topology_groups(pos_shared, RADII[:2], np.ones(2, np.uint64))
    with pytest.raises(ValueError, match="per group"):
        shared.mission_tick_begin_groups(RADII[:2], np.ones(3, np.uint64))
    assert list(numbers) == [1, 1, 1] and all(shared.connections(r) == [] for g in ids for r in g)      # nothing happened
    with pytest.raises(hostlib.MgxError, match="without"):
        shared.mission_tick_end(scs[0]["steps"], 1.0, 0.1)                                                # ... and no tick began
    nxt, st = shared.update_topology_groups(pos_shared, RADII, numbers)                                   # the world is as it was
    for g, w in enumerate(alone):
        n, c, d = w.update_topology(pos[g], float(RADII[g]), 1)
        assert (int(nxt[g]), int(st[g, 0]), int(st[g, 1])) == (n, c, d)
    same_connections(shared, alone, ids, "after the refused calls")
