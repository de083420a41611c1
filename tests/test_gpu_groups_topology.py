"""One GROUPED world of three groups against three worlds of their own (include/mgx.h, ROBOT GROUPS): every group of the shared
world has to be, bit for bit, the run it would be alone — robot numbers from its own generator, the same connections created and
deleted in the same passes, the same connection sets, beliefs equal as bit patterns, the same message counts.

9, 12 and 5 robots with K = 8 (magics_amd/scenarios.py robots), ids interleaved across the groups, all three groups in the same
place; the robots drive apart over 30 ticks, so connections come and go.  Once through mgx_update_topology_groups + mgx_tick over
positions the test hands in, once through mgx_mission_tick_begin_groups / mgx_mission_tick_end with missions that end (despawns)."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S

pytestmark = pytest.mark.gpu

SIZES, K, TICKS, RADIUS, HZ = (9, 12, 5), 8, 30, 8.0, 10.0
F = np.float32


def scenarios():
    """one grid scenario per group (its own seed: other places, other headings), and the shared world's order: robot (group g, local
    index i) by turns — [(g, i)] in the order the robots are added"""
    added = K not in S.HORIZON_FOR_K     # (the table of horizons has no entry for 8 variables: one for the time being, as other tests do)
    if added:
        S.HORIZON_FOR_K[K] = next(h for h in range(1, 200) if len(hostlib.variable_timesteps(h, 3)) == K)
    try:
        scs = [S.grid_scenario(n, K, interrobot=True, comm_radius=RADIUS, obstacles=False, seed=805 + g, pitch=4.0) for g, n in enumerate(SIZES)]
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
    for key, (g, i) in enumerate(order):   # (order keys unique per world, ascending within every group as in its own world)
        rb = scs[g]["robots"][i]
        ids[g][i] = shared.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=key, group=g)
    for g, sc in enumerate(scs):
        for i, rb in enumerate(sc["robots"]):
            assert alone[g].add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=i) == i
    if missions:
        dt32 = F(1.0) / F(HZ)
        for g, sc in enumerate(scs):
            for i, rb in enumerate(sc["robots"]):
                heading = (rb["goal"] - rb["pos"]) / np.linalg.norm(rb["goal"] - rb["pos"])
                wp = np.array([rb["pos"] + (4.0 + 2.0 * (i % 4)) * heading])      # 4 .. 10 m ahead: missions end at different ticks
                tr = np.array([rb["pos"][0], -1.5, rb["pos"][1]], dtype=F)
                for w, rid in ((shared, ids[g][i]), (alone[g], i)):
                    w.mission_set(rid, wp, 0, 0, 1.0, 1.0, tr, float(dt32 / rb["t0"]))
    return shared, alone, ids


def positions(scs, t):
    """Transforms the test keeps: every robot on its heading at the target speed — per group [n, 3] f32"""
    out = []
    for sc in scs:
        p = np.zeros((len(sc["robots"]), 3), dtype=F)
        for i, rb in enumerate(sc["robots"]):
            heading = (rb["goal"] - rb["pos"]) / np.linalg.norm(rb["goal"] - rb["pos"])
            xy = rb["pos"] + heading * sc["target_speed"] * t / HZ
            p[i] = [xy[0], 0.5, xy[1]]
        out.append(p)
    return out


def same_state(shared, alone, ids, what):
    bs = shared.read_beliefs()    # per variable, robots in id order
    for g, w in enumerate(alone):
        sel = np.array(ids[g])
        for name, a, b in zip(("eta", "lam", "mean"), bs, w.read_beliefs()):
            a, b = a.reshape((sum(SIZES), K) + a.shape[1:]), b.reshape((SIZES[g], K) + b.shape[1:])
            assert np.array_equal(a[sel], b), (what, g, name)


def same_connections(shared, alone, ids, what):
    for g, w in enumerate(alone):
        for i, rid in enumerate(ids[g]):
            assert shared.connections(rid) == [ids[g][j] for j in w.connections(i)], (what, g, i)


def same_counts(shared, alone, ids):
    for g, w in enumerate(alone):
        for i, rid in enumerate(ids[g]):
            assert shared.message_counts(rid) == w.message_counts(i), (g, i)


def test_update_topology_groups_and_ticks():
    scs, order = scenarios()
    shared, alone, ids = build(scs, order)
    every = {"robots": [scs[g]["robots"][i] for g, i in order], "target_speed": scs[0]["target_speed"]}
    tick_shared, tick_alone = S.tick_inputs(every, HZ), [S.tick_inputs(sc, HZ) for sc in scs]
    steps = scs[0]["steps"]
    nxt, nxt_alone = np.ones(len(SIZES), np.uint64), [1] * len(SIZES)
    created = deleted = 0
    for t in range(TICKS):
        pos = positions(scs, t)
        pos_shared = np.zeros((len(order), 3), dtype=F)
        for g in range(len(SIZES)):
            pos_shared[ids[g]] = pos[g]
        nxt, stats = shared.update_topology_groups(pos_shared, RADIUS, nxt)
        assert shared.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS
        for g, w in enumerate(alone):
            nxt_alone[g], c, d = w.update_topology(pos[g], RADIUS, nxt_alone[g])
            assert (int(nxt[g]), int(stats[g, 0]), int(stats[g, 1])) == (nxt_alone[g], c, d), (t, g)
            created, deleted = created + c, deleted + d
        same_connections(shared, alone, ids, t)
        shared.tick(steps=steps, **tick_shared)
        for g, w in enumerate(alone):
            w.tick(steps=steps, **tick_alone[g])
        if t % 5 == 4:
            same_state(shared, alone, ids, t)
    assert created > 0 and deleted > 0      # connections came and went
    same_counts(shared, alone, ids)


def test_mission_ticks_by_group_with_despawns():
    scs, order = scenarios()
    shared, alone, ids = build(scs, order, missions=True)
    back = {ids[g][i]: (g, i) for g in range(len(SIZES)) for i in range(SIZES[g])}
    steps = scs[0]["steps"]
    speed, dt = S.f32w(scs[0]["target_speed"]), float(F(1.0) / F(HZ))
    nxt, nxt_alone = np.ones(len(SIZES), np.uint64), [1] * len(SIZES)
    created = deleted = finished = 0
    for t in range(TICKS):
        nxt, stats, fin = shared.mission_tick_begin_groups(RADIUS, nxt, despawn_finished=True)
        assert shared.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS
        fin_by_group = [[i for g2, i in (back[int(r)] for r in fin) if g2 == g] for g in range(len(SIZES))]
        for g, w in enumerate(alone):
            nxt_alone[g], c, d, f = w.mission_tick_begin(RADIUS, nxt_alone[g], despawn_finished=True)
            assert (int(nxt[g]), int(stats[g, 0]), int(stats[g, 1]), int(stats[g, 2])) == (nxt_alone[g], c, d, len(f)), (t, g)
            assert fin_by_group[g] == [int(i) for i in f], (t, g)
            created, deleted, finished = created + c, deleted + d, finished + len(f)
        same_connections(shared, alone, ids, t)
        shared.mission_tick_end(steps, speed, dt)
        for w in alone:
            w.mission_tick_end(steps, speed, dt)
        if t % 5 == 4:
            same_state(shared, alone, ids, t)
            tr = shared.mission_read()[0]
            for g, w in enumerate(alone):
                assert np.array_equal(tr[ids[g]].view(np.uint32), w.mission_read()[0].view(np.uint32)), (t, g)
    assert created > 0 and finished > 0     # robots met, and missions ended (their robots despawned)
    same_counts(shared, alone, ids)


def test_single_generator_calls_keep_working_on_a_grouped_world():
    """one shared generator, grouped search: the numbers run through all groups in robot id order, nobody connects across groups"""
    scs, order = scenarios()
    shared, _, ids = build(scs, order)
    pos = positions(scs, 0)
    pos_shared = np.zeros((len(order), 3), dtype=F)
    for g in range(len(SIZES)):
        pos_shared[ids[g]] = pos[g]
    nxt, c, d = shared.update_topology(pos_shared, RADIUS, 1)
    assert shared.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS
    assert c > 0 and d == 0 and nxt == 1 + c * (K - 1)
    group_of = {rid: g for g in range(len(SIZES)) for rid in ids[g]}
    for rid in group_of:
        assert all(group_of[o] == group_of[rid] for o in shared.connections(rid))


def test_arguments_that_need_a_world():
    """a robot's group not below n_groups; ghosts and groups do not share a world"""
    scs, order = scenarios()
    shared, _, ids = build(scs, order)
    pos = np.zeros((len(order), 3), dtype=F)
    with pytest.raises(hostlib.MgxError, match="n_groups"):
        shared.update_topology_groups(pos, RADIUS, np.ones(len(SIZES) - 1, np.uint64))
    with pytest.raises(hostlib.MgxError, match="n_groups"):
        shared.mission_tick_begin_groups(RADIUS, np.ones(len(SIZES) - 1, np.uint64))
    assert all(shared.connections(r) == [] for g in ids for r in g)      # nothing happened
    rb = scs[0]["robots"][0]
    with pytest.raises(hostlib.MgxError, match="ghost"):
        shared.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=1000, ghost=True)
    with pytest.raises(hostlib.MgxError, match="MGX_GROUPS_MAX"):
        shared.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=1001, group=hostlib.GROUPS_MAX)
    sharded = World(scs[0]["params"])
    sharded.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=0, ghost=True)
    with pytest.raises(hostlib.MgxError, match="ghosts"):
        sharded.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=1, group=2)
