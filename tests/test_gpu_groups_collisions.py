"""Robot-robot collision bookkeeping of a GROUPED world (include/mgx.h, ROBOT GROUPS; magics_amd/csrc/mgx_collisions.hip) against
the same groups in worlds of their own: robots of different groups never collide — although here robot i of every group sits
exactly ON robot i of every other group, in every pass — and within a group the events (in (pass, a, b) order, AABBs as f32 bit
patterns) and the per-robot counts are the ones of the group's own world under the id mapping.  Both search forms of the pass,
all pairs and the hash grid; a pair that parts and meets again counts twice."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = (70, 25, 7)      # (the all-pairs form works in blocks of 64 robots: the largest group and the shared world span several)
PASSES = 6


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _events(ev):
    return [(int(e["pass"]), int(e["robot_a"]), int(e["robot_b"]), tuple(_bits(v) for v in e["mins"]), tuple(_bits(v) for v in e["maxs"]))
            for e in ev]


def _world(radii, groups=None):
    """robots that only stand for their radii (the passes get their positions handed in)"""
    w = World(scenarios.JUNCTION_PARAMS)
    mean0, prior, dt = scenarios.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), scenarios.timesteps_for_K(10), 1.0, 5.0, 5.0)
    for k, r in enumerate(radii):
        w.add_robot(mean0, prior, dt, float(r), group=0 if groups is None else int(groups[k]))
    return w


def script():
    """radii [n] and positions [pass][n, 3] that EVERY group uses (group g: the first SIZES[g] robots): a crowd that mills about,
    and robots 0 and 1 on their own far away — together, apart, together again"""
    rng = np.random.default_rng(5)
    n = max(SIZES)
    radii = rng.uniform(0.6, 1.4, n).astype(F)
    base = rng.uniform(-12, 12, size=(n, 2))
    passes = []
    for p in range(PASSES):
        xy = base + rng.normal(0, 1.2, size=(n, 2))
        xy[0] = (100.0, 100.0)
        xy[1] = (100.5, 100.0) if p % 2 == 0 else (110.0, 100.0)
        pos = np.zeros((n, 3), dtype=F)
        pos[:, 0], pos[:, 1], pos[:, 2] = xy[:, 0], -1.5, xy[:, 1]
        passes.append(pos)
    return radii, passes


@pytest.mark.parametrize("method", [hostlib.NEIGHBOURS_PAIRS, hostlib.NEIGHBOURS_GRID])
def test_groups_collide_only_among_themselves(method):
    radii, passes = script()
    order = [(g, i) for i in range(max(SIZES)) for g in range(len(SIZES)) if i < SIZES[g]]   # ids interleaved across the groups
    ids = [[None] * n for n in SIZES]
    for rid, (g, i) in enumerate(order):
        ids[g][i] = rid
    shared = _world([radii[i] for _, i in order], [g for g, _ in order])
    alone = [_world(radii[:n]) for n in SIZES]
    for w in [shared] + alone:
        w.collisions_enable(True, method=method)
    for pos in passes:
        every = np.zeros((len(order), 3), dtype=F)
        for g, n in enumerate(SIZES):
            every[ids[g]] = pos[:n]
        shared.collisions_update(every)
        for g, n in enumerate(SIZES):
            alone[g].collisions_update(pos[:n])
    ev, total, dropped, per = shared.collisions_read()
    assert dropped == 0 and total == len(ev)
    group_of = {rid: g for g in range(len(SIZES)) for rid in ids[g]}
    local = {rid: i for g in range(len(SIZES)) for i, rid in enumerate(ids[g])}
    got = [[] for _ in SIZES]
    for p, a, b, lo, hi in _events(ev):
        assert group_of[a] == group_of[b], (p, a, b)          # nobody collides across groups
        got[group_of[a]].append((p, local[a], local[b], lo, hi))
    for g, w in enumerate(alone):
        ev_g, total_g, dropped_g, per_g = w.collisions_read()
        assert dropped_g == 0
        assert got[g] == _events(ev_g), g                      # the shared log is in (pass, a, b) order; the mapping keeps it
        assert np.array_equal(per[ids[g]], per_g), g
    assert sum(len(x) for x in got) > 20 and all(len(x) > 0 for x in got[:2])
    pair = [e for e in got[0] if (e[1], e[2]) == (0, 1)]
    assert [e[0] for e in pair] == [0, 2, 4]                   # together, apart, together again: one event per meeting
    assert per[ids[2][0]] == sum(1 for e in got[2] if 0 in (e[1], e[2]))
