"""One comms radius per GROUP in the grouped search (include/mgx.h, ROBOT GROUPS; k_group_rows reads its segment's threshold from
GroupTables::thr): mgx_neighbours_groups against (a) a numpy all-pairs scan in f32 with every robot's own group's radius and (b)
mgx_neighbours on a world that holds that group alone, at that radius — the scalar calls this change does not touch.

About 330 robots in 6 groups, ids interleaved, every group in the same place.  Sizes 260 (two 256-candidate passes), 17 and 16 (the
GROUP_ROBOTS slice boundary), 33, 1, and a group whose robots are all removed before the query: it has no segment, and it sits
between two groups of different radii, so a table indexed by anything but the segment's group id shifts them.  Radii 5.0, the
float below 5.0, 0.5, 0.0, -1.0 and NaN.  Positions lie on a quarter-unit lattice (every coordinate, difference, square and sum is
exact in f32) with partners at offsets (3, 0, 4): many pairs at EXACTLY distance 5, in range under 5.0 and out of range under the
float below.  The 33 robots are the lattice points within 0.5 of their centre: its row has 32 entries and outgrows the world's
first row capacity.  One robot has a NaN coordinate, one an inf, in different groups.  Rows of integers are compared: no tolerance."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S

AUTO = hostlib.NEIGHBOURS_AUTO
F = np.float32
BELOW5 = float(np.nextafter(F(5), F(0)))
#          group:  0     1 (emptied)  2       3     4     5
SIZES = np.array([260,   5,           17,     33,   16,   1])
RADII = np.array([5.0,   np.nan,      BELOW5, 0.5,  0.0,  -1.0], dtype=F)
EMPTY, DENSE = 1, 3
SIDE = 320   # the lattice: quarter units 0 .. SIDE in x and z (80 world units: rows under radius 5 stay short)


def numpy_rows(pos, radii, group, alive=None):
    """all pairs in f32, every operation rounded on its own, as in_comms_range spells them: j is in i's row unless
    radius < |p_i - p_j| — with the radius of THEIR group, and only if the two are of one group and both in the query"""
    pos, group = np.asarray(pos, dtype=F), np.asarray(group)
    radii = np.asarray(radii, dtype=F)
    alive = np.ones(len(pos), bool) if alive is None else alive
    rows = []
    with np.errstate(all="ignore"):
        for i in range(len(pos)):
            d = pos[i] - pos
            s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert s.dtype == F
            inr = ~(radii[group[i]] < np.sqrt(s)) & (group == group[i]) & alive & alive[i]
            inr[i] = False
            rows.append(np.nonzero(inr)[0])
    return rows


def rows_of(csr):
    ptr, idx = csr
    return [idx[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def layout():
    """(group of every robot id, positions [n, 3] f32, alive): ids interleaved by a fixed shuffle, every group over the same square"""
    rng = np.random.default_rng(5)
    group = np.concatenate([np.full(n, g) for g, n in enumerate(SIZES)])
    group = group[rng.permutation(len(group))]
    q = np.zeros((len(group), 3), dtype=np.int64)          # quarter units
    q[:, 0], q[:, 2] = rng.integers(0, SIDE, len(group)), rng.integers(0, SIDE, len(group))
    q[:, 1] = 2
    for g in (0, 2, 4):                                    # every second robot of these groups: 3 - 4 - 5 from the one before it
        ids = np.nonzero(group == g)[0]
        q[ids[1::2]] = q[ids[0:len(ids) - 1:2]] + [12, 0, 16]
    dense = np.nonzero(group == DENSE)[0]                  # the 33 lattice points within 0.5 (two quarter units) of a centre
    ball = [(i, j, k) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3) if i * i + j * j + k * k <= 4]
    assert len(ball) == len(dense) == 33 and ball[16] == (0, 0, 0)
    q[dense] = np.array(ball) + [100, 8, 100]
    four = np.nonzero(group == 4)[0]
    q[four[5]] = q[four[4]]                                # coincident: in range under radius 0, out of range under -1
    pos = (q / 4.0).astype(F)
    assert np.array_equal(pos.astype(np.float64) * 4, q)   # (the lattice is exact in f32)
    pos[four[0], 0] = np.nan                               # a NaN distance is "in range" whatever the radius: of ITS group only
    pos[np.nonzero(group == 0)[0][7], 2] = np.inf
    alive = group != EMPTY
    return group, pos, alive


def make_world(group, alive=None):
    sc = S.grid_scenario(len(group), 10, interrobot=False, obstacles=False)
    w = World(sc["params"])
    w.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    for rb, g in zip(sc["robots"], group):
        w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=rb["order_key"], group=int(g))
    for r in ([] if alive is None else np.nonzero(~alive)[0]):
        w.remove_robot(int(r))
    return w


@pytest.fixture(scope="module")
def want():
    group, pos, alive = layout()
    return numpy_rows(pos, RADII, group, alive)


def test_layout_means_what_it_says(want):
    """on the CPU, with the numpy predicate: the pairs at exactly the radius are there, and they decide"""
    group, pos, alive = layout()
    assert len(group) == 332 and sorted(SIZES) == [1, 5, 16, 17, 33, 260]
    with np.errstate(all="ignore"):
        d = pos[:, None, :] - pos[None, :, :]
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    assert dist.dtype == F
    for g in (0, 2):                                        # exactly 5: in range under 5.0, out of range under the float below
        ids = np.nonzero(group == g)[0]
        exact = np.argwhere(dist[np.ix_(ids, ids)] == F(5))
        assert len(exact) >= len(ids) - 4, (g, len(exact))
        for a, b in exact:
            assert (ids[b] in want[ids[a]]) == (g == 0), (g, a, b)
    assert F(BELOW5) < F(5) and not (F(BELOW5) < F(np.nextafter(F(5), F(0))))
    dense = np.nonzero(group == DENSE)[0]                   # ... exactly 0.5 as well, and one row of 32: beyond a capacity of 16
    assert (dist[np.ix_(dense, dense)] == F(0.5)).sum() >= 6 * 2
    assert max(len(want[i]) for i in dense) == 32
    assert max(len(want[i]) for i in np.nonzero(group != DENSE)[0]) <= 16
    four = np.nonzero(group == 4)[0]                         # radius 0: the coincident pair and the NaN robot, nobody else
    assert list(want[four[4]]) == sorted([four[0], four[5]])
    assert len(want[four[0]]) == 15 and all(four[0] in want[j] for j in four[1:])
    assert all(len(want[i]) == 0 for i in np.nonzero(~alive)[0]) and len(want[np.nonzero(group == 5)[0][0]]) == 0
    # the groups overlap in space, and radii shifted by the emptied group would give other rows
    ungated = numpy_rows(pos, np.full(1, 5.0), np.zeros_like(group))
    assert sum(len(r) for r in ungated) > 2 * sum(len(want[i]) for i in np.nonzero(group == 0)[0])
    shifted = np.concatenate([RADII[:EMPTY], RADII[EMPTY + 1:], RADII[-1:]])
    assert not same(numpy_rows(pos, shifted, group, alive), want)


@pytest.mark.gpu
def test_rows_equal_the_numpy_predicate_and_the_groups_alone(want):
    group, pos, alive = layout()
    w = make_world(group, alive)      # (a fresh world: its row capacity is the initial 16)
    got = rows_of(w.neighbours_groups(pos, RADII, AUTO, capacity=sum(len(r) for r in want)))   # (capacity: ONE search, no sizing call)
    assert w.last_search()[:3] == (hostlib.SEARCH_ROWS_GROUPS, 32, 2)     # 32 entries outgrow 16: once more with room, and the table
    assert same(got, want)
    assert same(rows_of(w.neighbours_groups(pos, RADII, hostlib.NEIGHBOURS_GRID)), want)       # the capacity is remembered: one launch
    assert w.last_search()[:3] == (hostlib.SEARCH_ROWS_GROUPS, 32, 1)
    # (b) every group in a world of its own, through the scalar call
    for g in range(len(SIZES)):
        if g == EMPTY:
            continue
        ids = np.nonzero(group == g)[0]
        solo = make_world(np.zeros(len(ids), np.int64))
        alone = rows_of(solo.neighbours(pos[ids], float(RADII[g]), AUTO))
        assert solo.last_search()[0] != hostlib.SEARCH_ROWS_GROUPS
        assert same([ids[r] for r in alone], [got[i] for i in ids]), g


@pytest.mark.gpu
def test_every_radius_on_every_group(want):
    """the radii rotated through the groups: every search uploads another table, the kernel and the launch count stay"""
    group, pos, alive = layout()
    w = make_world(group, alive)
    cap = 16
    for k in range(len(RADII)):
        radii = np.roll(RADII, k)
        ref = numpy_rows(pos, radii, group, alive)
        longest = max(len(r) for r in ref)
        grew = longest > cap
        while cap < longest:
            cap *= 2
        got = rows_of(w.neighbours_groups(pos, radii, AUTO, capacity=sum(len(r) for r in ref)))
        assert w.last_search()[:3] == (hostlib.SEARCH_ROWS_GROUPS, cap, 2 if grew else 1), k
        assert same(got, ref), k
    assert cap == 512      # (the 260 under NaN: 259 entries)


@pytest.mark.gpu
def test_equal_radii_are_the_scalar_grouped_call():
    group, pos, alive = layout()
    w = make_world(group, alive)
    for r in (5.0, BELOW5, 0.0, float("nan")):
        one = rows_of(w.neighbours(pos, r, AUTO))
        assert w.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS
        assert same(rows_of(w.neighbours_groups(pos, np.full(len(SIZES), r, dtype=F))), one), r
        assert same(one, numpy_rows(pos, np.full(len(SIZES), r), group, alive)), r


@pytest.mark.gpu
def test_an_ungrouped_world_with_one_group_is_the_scalar_call():
    group, pos, _ = layout()
    w = make_world(np.zeros_like(group))
    for r in (5.0, BELOW5):
        one = rows_of(w.neighbours(pos, r, AUTO))
        kernel = w.last_search()[0]
        assert kernel not in (hostlib.SEARCH_ROWS_GROUPS, hostlib.SEARCH_NONE)
        assert same(rows_of(w.neighbours_groups(pos, [r])), one) and w.last_search()[0] == kernel, r
    with pytest.raises(hostlib.MgxError, match="n_groups"):
        make_world(group).neighbours_groups(pos, RADII[:3])     # robots of groups 3 .. 5, three radii
