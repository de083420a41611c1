"""The comms-range search of a GROUPED world (include/mgx.h, ROBOT GROUPS; k_group_rows, magics_amd/csrc/mgx_topology.hip)
against a numpy all-pairs scan masked by group — the f32 predicate restated as tests/test_oracle_topology.py restates it.

The kernel serves GROUP_ROBOTS = 16 robots of one group per workgroup and looks at 256 candidates per pass, so the group sizes
are 1, 15, 16, 17, 255, 256 and 257; one more group of 40 robots is dense (every row has 39 entries: it outgrows the world's row
capacity of 16 and of 32, the host repeats the search), and one holds NaN and inf coordinates.  Ids are interleaved across
the groups and EVERY group occupies the same region of space, so a search that did not look at the group would fail every row.
Nothing has a tolerance: rows of integers are compared."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S

pytestmark = pytest.mark.gpu

AUTO, PAIRS, GRID = hostlib.NEIGHBOURS_AUTO, hostlib.NEIGHBOURS_PAIRS, hostlib.NEIGHBOURS_GRID
SIZES = [1, 15, 16, 17, 255, 256, 257]   # groups 0 .. 6: the robot-slice (16) and candidate-pass (256) boundaries of k_group_rows
DENSE, WILD = 7, 8                       # group 7: 40 robots all in range of one another; group 8: 20 robots, some NaN / inf
N_DENSE, N_WILD = 40, 20
RADIUS = 3.0


def numpy_rows(pos, radius, group, alive=None):
    """all pairs in f32, every operation rounded on its own; j is in i's row unless radius < |p_i - p_j| — and only if the two are
    of one group (and both in the query)"""
    pos, r = np.asarray(pos, dtype=np.float32), np.float32(radius)
    alive = np.ones(len(pos), bool) if alive is None else alive
    rows = []
    with np.errstate(all="ignore"):
        for i in range(len(pos)):
            d = pos[i] - pos
            s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            inr = ~(r < np.sqrt(s)) & (group == group[i]) & alive & alive[i]
            inr[i] = False
            rows.append(np.nonzero(inr)[0])
    return rows


def rows_of(csr):
    ptr, idx = csr
    return [idx[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def layout():
    """(group of every robot id, positions): ids interleaved across the groups by a fixed shuffle, every group in the same square"""
    rng = np.random.default_rng(11)
    group = np.concatenate([np.full(n, g) for g, n in enumerate(SIZES)] + [np.full(N_DENSE, DENSE), np.full(N_WILD, WILD)]).astype(np.int64)
    group = group[rng.permutation(len(group))]
    pos = rng.uniform(-20, 20, size=(len(group), 3)).astype(np.float32)
    pos[:, 1] = 0.5
    dense = np.nonzero(group == DENSE)[0]
    pos[dense] = (rng.uniform(-0.5, 0.5, size=(N_DENSE, 3)) + [3.0, 0.0, -4.0]).astype(np.float32)   # all within RADIUS of one another
    wild = np.nonzero(group == WILD)[0]
    pos[wild[0], 0] = np.nan                 # a NaN distance is "in range": of everybody in ITS group, of nobody else
    pos[wild[1], 2] = np.inf
    pos[wild[2]] = [-np.inf, 0.0, 0.0]
    pos[wild[3]] = [3e38, 0.0, -3e38]        # squares overflow
    pos[wild[4]] = pos[wild[5]]              # coincident
    return group, pos


def make_world(group):
    sc = S.grid_scenario(len(group), 10, interrobot=False, obstacles=False)
    w = World(sc["params"])
    w.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    for rb, g in zip(sc["robots"], group):
        w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], order_key=rb["order_key"], group=int(g))
    return w


@pytest.fixture(scope="module")
def grouped():
    group, pos = layout()
    return make_world(group), group, pos


def test_layout_means_what_it_says():
    group, pos = layout()
    want = numpy_rows(pos, RADIUS, group)
    ungated = numpy_rows(pos, RADIUS, np.zeros_like(group))
    assert sum(len(r) for r in ungated) > 2 * sum(len(r) for r in want)          # the groups overlap in space
    assert all(len(want[i]) == N_DENSE - 1 for i in np.nonzero(group == DENSE)[0])  # beyond a capacity of 32
    wild = np.nonzero(group == WILD)[0]
    assert len(want[wild[0]]) == N_WILD - 1 and all(wild[0] in want[j] for j in wild[1:])
    assert not any(wild[0] in want[j] for j in np.nonzero(group != WILD)[0])


def test_rows_equal_the_masked_scan_and_the_search_is_repeated_with_room():
    group, pos = layout()
    w = make_world(group)     # (a fresh world: its row capacity is the initial 16)
    want = numpy_rows(pos, RADIUS, group)
    got = rows_of(w.neighbours(pos, RADIUS, AUTO, capacity=sum(len(r) for r in want)))   # (capacity: ONE search, no sizing call)
    kernel, cap, launches = w.last_search()[:3]
    assert kernel == hostlib.SEARCH_ROWS_GROUPS
    assert cap == 64 and launches == 2           # 39 entries outgrow 16: once more with 64
    assert same(got, want)
    for method in (PAIRS, GRID, AUTO):           # whatever the method; the capacity is remembered: one launch
        assert same(rows_of(w.neighbours(pos, RADIUS, method)), want), method
        assert w.last_search()[:3] == (hostlib.SEARCH_ROWS_GROUPS, 64, 1), method


@pytest.mark.parametrize("radius", [0.0, -1.0, float("nan"), float("inf"), 1e-30, 11.0])
def test_degenerate_radii(grouped, radius):
    w, group, pos = grouped
    assert same(rows_of(w.neighbours(pos, radius, AUTO)), numpy_rows(pos, radius, group)), radius
    assert w.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS


def test_removed_robots_leave_the_query():
    group, pos = layout()
    w = make_world(group)
    alive = np.ones(len(group), bool)
    rng = np.random.default_rng(3)
    gone = rng.choice(len(group), size=120, replace=False)
    gone = np.unique(np.concatenate([gone, np.nonzero(group == 0)[0]]))   # ... and the one robot of group 0: a group nobody is left of
    for r in gone:
        w.remove_robot(int(r))
        alive[r] = False
    want = numpy_rows(pos, RADIUS, group, alive)
    assert same(rows_of(w.neighbours(pos, RADIUS, AUTO)), want)
    assert w.last_search()[0] == hostlib.SEARCH_ROWS_GROUPS
    assert all(len(want[r]) == 0 for r in gone)
    for r in np.nonzero((group == DENSE) & alive)[0][:5]:              # once more, other robots gone: the member lists are built again
        w.remove_robot(int(r))
        alive[r] = False
    assert same(rows_of(w.neighbours(pos, RADIUS, GRID)), numpy_rows(pos, RADIUS, group, alive))


def test_a_world_of_group_zero_runs_todays_kernels():
    group, pos = layout()
    w = make_world(np.zeros_like(group))
    n = len(group)
    assert 513 <= n <= 1024
    want = numpy_rows(pos, RADIUS, np.zeros_like(group))
    cap = 16
    while cap < max(len(r) for r in want):   # (the NaN robot is in range of everybody)
        cap *= 2
    assert cap > 32
    assert same(rows_of(w.neighbours(pos, RADIUS, AUTO, capacity=sum(len(r) for r in want))), want)
    # rows beyond the grid kernels' 32 entries: the all-pairs rows kernel of 513 .. 1024 robots, launched twice
    assert w.last_search()[:3] == (hostlib.SEARCH_ROWS_PAIRS_2, cap, 2)
    assert same(rows_of(w.neighbours(pos, RADIUS, PAIRS)), want) and w.last_search()[0] == hostlib.SEARCH_TWO_PASS_PAIRS
    assert same(rows_of(w.neighbours(pos, RADIUS, GRID)), want) and w.last_search()[0] == hostlib.SEARCH_TWO_PASS_GRID
    sparse = pos[(group != DENSE) & (group != WILD)]
    assert max(len(r) for r in numpy_rows(sparse, 1.0, np.zeros(len(sparse), np.int64))) <= 16
    w2 = make_world(np.zeros(len(sparse), np.int64))
    assert same(rows_of(w2.neighbours(sparse, 1.0, AUTO)), numpy_rows(sparse, 1.0, np.zeros(len(sparse), np.int64)))
    assert w2.last_search()[0] in (hostlib.SEARCH_ROWS_GRID_16, hostlib.SEARCH_ROWS_GRID_32)
