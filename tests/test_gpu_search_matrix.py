"""Every kernel of the comms-range neighbour search, stated and asserted (magics_amd/csrc/mgx_topology.hip).

Which kernel a search runs depends on things the caller cannot see: the number of robots (breaks at 512/513, 1024/1025 and
4096/4097), whether the radius is usable (finite and positive), and the world's row capacity, which starts at 16 and doubles
whenever a row outgrows it.  So every step below names the kernel it means to run and asserts it through World.last_search()
(mgx_last_search: what the launching branch wrote down) — a wrong kernel fails, it never skips — and then compares the CSR with
the oracle's all-pairs scan in f32 (tests/test_oracle_topology.py pins that scan against numpy), exactly.  The row capacity
belongs to the world and only grows: a test is a SCRIPT on one fresh world per size that walks the capacity upwards.

The inputs are recipes (plain numpy); test_recipes_mean_what_they_say runs every one of them through the oracle alone and checks
the conditions the scripts rely on, so the GPU half can fail only because of the engine.  The changed-row flags of the one-pass
grid kernels (what lets the host's create / delete pass skip robots) are compared byte for byte with what the oracle's rows of
two consecutive passes say.  Nothing here has a tolerance: every comparison is of integers."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from magics_amd import World, hostlib, scenarios as S

F = np.float32
AUTO, PAIRS, GRID = hostlib.NEIGHBOURS_AUTO, hostlib.NEIGHBOURS_PAIRS, hostlib.NEIGHBOURS_GRID
TWO_PAIRS, TWO_GRID = hostlib.SEARCH_TWO_PASS_PAIRS, hostlib.SEARCH_TWO_PASS_GRID
ROWS_PAIRS_4, ROWS_PAIRS_2 = hostlib.SEARCH_ROWS_PAIRS_4, hostlib.SEARCH_ROWS_PAIRS_2
GRID_16, GRID_32 = hostlib.SEARCH_ROWS_GRID_16, hostlib.SEARCH_ROWS_GRID_32
NAMES = {TWO_PAIRS: "TWO_PASS_PAIRS", TWO_GRID: "TWO_PASS_GRID", ROWS_PAIRS_4: "ROWS_PAIRS_4", ROWS_PAIRS_2: "ROWS_PAIRS_2",
         GRID_16: "ROWS_GRID_16", GRID_32: "ROWS_GRID_32"}
HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [1, 2, 3, 5, 6, 7, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1000, 1023, 1024, 1025, 4096, 4097]
TALLY = collections.Counter()   # kernel code -> times a step asserted it


# ---- the dispatch as include/mgx.h and mgx_search.h document it (restated here: never read from the code under test) -------------
def usable(radius):
    return bool(np.isfinite(radius) and radius > 0)


def pairs_rows(n):
    """k_pairs_rows<2,128> for the worlds that fill the device with their resident launch, <4,64> otherwise"""
    return ROWS_PAIRS_2 if 513 <= n <= 1024 else ROWS_PAIRS_4


def rows_kernel(n, cap, radius):
    if n <= 1024 and cap <= 32 and usable(radius):
        return GRID_16 if cap <= 16 else GRID_32
    return pairs_rows(n)


def grown(cap, longest):
    while cap < longest:
        cap *= 2
    return cap


def expected_search(n, cap, radius, longest):
    """(kernel launched last, its row capacity, launches) of an AUTO search on a world whose row capacity is `cap`"""
    if n > 4096:
        return (TWO_GRID if usable(radius) else TWO_PAIRS), 0, None
    after = grown(cap, longest)
    return rows_kernel(n, after, radius), after, (2 if after != cap else 1)


# ---- worlds ------------------------------------------------------------------------------------------------------------------
_SCENARIOS, _ORACLES = {}, {}


def _scenario(n):
    if n not in _SCENARIOS:
        _SCENARIOS[n] = S.grid_scenario(n, 10, interrobot=False, obstacles=False)   # inter-robot factors off, keys ascending
    return _SCENARIOS[n]


def _oracle(n):
    """one oracle world per size for the searches (orc_neighbours changes nothing)"""
    if n not in _ORACLES:
        w = oracle.OracleWorld(_scenario(n)["params"])
        S.populate(w, _scenario(n))
        _ORACLES[n] = w
    return _ORACLES[n]


def _engine(n):
    w = World(_scenario(n)["params"])
    S.populate(w, _scenario(n))
    return w


def degrees(want):
    return np.diff(want[0])


def rows_of(want):
    ptr, idx = want
    return [idx[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]


# ---- recipes (numpy only) ----------------------------------------------------------------------------------------------------
def _xyz(x, z):
    pos = np.zeros((len(x), 3), F)
    pos[:, 0], pos[:, 1], pos[:, 2] = x, 0.5, z
    return pos


def _isolated(m, pitch, x0):
    """m robots nobody reaches: a lattice of `pitch` to the right of x0, on both sides of zero in z"""
    side = max(1, int(np.ceil(np.sqrt(m))))
    k = np.arange(m)
    return x0 + pitch * (k % side), pitch * (k // side) - pitch * (side // 2) + 0.25


def sparse(n, seed=None):
    """random positions on both sides of zero, about three others in range of each; radius 1"""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    half = max(0.4, np.sqrt(n * np.pi / 12.0))
    return _xyz(rng.uniform(-half, half, n), rng.uniform(-half, half, n)), 1.0


def hub(n, k, seed=0):
    """one robot with exactly k others in range (on a circle of 0.95 radii around it: a spoke reaches the third of the others
    whose chord is short enough), everybody else out of anyone's reach; robot numbers shuffled; radius 1"""
    assert n >= k + 1
    rng = np.random.default_rng(7000 + 64 * n + k + seed)
    x, z = np.zeros(n), np.zeros(n)
    ang = 0.1 + 2 * np.pi * np.arange(k) / k
    x[1:k + 1], z[1:k + 1] = 0.95 * np.cos(ang), 0.95 * np.sin(ang)
    x[k + 1:], z[k + 1:] = _isolated(n - k - 1, 3.0, 6.0)
    perm = rng.permutation(n)
    return _xyz(x[perm], z[perm]), 1.0


def dense(n, seed=None):
    """a jittering unit lattice centred on zero under radius 2.3: an interior robot reaches the 12 within distance 2 and those of
    its 8 at sqrt(5) that the jitter leaves in range"""
    rng = np.random.default_rng(2000 + n if seed is None else seed)
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    x = (k % side) - side // 2 + rng.uniform(-0.08, 0.08, n)
    z = (k // side) - side // 2 + rng.uniform(-0.08, 0.08, n)
    return _xyz(x, z), 2.3


def crowd(n):
    """everyone within range of everyone; radius 1"""
    rng = np.random.default_rng(3000 + n)
    return _xyz(rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)), 1.0


Step = collections.namedtuple("Step", "label pos radius kernel cap launches check")


def _kernel_or_pairs(n, kernel):
    return pairs_rows(n) if n > 1024 else kernel


def main_script(n):
    """steps a-g of the table on ONE world (row capacity 16 at the start): (label, positions, radius, the kernel the step means to
    run last, its capacity, its launches, the condition on the oracle's degrees)"""
    out = []
    if n > 4096:   # the two-pass forms
        out.append(Step("a", *sparse(n), TWO_GRID, 0, 1, lambda d: d.max() <= 15 and (d > 0).any()))
        out.append(Step("d", *dense(n), TWO_GRID, 0, 2, lambda d: 17 <= d.max() <= 31 and (d > 16).sum() >= n / 4))   # (rows beyond the guess: the fill again)
        out.append(Step("a again", *sparse(n), TWO_GRID, 0, 1, lambda d: d.max() <= 15))
        return out
    big = n > 1024   # no grid in LDS: the all-pairs rows kernel throughout, the capacity walks the same way
    out.append(Step("a", *sparse(n), _kernel_or_pairs(n, GRID_16), 16, 1, lambda d: d.max() <= 15 and (n == 1 or (d > 0).any())))
    if not big:
        if n >= 17:
            out.append(Step("b", *hub(n, 16), GRID_16, 16, 1, lambda d: d.max() == 16 and (d == 16).sum() == 1))
        if n >= 18:
            out.append(Step("c", *hub(n, 17), GRID_32, 32, 2, lambda d: d.max() == 17 and (d > 16).sum() == 1))
    if n >= 63:
        first = big or n < 18   # (nothing before it grew the capacity)
        out.append(Step("d", *dense(n), _kernel_or_pairs(n, GRID_32), 32, 2 if first else 1,
                        lambda d: 17 <= d.max() <= 31 and (d > 16).sum() >= n / 4))
    if not big:
        if n >= 33:
            out.append(Step("e", *hub(n, 32), GRID_32, 32, 1, lambda d: d.max() == 32 and (d > 16).sum() == 1))
        if n >= 34:
            out.append(Step("f", *hub(n, 33), pairs_rows(n), 64, 2, lambda d: d.max() == 33 and (d > 32).sum() == 1))
    if n < 4096:   # (rows of n - 1: the pinned block of 4096 robots would be 64 MB)
        if n <= 17:   # everybody fits a row of 16: the grid kernel the world started with
            out.append(Step("g", *crowd(n), GRID_16, 16, 1, lambda d: d.max() == n - 1))
        else:
            cap = grown(64 if not big else 32, n - 1)
            out.append(Step("g", *crowd(n), pairs_rows(n), cap, 1 if cap == 64 and not big else 2, lambda d: d.min() == n - 1))
    return out


def degenerate_script(n):
    """step h on a FRESH world: the positions of a and d under radii no grid can take — 0 and -1 (nobody but coincident robots: the
    capacity stays 16), then NaN and inf (everybody); capacity and launches as expected_search says"""
    radii = (0.0, -1.0) if n >= 4096 else (0.0, -1.0, np.nan, np.inf)
    inputs = [("a", sparse(n)[0])] + ([("d", dense(n)[0])] if n >= 63 else [])
    return [(f"h {name} radius {r}", pos, r) for r in radii for name, pos in inputs]


# ---- inputs random positions do not produce ----------------------------------------------------------------------------------
CELL_R = 2.0   # radius of the recipes that place robots by cell


def cells_of(pos, radius):
    c = np.floor(pos[:, [0, 2]].astype(np.float64) / (radius * 1.001))
    return np.clip(c, -2.0 ** 30, 2.0 ** 30).astype(np.int64)


def bucket_of(cx, cz, mask=1023):
    return (((int(cx) * 73856093) & 0xffffffff) ^ ((int(cz) * 19349663) & 0xffffffff)) & mask


def _at(cell, frac):
    return (np.asarray(cell, float) + np.asarray(frac, float)) * (CELL_R * 1.001)


def aliasing(n):
    """clusters in DIFFERENT cells that share one of the 1024 buckets.  Two neighbourhoods in which two of the nine cells around a
    robot collide (the robot stands in the middle, three robots in each of the two cells, all in its range: without the true-cell
    check it would see them twice), and seven pairs of far cells that collide (three robots each).  -> (positions, radius,
    [(cell, cell)] colliding pairs, [centre robots])"""
    near = []   # (centre cell, cell A, cell B): A, B among the nine around the centre, same bucket
    for cx in range(-28, 28):
        for cz in range(-28, 28):
            nine = [(cx + dx, cz + dz) for dx in (-1, 0, 1) for dz in (-1, 0, 1)]
            hit = [(a, b) for i, a in enumerate(nine) for b in nine[i + 1:] if bucket_of(*a) == bucket_of(*b)]
            if hit and all(max(abs(cx - c[0][0]), abs(cz - c[0][1])) >= 6 for c in near):
                near.append(((cx, cz), hit[0][0], hit[0][1]))
    near = [near[0], near[len(near) // 2]]
    assert near[0][0][0] < 0   # (cells on the negative side too)
    taken = {c for t in near for c in ((t[0][0] + dx, t[0][1] + dz) for dx in range(-3, 4) for dz in range(-3, 4))}
    by_bucket, far = {}, []
    for cx in range(-60, 60, 4):        # far cells, four apart: no cluster reaches another
        for cz in range(-60, 60, 4):
            if (cx, cz) in taken or any(max(abs(cx - t[0][0]), abs(cz - t[0][1])) < 6 for t in near):
                continue
            other = by_bucket.setdefault(bucket_of(cx, cz), (cx, cz))
            if other != (cx, cz) and len(far) < 7 and all(other not in p and (cx, cz) not in p for p in far):
                far.append((other, (cx, cz)))
    assert len(far) == 7
    pts, centres = [], []
    for centre, a, b in near:
        centres.append(len(pts))
        pts.append(_at(centre, (0.5, 0.5)))
        for cell in (a, b):
            o = np.array(cell) - np.array(centre)
            for q in (1, 2, 3):   # towards the centre robot: 0.6 cells from it along each axis that differs, a little apart
                pts.append(_at(cell, 0.5 - 0.4 * o + 0.03 * q))
    for a, b in far:
        for cell in (a, b):
            for q in range(3):
                pts.append(_at(cell, (0.3 + 0.2 * q, 0.5)))
    pts = np.array(pts)
    assert len(pts) <= n
    x, z = np.zeros(n), np.zeros(n)
    x[:len(pts)], z[:len(pts)] = pts[:, 0], pts[:, 1]
    x[len(pts):], z[len(pts):] = _isolated(n - len(pts), 3.0 * CELL_R, 80 * CELL_R * 1.001)
    return _xyz(x, z), CELL_R, [(t[1], t[2]) for t in near] + far, centres


def one_lane(n, which):
    """groups of a robot in the middle of a cell and neighbours ONLY in the cells due left, right, up and down of it ("cross":
    the second lane of k_grid_rows finds every hit, the first none) or ONLY in the four corner cells and its own ("corners": the
    other way round); the groups six cells apart on both sides of zero.  -> (positions, radius, [middle robots])"""
    offs = [(-1, 0), (1, 0), (0, -1), (0, 1)] if which == "cross" else [(-1, -1), (-1, 1), (1, -1), (1, 1), (0, 0)]
    groups = min(12, n // (len(offs) + 1))
    pts, middles = [], []
    for g in range(groups):
        cell = (6 * (g % 4) - 12, 6 * (g // 4) - 9)
        middles.append(len(pts))
        pts.append(_at(cell, (0.5, 0.5)))
        for o in offs:
            pts.append(_at(cell, (0.5 + 0.6 * o[0], 0.5 + 0.6 * o[1])) if o != (0, 0) else _at(cell, (0.6, 0.55)))
    pts = np.array(pts)
    x, z = np.zeros(n), np.zeros(n)
    x[:len(pts)], z[:len(pts)] = pts[:, 0], pts[:, 1]
    x[len(pts):], z[len(pts):] = _isolated(n - len(pts), 3.0 * CELL_R, 80 * CELL_R * 1.001)
    return _xyz(x, z), CELL_R, middles


def lattice5(n):
    """the integer lattice under radius 5, cut to n robots and centred on zero: the 3-4-5 pairs sit exactly on the boundary (in
    range), robots exactly on cell edges, rows of 80"""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return _xyz((k % side) - side // 2, (k // side) - (n // side) // 2), 5.0


def non_finite(n, case):
    pos, radius = sparse(n, seed=4000 + n)
    if case == "sprinkle":      # five robots: NaN, +inf and -inf, in x or z
        for r, (axis, v) in zip((3, n // 3, n // 2, n - 7, n - 1), ((0, np.nan), (0, np.inf), (2, -np.inf), (2, np.nan), (2, np.inf))):
            pos[r, axis] = v
    elif case == "infinities":  # no NaN: an infinite robot is out of everyone's range but of those at the same infinity
        for r, (axis, v) in zip((3, n // 3, n // 2, n - 7, n - 1, 11), ((0, np.inf), (0, -np.inf), (2, -np.inf), (2, np.inf), (0, np.inf), (2, np.inf))):
            pos[r, axis] = v
    elif case == "all":         # every distance is NaN: every row is n - 1
        pos[0::2, 0] = np.nan
        pos[1::2, 2] = np.nan
    elif case == "all but one":
        pos[:, 0] = np.nan
        pos[n // 2] = (0.25, 0.5, -0.25)
    return pos, radius


def clamped(n, which):
    if which == "tiny radius":   # every cell clamps to +-2^30 (or is 0): four heavy buckets, rows of coincident robots only
        pos, _ = sparse(n, seed=5000 + n)
        pos[5] = pos[n - 3]
        pos[n // 2] = (0.0, 0.5, 0.0)
        return pos, 1e-30
    pos, radius = sparse(n, seed=6000 + n)   # positions at the end of f32 under radius 1: differences overflow, or are zero
    for q, r in enumerate(range(10, 18)):
        pos[r] = ((3e38, -3e38)[q & 1], 0.5, (3e38, -3e38)[(q >> 1) & 1])
    return pos, radius


def special_inputs(n):
    """[(label, positions, radius)], the ones with short rows first (the row capacity only grows)"""
    out = [("bucket aliasing",) + aliasing(n)[:2], ("one lane: cross",) + one_lane(n, "cross")[:2],
           ("one lane: corners",) + one_lane(n, "corners")[:2], ("non-finite: none",) + non_finite(n, "none"),
           ("non-finite: infinities",) + non_finite(n, "infinities"), ("clamped: tiny radius",) + clamped(n, "tiny radius"),
           ("clamped: end of f32",) + clamped(n, "end of f32"), ("integer lattice, radius 5",) + lattice5(n),
           ("non-finite: sprinkle",) + non_finite(n, "sprinkle"), ("non-finite: all but one",) + non_finite(n, "all but one"),
           ("non-finite: all",) + non_finite(n, "all")]
    return out


SHORT_ROWS = 7   # the first seven of special_inputs have rows of at most 16: the kernel of the world's state answers them


# ---- the recipes through the oracle alone --------------------------------------------------------------------------------------
_WANT = {}


def want_of(n, label, pos, radius):
    key = (n, label)
    if key not in _WANT:
        _WANT[key] = _oracle(n).neighbours(pos, radius)
    return _WANT[key]


@pytest.mark.parametrize("n", SIZES)
def test_recipes_mean_what_they_say(n):
    """the table's conditions on the oracle's result, and that the kernels the steps name are the ones the documented dispatch
    gives for the capacity the script has walked to"""
    cap = 16
    for st in main_script(n):
        d = degrees(want_of(n, st.label, st.pos, st.radius))
        assert st.check(d), (n, st.label, int(d.max()))
        assert n < 63 or all((st.pos[:, a] < 0).any() and (st.pos[:, a] > 0).any() for a in (0, 2))   # (both sides of zero)
        kernel, after, launches = expected_search(n, cap, st.radius, int(d.max()))
        assert (kernel, after) == (st.kernel, st.cap), (n, st.label, NAMES[kernel], after)
        assert launches is None or launches == st.launches, (n, st.label, launches)
        cap = after if n <= 4096 else cap
    cap = 16
    for label, pos, radius in degenerate_script(n):
        d = degrees(want_of(n, label, pos, radius))
        if not radius != radius and radius <= 0:
            assert d.max() == 0                       # nobody (no coincident robots in a or d)
        elif radius != radius:
            assert d.min() == n - 1                   # NaN: `radius < d` is false for everybody
        else:
            assert d.min() == n - 1                   # inf
        kernel, cap, _ = expected_search(n, cap, radius, int(d.max()))
        assert kernel == (TWO_PAIRS if n > 4096 else pairs_rows(n))


@pytest.mark.parametrize("n", [300, 1000])
def test_special_recipes_mean_what_they_say(n):
    pos, radius, pairs, centres = aliasing(n)
    cells = cells_of(pos, radius)
    want = want_of(n, "bucket aliasing", pos, radius)
    rows = rows_of(want)
    occupied = {tuple(c) for c in cells}
    assert len(pairs) >= 8 and all(a != b and bucket_of(*a) == bucket_of(*b) and a in occupied and b in occupied for a, b in pairs)
    for centre, (a, b) in zip(centres, pairs[:2]):   # both colliding cells among the centre robot's nine, their robots in its row
        assert all(max(abs(c[0] - cells[centre][0]), abs(c[1] - cells[centre][1])) <= 1 for c in (a, b))
        in_row = {tuple(cells[j]) for j in rows[centre]}
        assert {a, b} <= in_row | {tuple(cells[centre])} and len(rows[centre]) == 6
    assert degrees(want).max() <= 16
    for which, lane_cells in (("cross", {(-1, 0), (1, 0), (0, -1), (0, 1)}), ("corners", {(-1, -1), (-1, 1), (1, -1), (1, 1), (0, 0)})):
        pos, radius, middles = one_lane(n, which)
        cells, rows = cells_of(pos, radius), rows_of(want_of(n, "one lane: " + which, pos, radius))
        assert len(middles) >= 8 and (cells[middles][:, 0] < 0).any() and (cells[middles][:, 0] > 0).any()
        for m in middles:
            assert {tuple(cells[j] - cells[m]) for j in rows[m]} == lane_cells and len(rows[m]) == len(lane_cells)
    for i, (label, pos, radius) in enumerate(special_inputs(n)):
        d = degrees(want_of(n, label, pos, radius))
        assert (d.max() <= 16) == (i < SHORT_ROWS), (label, int(d.max()))
        assert d.max() >= 1, label
    assert degrees(want_of(n, "integer lattice, radius 5", *lattice5(n))).max() == 80
    for case in ("all", "all but one"):
        assert degrees(want_of(n, "non-finite: " + case, *non_finite(n, case))).min() == n - 1
    assert not np.isfinite(non_finite(n, "all")[0][:, [0, 2]]).all(axis=1).any()
    assert np.isfinite(non_finite(n, "all but one")[0]).all(axis=1).sum() == 1
    pos, radius = clamped(n, "tiny radius")
    assert set(np.unique(np.abs(cells_of(pos, radius)))) == {0, 2 ** 30}
    pos, radius = clamped(n, "end of f32")
    assert (np.abs(cells_of(pos, radius)) == 2 ** 30).all(axis=1).sum() == 8
    d = degrees(want_of(n, "non-finite: infinities", *non_finite(n, "infinities")))
    assert d[3] == 1 and d[n - 1] == 1 and d[n // 3] == 0   # the same infinity: a NaN distance; any other: out of range


# ---- the searches on the device -----------------------------------------------------------------------------------------------
def same_csr(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def search(eng, n, pos, radius, want, kernel, cap, launches, what):
    """ONE AUTO search (a buffer of the oracle's size: more is an error), the kernel it ran asserted, the rows the oracle's"""
    got = eng.neighbours(pos, radius, AUTO, capacity=len(want[1]))
    ran = eng.last_search()
    assert ran[:2] == (kernel, cap) and (launches is None or ran[2] == launches), \
        f"{what}: meant {NAMES[kernel]} cap {cap} in {launches} launch(es), ran {NAMES.get(ran[0], ran[0])} cap {ran[1]} in {ran[2]}"
    assert ran[3] == -1 and ran[4] is None, what   # (no topology pass: no flags)
    TALLY[kernel] += 1
    assert same_csr(got, want), what
    return ran


def run_matrix(n):
    eng = _engine(n)
    assert eng.last_search()[:3] == (hostlib.SEARCH_NONE, 0, 0)
    for st in main_script(n):
        want = want_of(n, st.label, st.pos, st.radius)
        assert st.check(degrees(want)), (n, st.label)   # (the condition, before the device is asked)
        search(eng, n, st.pos, st.radius, want, st.kernel, st.cap, st.launches, f"n = {n}, step {st.label}")
    eng.close()
    eng = _engine(n)   # step h: a fresh world, capacity 16
    cap = 16
    for label, pos, radius in degenerate_script(n):
        want = want_of(n, label, pos, radius)
        kernel, cap, launches = expected_search(n, cap, radius, int(degrees(want).max()))
        assert kernel == (TWO_PAIRS if n > 4096 else pairs_rows(n))
        search(eng, n, pos, radius, want, kernel, cap, launches, f"n = {n}, step {label}")
    eng.close()


_MATRIX_RAN = set()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_search_matrix(n):
    run_matrix(n)
    _MATRIX_RAN.add(n)


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["GRID_16", "GRID_32", "pairs"])
@pytest.mark.parametrize("n", [300, 1000])
def test_special_inputs_in_every_state(n, state):
    """the inputs random positions do not produce, on a world walked to the state that answers with k_grid_rows<16>, <32> or the
    all-pairs rows kernel: the short-row inputs are answered by that kernel in one launch, the long-row ones grow the capacity"""
    eng, cap = _engine(n), 16
    if state != "GRID_16":   # walk there: a hub of 17, or of 33
        pos, radius = hub(n, 17 if state == "GRID_32" else 33)
        want = want_of(n, "walk " + state, pos, radius)
        kernel, cap, launches = expected_search(n, cap, radius, int(degrees(want).max()))
        assert (kernel, cap) == ((GRID_32, 32) if state == "GRID_32" else (pairs_rows(n), 64))
        search(eng, n, pos, radius, want, kernel, cap, launches, f"n = {n}, walking to {state}")
    state_kernel = {"GRID_16": GRID_16, "GRID_32": GRID_32, "pairs": pairs_rows(n)}[state]
    for i, (label, pos, radius) in enumerate(special_inputs(n)):
        want = want_of(n, label, pos, radius)
        kernel, after, launches = expected_search(n, cap, radius, int(degrees(want).max()))
        if i < SHORT_ROWS:
            assert (kernel, after, launches) == (state_kernel, cap, 1), label
        cap = after
        search(eng, n, pos, radius, want, kernel, cap, launches, f"n = {n}, state {state}: {label}")
    eng.close()


# ---- the changed-row flags, directly ------------------------------------------------------------------------------------------
class FlagScript:
    """A world that follows its topology through tracked passes (update_topology) and the transitions that must invalidate the
    rows the device keeps, on the ORACLE: per pass the oracle's results and the flags the engine has to report — a robot is
    changed iff its row differs from its row of the pass before, or it has a non-finite coordinate now or had one then, or the
    pass before did not go through as a tracked pass of a one-pass grid kernel (the first pass included)."""

    def __init__(self, n, radius, walk_to_32):
        self.n, self.radius = n, radius
        sc = S.grid_scenario(n + 1, 10, interrobot=False, obstacles=False)   # (one robot joins on the way)
        self.sc = sc
        self.ref = oracle.OracleWorld(sc["params"])
        S.populate(self.ref, dict(sc, robots=sc["robots"][:n]))
        self.base = np.array([[rb["pos"][0], 0.5, rb["pos"][1]] for rb in sc["robots"]], dtype=F)
        self.rng = np.random.default_rng(31 * n + int(radius * 10))
        self.cap, self.kept, self.prev_rows, self.prev_finite, self.compact, self.nxt = 16, False, None, None, False, 1
        self.events = []   # what the engine replays
        self.churn = []    # share of robots whose oracle row changed, per ordinary pass after the first
        big = 11.5 if radius < 11.5 else 16.5   # rows of 20, of 36
        far_apart = self.base[:, [0, 2]].max() + 100.0
        self.jitter(2 if walk_to_32 else 1)
        self.jitter(3, ordinary=True)
        self.events.append(("untracked", self.positions(), radius))   # an untracked search: the kept rows stay what they are
        self.jitter(2, ordinary=True)
        self.jitter(1, method=GRID)                                            # a pass of the two-pass grid: no flags, nothing kept
        self.jitter(1, all_changed=True)
        self.jitter(2, ordinary=True)
        self.jitter(1, wild=(n // 2, far_apart, np.inf))                       # infinite for one pass: changed then and in the next
        self.jitter(1, was_wild=n // 2)
        self.jitter(2, ordinary=True)
        self.events.append(("add",))
        self.n += 1
        self.ref.add_robot(*[sc["robots"][n][k] for k in ("mean0", "prior_diag", "dt", "radius")], path=None, order_key=n)
        self.kept = False
        self.jitter(1, all_changed=True)
        self.jitter(2, ordinary=True)
        self.jitter(1, radius=big)                                             # a row outgrows the capacity: run again, no flags
        self.jitter(1, radius=big, all_changed=not walk_to_32)                 # (beyond 32 the all-pairs kernel: never flags)
        self.jitter(2, radius=big, ordinary=not walk_to_32)
        self.events.append(("remove", 5))
        self.ref.remove_robot(5)
        self.compact = True
        self.jitter(2, radius=big)                                             # a compact world: no flags
        self.jitter(1, radius=big, wild=(7, 0.0, np.nan))                      # a NaN robot is in everybody's row

    def positions(self):
        pos = self.base[:self.n] + self.rng.normal(0, SIGMA, size=(self.n, 3)).astype(F)
        pos[:, 1] = 0.5
        return pos.astype(F)

    def jitter(self, passes, ordinary=False, method=AUTO, radius=None, wild=None, was_wild=None, all_changed=False):
        radius = self.radius if radius is None else radius
        for _ in range(passes):
            pos = self.positions()
            if wild:
                pos[wild[0]] = (wild[1], 0.5, wild[2])
            want = self.ref.neighbours(pos, radius)
            rows = [r.tolist() for r in rows_of(want)]
            out = self.ref.update_topology(pos, radius, self.nxt)
            self.nxt = out[0]
            conns = [self.ref.connections(r) for r in range(self.n)]
            assert conns == rows or self.compact       # (after a pass a robot's connection set IS its row)
            longest = max(len(r) for r in rows)
            finite = np.isfinite(pos).all(axis=1)
            if method == GRID:
                kernel, cap, launches, flags = TWO_GRID, 0, None, None
            else:
                kernel, cap, launches = expected_search(self.n - (1 if self.compact else 0), self.cap, radius, longest)
                delivered = launches == 1 and kernel in (GRID_16, GRID_32) and not self.compact
                flags = None
                if delivered:
                    flags = np.ones(self.n, np.uint8)
                    if self.kept:
                        flags = np.array([rows[i] != self.prev_rows[i] or not finite[i] or not self.prev_finite[i] for i in range(self.n)], np.uint8)
                self.cap = cap
            if ordinary:
                assert flags is not None and self.kept and finite.all() and self.prev_finite.all()
                self.churn.append(float(flags.mean()))
            if all_changed:
                assert flags is not None and flags.all() and not self.kept
            if was_wild is not None:
                assert flags[was_wild] == 1 and not flags.all()
            if wild and flags is not None:
                assert flags[wild[0]] == 1 and not flags.all()
            self.events.append(("pass", pos, radius, method, out, conns, (kernel, cap, launches), flags))
            self.kept = flags is not None
            self.prev_rows, self.prev_finite = rows, finite


_FLAG_SCRIPTS = {}
SIGMA = 0.04   # jitter per coordinate and pass: the rows of a fifth to a third of the robots change (checked on the oracle)
FLAG_WORLDS = [(200, 7.3, False), (1000, 7.3, False), (1000, 11.5, True)]   # pitch 5: the diagonal at 7.07, the knight's move at 11.18


def flag_script(n, radius, walk_to_32):
    key = (n, radius, walk_to_32)
    if key not in _FLAG_SCRIPTS:
        _FLAG_SCRIPTS[key] = FlagScript(n, radius, walk_to_32)
    return _FLAG_SCRIPTS[key]


@pytest.mark.parametrize("n,radius,walk_to_32", FLAG_WORLDS)
def test_flag_scripts_churn_on_the_oracle(n, radius, walk_to_32):
    """in every ordinary pass the oracle's rows change for between 5 % and 50 % of the robots (a test that passes on no change, or
    on everything changed, says nothing about the flags), and the passes reach the kernel the world is meant for"""
    fs = flag_script(n, radius, walk_to_32)
    assert len(fs.churn) >= 11 and all(0.05 <= c <= 0.5 for c in fs.churn), fs.churn
    passes = [e for e in fs.events if e[0] == "pass"]
    assert len(passes) >= 12
    selective = [e[6][0] for e in passes if e[7] is not None and not e[7].all()]
    assert selective.count(GRID_32 if walk_to_32 else GRID_16) >= 9
    assert walk_to_32 or selective.count(GRID_32) >= 2   # (the GRID_16 worlds walk on to <32> when a row outgrows 16)
    assert sum(1 for e in passes if e[7] is None) >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("n,radius,walk_to_32", FLAG_WORLDS)
def test_changed_row_flags_equal_the_oracles(n, radius, walk_to_32):
    fs = flag_script(n, radius, walk_to_32)
    assert all(0.05 <= c <= 0.5 for c in fs.churn), fs.churn
    sc = fs.sc
    eng = World(sc["params"])
    S.populate(eng, dict(sc, robots=sc["robots"][:n]))
    nxt, n_now = 1, n
    for k, ev in enumerate(fs.events):
        if ev[0] == "untracked":
            eng.neighbours(ev[1], ev[2])
            assert eng.last_search()[3] == -1
        elif ev[0] == "add":
            rb = sc["robots"][n]
            eng.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=None, order_key=n)
            n_now += 1
        elif ev[0] == "remove":
            eng.remove_robot(ev[1])
        else:
            _, pos, r, method, out, conns, (kernel, cap, launches), flags = ev
            got = eng.update_topology(pos, r, nxt, method)
            nxt = got[0]
            what = f"event {k}: {NAMES[kernel]} cap {cap}"
            assert got == out, what
            ran = eng.last_search()
            assert ran[:2] == (kernel, cap) and (launches is None or ran[2] == launches), (what, ran[:3])
            TALLY[kernel] += 1
            if flags is None:
                assert ran[3] == -1 and ran[4] is None, what
            else:
                assert ran[4] is not None and len(ran[4]) == n_now, what
                missed = np.nonzero((flags == 1) & (ran[4] == 0))[0]      # a connection or disconnection the pass never sees
                spurious = np.nonzero((flags == 0) & (ran[4] == 1))[0]    # the feature not working
                assert len(missed) == 0 and len(spurious) == 0, (what, missed[:8], spurious[:8])
                assert ran[3] == int(flags.sum())
            assert [eng.connections(q) for q in range(n_now)] == conns, what
    eng.close()


# ---- the cross-check at <32> with churn ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_topology_differences_are_cross_checked_at_rows_of_32():
    """tests/topology_check_worker.py under comms radius 11.5: about 20 neighbours per interior robot, the lattice distances 11.18
    and 14.14 on either side of the radius under the jitter — with MGX_CHECK_INDEX on, every row k_grid_rows<32> calls unchanged
    is compared with the robot's connection set by the pass.  (The robot that leaves goes after tick 9: a world with a removed
    robot gets no flags.)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "topology_check_worker.py"), "300", "12", "11.5", "9"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "OK 300 robots" in out, out[-3000:]
    line = next(ln for ln in out.splitlines() if ln.startswith("searches:"))
    print(line)
    kernels = {int(k): int(v) for k, v in (kv.split("=") for kv in line.split()[1].split(","))}
    flagged = {int(k): int(v) for k, v in (kv.split("=") for kv in line.split()[3].split(","))}
    assert GRID_32 in kernels and flagged.get(GRID_32, 0) >= 8, line
    TALLY[GRID_32] += 1


# ---- the tally ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_search_kernel_was_asserted():
    """one line: how often each of the six kernel codes was asserted by the tests of this file (the sizes that cover them are run
    here if this test runs without the others)"""
    for n in (65, 513, 4097):
        if n not in _MATRIX_RAN:
            run_matrix(n)
            _MATRIX_RAN.add(n)
    print("search kernels asserted: " + ", ".join(f"{NAMES[k]} x {TALLY[k]}" for k in sorted(NAMES)))
    assert all(TALLY[k] > 0 for k in NAMES), dict(TALLY)
