"""What the four observers share on the host (magics_amd/csrc/mgx_world_observers.inc: one radii array, one staged pair of positions
and flags, one growth rule, one "sharded" flag) against the host restatements in magics_amd/sim.py — `_collide`,
`environment_contacts`, `goal_area_contacts`, `_track`, through the checkers of the observers' own tests: updates of different
observers back to back, robots that join with all four on, an observer switched on late, one switched off, worlds with ghosts,
and robots that join between the two halves of a tick.  Integers and records, compared for equality."""
import numpy as np
import pytest

from magics_amd import World, hostlib, scenarios as S, sim

from test_gpu_collisions import Checker as CollChecker, _device_events as _coll_events
from test_gpu_env_collisions import Checker as EnvChecker, _add, _device_events as _env_events, _scenario, _xyz
from test_gpu_goal_areas import _table
from test_gpu_tracks import PERIOD, Checker as TrackChecker, _device_samples

pytestmark = pytest.mark.gpu
F = np.float32
ALL = ("coll", "env", "goals", "trk")
WALL_LO, WALL_HI = 0, 1                                 # the map's two colliders: z in [-50, -25] and z in [25, 50]
AREAS = [((-34, -4), (-26, 4)), ((30, -4), (38, 4))]
COLL_TEXT, TRK_TEXT, GOAL_TEXT = "collision bookkeeping runs on unsharded worlds", "the trackers run on unsharded worlds", "the goal areas run on unsharded worlds"


def _walls():
    """one tile of road between two walls and nothing else: cuboids, and every coordinate below a multiple of 0.5 — no contact
    within rounding of tangency"""
    env = _scenario("Obstacle Shapes Showcase")["environment"]
    env["tiles"]["grid"], env["obstacles"] = ["─"], []
    env["tiles"]["settings"]["path-width"] = 0.5
    return env


class GoalChecker:
    """sim.goal_area_contacts pass by pass: (robot, area) -> the tick of the first contact"""

    def __init__(self, areas):
        self.areas, self.first = areas, {}

    def step(self, tick, ids, radii, pos):
        ids = np.asarray(ids, dtype=np.int64)
        hit = sim.goal_area_contacts(self.areas, np.asarray(pos, F)[ids][:, [0, 2]], np.asarray(radii, F)[ids])
        for i, a in zip(*np.nonzero(hit)):
            self.first.setdefault((int(ids[i]), int(a)), int(tick))

    def table(self, n):
        t = np.full((n, len(self.areas)), -1, np.int64)
        for (r, a), tick in self.first.items():
            t[r, a] = tick
        return t


def _checker(what, env, n, areas=AREAS):
    return {"coll": CollChecker, "env": lambda: EnvChecker(env), "goals": lambda: GoalChecker(areas), "trk": lambda: TrackChecker(n, PERIOD)}[what]()


def _step(chk, what, tick, radii, pos, moved=None):
    ids = list(range(len(radii)))
    if what == "goals":
        chk.step(tick, ids, radii, pos)
    elif what == "trk":
        chk.step(tick, ids if moved is None else np.nonzero(moved)[0], pos)
    else:
        chk.step(ids, radii, pos)


def _answer(chk, what):
    """what a checker has seen, without the pass numbers: (a, b) of its events, (robot, area) -> tick, or its samples"""
    return sorted(chk.first.items()) if what == "goals" else chk.samples if what == "trk" else [e[1:3] for e in chk.events]


class Four:
    """a world, the observers asked for switched on, and a host checker beside each"""

    def __init__(self, radii, on=ALL):
        self.env, self.radii, self.chk, self.taken = _walls(), [float(r) for r in radii], {}, 0
        self.w = World(S.JUNCTION_PARAMS)
        for r in self.radii:
            _add(self.w, r)
        for what in on:
            self.enable(what)

    def enable(self, what):
        if what == "coll":
            self.w.collisions_enable(True)
        elif what == "env":
            self.w.env_collisions_enable(self.env)
        elif what == "goals":
            self.w.goal_areas_enable(AREAS, next_tick=0)
        else:
            self.w.tracks_enable(True, period_ns=PERIOD, tick_ns=PERIOD, next_tick=0)
        self.chk[what] = _checker(what, self.env, len(self.radii))

    def join(self, radii):
        for r in radii:
            _add(self.w, r)
            self.radii.append(float(r))
        if "trk" in self.chk:
            self.chk["trk"].grow(len(self.radii))

    def update(self, what, tick, pos, moved=None):
        """one pass of one observer over `pos`, enqueued — nothing read, nothing waited for — and the checker's step beside it"""
        if what == "coll":
            self.w.collisions_update(pos)
        elif what == "env":
            self.w.env_collisions_update(pos)
        elif what == "goals":
            self.w.goal_areas_update(tick, pos)
        else:
            self.w.tracks_update(tick, pos, moved)
        _step(self.chk[what], what, tick, self.radii, pos, moved)

    def check(self, what):
        """the device's answer is the checker's (the trackers: the samples since the last check)"""
        n, chk = len(self.radii), self.chk[what]
        if what == "coll":
            ev, total, dropped, per = self.w.collisions_read()
            assert (total, dropped) == (len(chk.events), 0) and _coll_events(ev) == chk.events and np.array_equal(per, chk.per_robot(n))
        elif what == "env":
            ev, total, dropped, per = self.w.env_collisions_read()
            assert (total, dropped) == (len(chk.events), 0) and _env_events(ev) == chk.events and np.array_equal(per, chk.per_robot(n))
        elif what == "goals":
            assert np.array_equal(_table(self.w, len(AREAS), n), chk.table(n))
        else:
            got, _, dropped, _ = self.w.tracks_take()
            assert dropped == 0 and _device_samples(got) == chk.samples[self.taken:]
            self.taken = len(chk.samples)
        return chk


# ---- the robots of the tests below: three old ones, radius 1, and newcomers of radius 2 whose contacts need that radius ----------------
OLD = {0: (-30.0, 0.0), 1: (-28.5, 0.0), 2: (0.0, 24.5)}   # a pair that overlaps inside area 0; one robot at the upper wall
# newcomers that touch something with their own radius 2 and would not with a stale 1 or a missing 0, some in each wave of joins:
# (at a wall, one of a pair, the other, at an area's edge)
NEW = {3: (10.0, 23.5), 4: (20.0, 0.0), 5: (23.5, 0.0), 6: (-35.5, 0.0),
       40: (-10.0, -23.5), 41: (32.0, 5.5), 42: (-15.0, 0.0), 43: (-11.5, 0.0),
       90: (-40.0, 23.5), 91: (39.5, 0.0), 92: (5.0, 0.0), 93: (8.5, 0.0)}
# 3 robots, grown to 90 in two steps: both fit the room the first sizing leaves (3 + 3 / 4 + 64, rounded up to a multiple of 64: 128),
# so a third step goes past it
WAVES = (3, 40, 90, 140)


def _crowd(n=WAVES[-1]):
    """radii [n] and positions [n, 3]: OLD, NEW, and between them robots that stand clear of those"""
    special = {**OLD, **NEW}
    spots = [(-47.5 + 5.0 * c, z) for z in (-20.0, -15.0, -10.0, 10.0, 15.0, 20.0, -5.0, 5.0) for c in range(20)]
    free = iter(p for p in spots if all(np.hypot(p[0] - q[0], p[1] - q[1]) > 5.0 for q in special.values()))
    points = [special[i] if i in special else next(free) for i in range(n)]
    return np.array([1.0 if i in OLD else 2.0 for i in range(n)], F), _xyz(points)


def test_the_crowd_means_what_it_says():
    """(the host's arithmetic alone) every designed contact holds with radius 2 and fails with radius 1"""
    radii, pos = _crowd()
    xz = pos[:, [0, 2]]
    cols, verts = hostlib.env_colliders(_walls())
    assert len(cols) == 2 and cols["maxs"][WALL_LO][1] == -25.0 and cols["mins"][WALL_HI][1] == 25.0
    for r, want in ((2.0, True), (1.0, False)):
        rad = np.where(np.isin(np.arange(len(radii)), list(NEW)), F(r), radii).astype(F)
        env, goal = sim.environment_contacts(cols, verts, xz, rad), sim.goal_area_contacts(AREAS, xz, rad)
        assert [bool(env[3, WALL_HI]), bool(env[40, WALL_LO]), bool(env[90, WALL_HI])] == [want] * 3
        assert [bool(goal[6, 0]), bool(goal[41, 1]), bool(goal[91, 1])] == [want] * 3
        for a, b in ((4, 5), (42, 43), (92, 93)):
            assert bool(np.hypot(*(xz[a] - xz[b])) <= rad[a] + rad[b]) == want
    assert env[2, WALL_HI] and goal[0, 0] and goal[1, 0] and np.hypot(*(xz[0] - xz[1])) <= 2.0


# ---- 1. updates of different observers, back to back ----------------------------------------------------------------------------------
def _four_position_sets():
    """P1 .. P4 for three robots of radius 1: who overlaps, who touches the wall and who stands in area 0 differ from set to set"""
    A, A2, W, O, O2, O3 = (-30.0, 0.0), (-28.5, 0.0), (0.0, 24.5), (10.0, 0.0), (11.5, 0.0), (20.0, 10.0)
    return dict(zip(ALL, (_xyz(p) for p in ([O, O2, W], [W, A, A2], [A, W, A2], [A, O, O3]))))


def _alone(what, pos, moved):
    chk = _checker(what, _walls(), 3)
    _step(chk, what, 0, [1.0] * 3, pos, moved)
    return _answer(chk, what)


@pytest.mark.parametrize("order", [ALL, ALL[::-1]], ids=["forward", "reverse"])
def test_back_to_back_updates_each_read_their_own_positions(order):
    P, moved = _four_position_sets(), np.array([1, 0, 1], np.uint8)
    for what in ALL:                                     # every observer's answer to its own positions is no answer to the others'
        own = _alone(what, P[what], moved)
        assert own and all(_alone(what, P[other], moved) != own for other in ALL if other != what), what
    f = Four([1.0] * 3)
    for what in order:                                   # no read, no synchronisation in between
        f.update(what, 0, P[what], moved if what == "trk" else None)
    for what in order:
        f.check(what)
    assert _answer(f.chk["coll"], "coll") == [(0, 1)] and _answer(f.chk["env"], "env") == [(0, WALL_HI)]
    assert sorted(f.chk["goals"].first) == [(0, 0), (2, 0)] and [s[1] for s in f.chk["trk"].samples] == [0, 2]


# ---- 2. robots that join with all four on -------------------------------------------------------------------------------------------
def test_robots_join_with_all_four_on():
    radii, pos = _crowd()
    f = Four(radii[:WAVES[0]])
    for tick, n in enumerate(WAVES):
        f.join(radii[len(f.radii):n])
        for what in ALL:
            f.update(what, tick, pos[:n])
        for what in ALL:
            f.check(what)
    coll, env = ([e[:3] for e in f.chk[k].events] for k in ("coll", "env"))
    goals, samples = f.chk["goals"].first, f.chk["trk"].samples
    # what the first three held is logged once; the newcomers' contacts come with the pass they joined in, under their own radii
    assert [e for e in coll if e[1] < 3 and e[2] < 3] == [(0, 0, 1)] and [e for e in env if e[1] < 3] == [(0, 2, WALL_HI)]
    assert {(1, 4, 5), (2, 42, 43), (3, 92, 93)} <= set(coll) and {(1, 3, WALL_HI), (2, 40, WALL_LO), (3, 90, WALL_HI)} <= set(env)
    assert (goals[(0, 0)], goals[(1, 0)], goals[(6, 0)], goals[(41, 1)], goals[(91, 1)]) == (0, 0, 1, 2, 3)
    # the trackers' state moved along: a first sample (span 0) in the wave a robot joined in, and span 1 ever after
    joined = {r: min(k for k, n in enumerate(WAVES) if r < n) for r in range(WAVES[-1])}
    assert len(samples) == sum(WAVES) and all(s[4] == (0 if s[0] == joined[s[1]] else 1) for s in samples)


# ---- 3. an observer switched on late finds the radii there --------------------------------------------------------------------------
def test_late_enable():
    radii, pos = _crowd(WAVES[2])
    f = Four(radii, on=("coll",))
    f.update("coll", 0, pos)
    f.enable("goals")
    f.enable("env")
    for what in ("goals", "env", "coll"):
        f.update(what, 1, pos)
    for what in ("goals", "env", "coll"):
        f.check(what)
    assert {(4, 5), (42, 43)} <= set(_answer(f.chk["coll"], "coll")) and {(3, WALL_HI), (40, WALL_LO)} <= set(_answer(f.chk["env"], "env"))
    assert {(6, 0), (41, 1)} <= set(f.chk["goals"].first)


# ---- 4. one switched off, the others go on ------------------------------------------------------------------------------------------
def test_switch_one_off_keep_the_others():
    radii, pos = _crowd(WAVES[1])
    f = Four(radii)
    for what in ALL:
        f.update(what, 0, pos)
    f.w.env_collisions_enable(None)
    with pytest.raises(hostlib.MgxError, match=r"environment collision bookkeeping is off \(mgx_env_collisions_enable\)"):
        f.w.env_collisions_update(pos)
    parted = pos.copy()
    parted[4] = _xyz([(20.0, -40.0)])[0]                 # the pair (4, 5) parts
    for tick, p in ((1, parted), (2, pos)):              # ... and meets again: a second event, under radii nobody uploaded again
        for what in ("coll", "goals", "trk"):
            f.update(what, tick, p)
    for what in ("coll", "goals", "trk"):
        f.check(what)
    assert [e[0] for e in f.chk["coll"].events if e[1:3] == (4, 5)] == [0, 2]
    f.enable("env")                                      # on again: from everybody Free, against a fresh checker
    f.update("env", 0, pos)
    assert {(2, WALL_HI), (3, WALL_HI)} <= set(_answer(f.check("env"), "env"))


# ---- 5. a world with ghosts is refused by every observer, in its own words ------------------------------------------------------------
def test_a_world_with_ghosts_is_refused_by_every_observer():
    for what, text in zip(ALL, (COLL_TEXT, COLL_TEXT, GOAL_TEXT, TRK_TEXT)):     # _enable on a world that has a ghost
        f = Four([1.0], on=())
        _add(f.w, 1.0, ghost=True)
        with pytest.raises(hostlib.MgxError, match=text):
            f.enable(what)
    f = Four([1.0])
    _add(f.w, 1.0, ghost=True)                                                   # _update on a world that got one later
    for update, text in ((f.w.collisions_update, COLL_TEXT), (f.w.env_collisions_update, COLL_TEXT),
                         (lambda: f.w.goal_areas_update(0), GOAL_TEXT), (lambda: f.w.tracks_update(0), TRK_TEXT)):
        with pytest.raises(hostlib.MgxError, match=text):
            update()
    # a robot given away is a ghost here, taken back it is none: mgx_robot_release and mgx_robot_import keep the flag too
    g = Four([1.0, 1.0], on=("goals",))
    record = g.w.robot_export(1)
    g.w.robot_release(1)
    with pytest.raises(hostlib.MgxError, match=GOAL_TEXT):
        g.w.goal_areas_update(0)
    g.w.robot_import(1, record)
    g.w.goal_areas_update(0, _xyz([(-30.0, 0.0), (34.0, 0.0)]))
    assert _table(g.w, 2, 2).tolist() == [[0, -1], [-1, 0]]


# ---- 6. robots that join between the two halves of a tick, all four on --------------------------------------------------------------
@pytest.mark.parametrize("reserve", [True, False], ids=["appended", "relayout"])
def test_a_robot_joins_between_the_two_halves_of_a_tick_with_all_four_on(reserve):
    """tests/test_gpu_tracks_join.py's case with the two contact books and the goal areas on as well: their passes of the tick the
    robot joined in look at it too, over the Transforms the mission chain has just moved (area 1 holds the whole circle)"""
    n, K, ticks, join = 6, 10, 12, 5
    sc = S.circle_scenario(n, K, circle_radius=12.0, n_internal=10, n_external=10)
    sc["ir"] = []
    w = World(sc["params"])
    if reserve:
        w.reserve(n + 2)
    assert S.populate(w, dict(sc, robots=sc["robots"][:n - 1])) == list(range(n - 1))
    dt32 = F(1.0) / F(10.0)
    ts = np.array([float(dt32 / F(rb["t0"])) for rb in sc["robots"]])
    radii, env, areas = [float(rb["radius"]) for rb in sc["robots"]], _walls(), [((-3, -3), (3, 3)), ((-20, -20), (20, 20))]

    def mission(r):
        rb = sc["robots"][r]
        r2, cur = float(F(rb["radius"]) * F(rb["radius"])), rb["mean0"][0]
        w.mission_set(r, np.asarray([tuple(rb["goal"])], dtype=np.float64), K - 1, 0, r2, r2, (F(cur[0]), F(0.5), F(cur[1])), ts[r])
    for r in range(n - 1):
        mission(r)
    w.tracks_enable(True, period_ns=PERIOD, tick_ns=PERIOD, next_tick=0)
    w.collisions_enable(True)
    w.env_collisions_enable(env)
    w.goal_areas_enable(areas, next_tick=0)
    own, nn = np.zeros(n), 1
    chk = {what: _checker(what, env, n, areas) for what in ALL}
    for k in range(ticks):
        m0, m1 = w.read_variable_means(0), w.read_variable_means(1)
        old = np.arange(len(m0))
        nn, _, _, fin = w.mission_tick_begin(12.0, nn)
        assert not len(fin)
        if k == join:
            rb = sc["robots"][n - 1]
            assert w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=rb["order_key"]) == n - 1
            mission(n - 1)
        w.mission_tick_end(sc["steps"], float(F(sc["target_speed"])), float(dt32))
        change = ts[old, None] * (m1[old] - m0[old])
        own[old] += np.sqrt(change[:, 0] * change[:, 0] + change[:, 1] * change[:, 1])      # (driver.py, Driver.tick)
        tr = np.zeros((n, 3), F)
        got = w.mission_read()[0]
        tr[:len(got)] = got
        if k == join:  # the newcomer moved in the tick it joined: its first increment, as far as its Transform shows it
            start = np.array([sc["robots"][n - 1]["mean0"][0][0], sc["robots"][n - 1]["mean0"][0][1]])
            moved = float(np.hypot(float(tr[n - 1, 0]) - start[0], float(tr[n - 1, 2]) - start[1]))
            samples, in_log, dropped, dist = w.tracks_take(capacity=0)               # (too little room: nothing is taken)
            assert len(samples) == 0 and in_log == (n - 1) * (join + 1) + 1 and dropped == 0
            assert moved > 0 and abs(dist[n - 1] - moved) <= 1e-4 * moved
            own[n - 1] = dist[n - 1]
        alive = n - 1 if k < join else n
        for what in ALL:
            _step(chk[what], what, k, radii[:alive], tr)
    got, in_log, dropped, dist = w.tracks_take()
    samples = chk["trk"].samples
    assert dropped == 0 and _device_samples(got) == samples
    assert np.array_equal(dist, own) and (dist > 0).all()
    new = [s for s in samples if s[1] == n - 1]
    assert new[0][0] == join and new[0][4] == 0 and all(s[4] == 1 for s in new[1:])
    assert all(s[4] == 1 for s in samples if s[1] < n - 1 and s[0] > 0)                  # nobody else started again
    ev, total, dropped, per = w.collisions_read()
    assert (total, dropped) == (len(chk["coll"].events), 0) and _coll_events(ev) == chk["coll"].events
    assert np.array_equal(per, chk["coll"].per_robot(n))
    ev, total, dropped, per = w.env_collisions_read()
    assert (total, dropped) == (len(chk["env"].events), 0) and _env_events(ev) == chk["env"].events
    assert np.array_equal(per, chk["env"].per_robot(n))
    assert np.array_equal(_table(w, len(areas), n), chk["goals"].table(n))
    assert [chk["goals"].first[(r, 1)] for r in range(n)] == [0] * (n - 1) + [join]       # the goal areas saw the newcomer when it joined
    appends = w.append_stats()
    assert appends[0] >= 1 if reserve else appends[:2] == (0, 0), appends
