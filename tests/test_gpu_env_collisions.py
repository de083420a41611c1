"""Robot-environment collision bookkeeping on the device (mgx_env_collisions_*, magics_amd/csrc/mgx_collisions.hip) against
the host pass `sim.Simulation._collide_environment` (the contact include/mgx.h specifies, over hostlib.env_colliders): same
(pass, robot, collider) events, AABBs equal as f32 bit patterns, same per-robot counts — a scripted state machine, crowds of a
thousand over three maps with both libraries, inside the mission chain tick by tick and many ticks per call, with a full
log, with more simultaneous contacts than the device remembers, with a radius larger than a tile, and switched off.

Crowd positions keep 2e-3 world units away from tangency to every collider, judged by an f64 checker of the geometry written
below (`signed_gap`): offenders are redrawn before either side sees them, so the f32 contact and the exact one agree on
every sample and no sample is skipped."""
import ctypes
import json
import os

import numpy as np
import pytest

from magics_amd import World, config, environment, hostlib, scenarios, sim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BALL, CUBOID, POLYGON = hostlib.COLLIDER_BALL, hostlib.COLLIDER_CUBOID, hostlib.COLLIDER_POLYGON
KIND_NAMES = {BALL: "ball", CUBOID: "cuboid", POLYGON: "polygon"}


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _scenario(name):
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)[name]


def signed_gap(cols, verts, pos, rad):
    """f64: [n, m] (distance from robot i's centre to collider j's boundary, negative inside) - r_i: a contact iff <= 0, and
    its absolute value is how far the robot is from tangency"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    x, z = p[:, 0:1], p[:, 1:2]
    sd = np.full((len(p), len(cols)), np.inf)
    b = np.nonzero(cols["kind"] == BALL)[0]
    if len(b):
        sd[:, b] = np.hypot(x - cols["tx"][b].astype(np.float64)[None], z - cols["tz"][b].astype(np.float64)[None]) - cols["radius"][b].astype(np.float64)[None]
    c = np.nonzero(cols["kind"] == CUBOID)[0]
    if len(c):
        h = cols["half_extents"][c].astype(np.float64)
        dx = np.abs(x - cols["tx"][c].astype(np.float64)[None]) - h[None, :, 0]
        dz = np.abs(z - cols["tz"][c].astype(np.float64)[None]) - h[None, :, 1]
        sd[:, c] = np.where((dx <= 0) & (dz <= 0), np.maximum(dx, dz), np.hypot(np.maximum(dx, 0), np.maximum(dz, 0)))
    for j in np.nonzero(cols["kind"] == POLYGON)[0]:
        a = verts[int(cols["first_vertex"][j]):int(cols["first_vertex"][j]) + int(cols["n_vertices"][j])].astype(np.float64)
        e = np.roll(a, -1, axis=0) - a
        q = p[:, None, :] - a[None]
        t = np.clip((q * e[None]).sum(axis=2) / (e * e).sum(axis=1)[None], 0.0, 1.0)
        d = np.linalg.norm(q - t[..., None] * e[None], axis=2).min(axis=1)
        inside = (e[None, :, 0] * q[..., 1] - e[None, :, 1] * q[..., 0] >= 0).all(axis=1)
        sd[:, j] = np.where(inside, -d, d)
    return sd - np.asarray(rad, dtype=np.float64)[:, None]


class Checker:
    """the host pass on a bare Simulation, and the events it makes: (pass, robot, collider, mins bits, maxs bits)"""

    def __init__(self, env):
        self.s = sim.Simulation.__new__(sim.Simulation)
        self.s._env_coll, self.s._dev_env_coll, self.s._env_collisions = True, False, {}
        self.cols, self.verts = self.s._colliders, self.s._collider_vertices = hostlib.env_colliders(env)
        self.events, self.seen, self.n_pass = [], {}, 0
        self.hits, self.ends = {k: 0 for k in KIND_NAMES}, {k: 0 for k in KIND_NAMES}

    def step(self, ids, radii, pos):
        before = {k for k, h in self.s._env_collisions.items() if h["colliding"]}
        self.s._collide_environment([{"id": int(i), "radius": F(radii[i])} for i in ids], pos)
        fresh = []
        for (a, k), h in self.s._env_collisions.items():
            n = self.seen.get((a, k), 0)
            assert len(h["aabbs"]) - n in (0, 1)
            if len(h["aabbs"]) > n:
                box = h["aabbs"][-1]
                fresh.append((self.n_pass, a, k, tuple(_bits(v) for v in box["mins"]), tuple(_bits(v) for v in box["maxs"])))
                self.seen[(a, k)] = n + 1
                self.hits[int(self.cols["kind"][k])] += 1
            if (a, k) in before and not h["colliding"]:
                self.ends[int(self.cols["kind"][k])] += 1
        self.events += sorted(fresh)
        self.n_pass += 1
        return len(fresh)

    def per_robot(self, n):
        out = np.zeros(n, np.uint32)
        for (a, _), h in self.s._env_collisions.items():
            out[a] += h["times"]
        return out


def _device_events(ev):
    return [(int(e["pass"]), int(e["robot"]), int(e["collider"]), tuple(_bits(v) for v in e["mins"]), tuple(_bits(v) for v in e["maxs"])) for e in ev]


def _bare_world(radii, fma=None):
    """robots that only stand for their radii (the passes below get their positions handed in)"""
    w = World(scenarios.JUNCTION_PARAMS, fma=fma)
    for r in radii:
        _add(w, r)
    return w


def _add(w, radius, ghost=False):
    mean0, prior, dt = scenarios.robot_initial_state((0.0, 0.0, 5.0, 0.0), (10.0, 0.0, 5.0, 0.0), scenarios.timesteps_for_K(10), 1.0, 5.0, 5.0)
    return w.add_robot(mean0, prior, dt, float(radius), ghost=ghost)


def _xyz(points):
    pos = np.zeros((len(points), 3), F)
    pos[:, 0], pos[:, 1], pos[:, 2] = [p[0] for p in points], -1.5, [p[1] for p in points]
    return pos


# ---- 4. the state machine, literally ------------------------------------------------------------------------------------------
def test_state_machine_along_a_scripted_line():
    env = _scenario("Obstacle Shapes Showcase")["environment"]
    env["tiles"]["grid"] = ["─"]                       # a tile with walls: z in [25, 50] and [-50, -25]
    env["tiles"]["settings"]["path-width"] = 0.5
    chk = Checker(env)
    cols, verts = chk.cols, chk.verts
    wall = 1
    circle = int(np.nonzero(cols["kind"] == BALL)[0][0])
    tri = len(cols) - 1                                # the last obstacle: the triangle with rotation 5.2
    assert list(cols["kind"][:2]) == [CUBOID, CUBOID] and list(cols["obstacle"][:2]) == [-1, -1] and cols["mins"][wall][1] == 25.0
    assert env["obstacles"][cols["obstacle"][tri]]["shape"]["kind"] == "triangle" and env["obstacles"][cols["obstacle"][tri]]["rotation"] == 5.2
    assert cols["n_vertices"][tri] == 3
    T = tuple(verts[cols["first_vertex"][tri]:cols["first_vertex"][tri] + 3].astype(np.float64).mean(axis=0))
    Fr, W, Cc = (-30.0, 0.0), (0.0, 40.0), (float(cols["tx"][circle]), float(cols["tz"][circle]))
    for point, touched in ((Fr, []), (W, [wall]), (Cc, [circle]), (T, [tri])):   # the script means what it says
        gap = signed_gap(cols, verts, [point], [1.0])[0]
        assert list(np.nonzero(gap <= 0)[0]) == touched and (np.abs(gap) > 0.05).all()
    script = [(Fr, None), (W, None), ((0.5, 40.5), None), (Fr, None), (W, None), (Cc, None), ((Cc[0] + 1.0, Cc[1]), None), (Fr, None),
              (T, None), (T, None), (T, "despawn"), (T, "re-add"), (T, None)]
    expected = [(1, 0, wall), (4, 0, wall), (5, 0, circle), (8, 0, tri), (11, 1, tri)]
    w = _bare_world([1.0])
    w.env_collisions_enable(env)
    radii, alive = [1.0], [0]
    for point, what in script:
        if what == "despawn":
            w.remove_robot(0)
            alive = []
        elif what == "re-add":
            assert _add(w, 1.0) == 1
            radii, alive = [1.0, 1.0], [1]
        pos = _xyz([point] * len(radii))
        w.env_collisions_update(pos)
        chk.step(alive, radii, pos)
    ev, total, dropped, per = w.env_collisions_read()
    assert [(int(e["pass"]), int(e["robot"]), int(e["collider"])) for e in ev] == expected
    assert (total, dropped, list(per)) == (5, 0, [4, 1])
    assert _device_events(ev) == chk.events
    assert np.array_equal(per, chk.per_robot(2))
    first = ev[0]                                      # robot_aabb intersected with the wall's AABB
    assert list(first["mins"]) == [-1.0, 39.0] and list(first["maxs"]) == [1.0, 41.0]
    w.env_collisions_clear()                           # everybody Free, log empty, pass 0
    w.env_collisions_update(_xyz([T, T]))
    ev, total, _, per = w.env_collisions_read()
    assert total == 1 and (int(ev[0]["pass"]), int(ev[0]["robot"]), int(ev[0]["collider"])) == (0, 1, tri) and list(per) == [0, 1]


# ---- 5. crowds ----------------------------------------------------------------------------------------------------------------
def _cross_grid():
    return environment.new(["┼" * 20] * 20, 0.4, 1.0, 10.0)


_MAPS = {
    # name: (environment, half side of the square the crowd lives in, radii, step of the walk)
    "obstacles": (lambda: _scenario("Environment Obstacles Experiment")["environment"], 32.0, (0.5, 3.0), 1.0),
    "showcase": (lambda: _scenario("Obstacle Shapes Showcase")["environment"], 48.0, (0.5, 3.0), 1.0),
    "cross-grid": (_cross_grid, 100.0, (0.3, 1.6), 0.5),
}
TANGENCY = 2e-3


def _crowd(which, n=1000, seed=5, passes=30):
    """[(alive ids, positions [n, 3])], radii, environment: a random walk whose every sample keeps TANGENCY away from tangency
    to every collider (f64 checker); offenders are drawn again before anybody sees them"""
    make, side, (r0, r1), step = _MAPS[which]
    env = make()
    cols, verts = hostlib.env_colliders(env)
    rng = np.random.default_rng(seed)
    radii = rng.uniform(r0, r1, n).astype(F)

    def settle(draw):
        p = draw(np.arange(n))
        for _ in range(100):
            bad = np.nonzero((np.abs(signed_gap(cols, verts, p.astype(np.float64), radii.astype(np.float64))) < TANGENCY).any(axis=1))[0]
            if not len(bad):
                return p
            p[bad] = draw(bad)
        raise AssertionError("could not draw positions away from tangency")
    p = settle(lambda ids: rng.uniform(-side, side, (len(ids), 2)).astype(F))
    alive = np.ones(n, bool)
    out = []
    for k in range(passes):
        if k == 10:
            alive[rng.choice(n, n // 20, replace=False)] = False
        pos = _xyz(p)
        if k >= 5:
            pos[3, 0] = np.nan                          # a robot that is nowhere touches nothing
        out.append((np.nonzero(alive)[0], pos))
        last = p.copy()
        p = settle(lambda ids: (last[ids] + rng.normal(0.0, step, (len(ids), 2)).astype(F)).astype(F))
    return out, radii, env


_CHECKED = {}


def _crowd_checked(which):
    if which not in _CHECKED:
        passes, radii, env = _crowd(which)
        chk = Checker(env)
        per_pass = [chk.step(ids, radii, pos) for ids, pos in passes]
        _CHECKED[which] = (passes, radii, env, chk, per_pass)
    return _CHECKED[which]


def _run_crowd(w, passes):
    gone = set()
    for ids, pos in passes:
        for r in sorted(set(range(len(pos))) - set(int(i) for i in ids) - gone):
            w.remove_robot(r)
            gone.add(r)
        w.env_collisions_update(pos)


@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
@pytest.mark.parametrize("which", sorted(_MAPS))
def test_crowd_of_a_thousand_equals_the_host_pass(which, fma):
    passes, radii, env, chk, per_pass = _crowd_checked(which)
    kinds = sorted(set(int(k) for k in chk.cols["kind"]))
    print(f"{which}: {len(chk.cols)} colliders, {len(chk.events)} events; hits {chk.hits}, Colliding -> Free edges {chk.ends}")
    for k in kinds:                                     # (the test cannot pass on an empty log)
        assert chk.hits[k] >= 1 and chk.ends[k] >= 1, KIND_NAMES[k]
    w = _bare_world(radii, fma=fma)
    w.env_collisions_enable(env)
    _run_crowd(w, passes)
    ev, total, dropped, per = w.env_collisions_read()
    assert (total, dropped) == (len(chk.events), 0)
    assert _device_events(ev) == chk.events
    assert np.array_equal(per, chk.per_robot(len(radii)))
    again, _, _, _ = w.env_collisions_read(first=total - 7)                 # a cursor into the log
    assert _device_events(again) == chk.events[-7:]


def test_the_three_maps_cover_every_collider_kind():
    seen = set()
    for which in _MAPS:
        chk = _crowd_checked(which)[3]
        seen |= {k for k in KIND_NAMES if chk.hits[k] and chk.ends[k]}
    assert seen == set(KIND_NAMES)


# ---- 6. inside the mission chain ----------------------------------------------------------------------------------------------
def _blind_obstacles():
    sc = _scenario("Environment Obstacles Experiment")
    sc["config"]["gbp"]["factors-enabled"]["obstacle"] = False          # nothing keeps the robots off the shapes
    return sc


def _engine(sc, environment_collisions):
    return sim.Simulation(sc, World(config.world_params(sc["config"])), environment_collisions=environment_collisions)


def _export(s):
    return json.dumps(s.export(), sort_keys=True)


def test_blinded_obstacles_inside_the_mission_chain():
    sc, ticks = _blind_obstacles(), 60
    dev, host, off = _engine(sc, True), _engine(sc, "host"), _engine(sc, False)
    assert dev.dev and host.dev and dev._dev_env_coll and not host._dev_env_coll and host._env_coll and not off._env_coll
    for t in range(ticks):
        for s in (dev, host, off):
            s.tick()
        host._flush_trackers(synchronise=True)          # tick by tick: the device's log against the host's history so far
        d, h = dev.environment_collisions, host.environment_collisions
        assert {k: v["aabbs"] for k, v in d.items()} == {k: v["aabbs"] for k, v in h.items() if v["aabbs"]}, t
    ex = dev.export()
    counts = {rid: r["collisions"]["environment"] for rid, r in ex["robots"].items()}
    print("environment collisions per robot:", counts, "pairs:", [(e["robot"], e["obstacle"], len(e["aabbs"])) for e in ex["collisions"]["environment"]])
    assert sum(counts.values()) > 0 and len(ex["collisions"]["environment"]) > 0
    assert sum(counts.values()) == sum(len(e["aabbs"]) for e in ex["collisions"]["environment"])
    assert _export(dev) == _export(host)
    chunked = _engine(sc, True).run(max_ticks=ticks, chunk=256)          # through mgx_mission_run
    assert chunked.tick_no == ticks and _export(chunked) == _export(host)
    # the option off: today's export, field for field — which is the one above with the two fields at their constants
    ex_off = off.export()
    assert all(r["collisions"]["environment"] == 0 for r in ex_off["robots"].values()) and ex_off["collisions"]["environment"] == []
    for r in ex["robots"].values():
        r["collisions"]["environment"] = 0
    ex["collisions"]["environment"] = []
    assert json.dumps(ex, sort_keys=True) == json.dumps(ex_off, sort_keys=True)
    for x, y in zip(dev.w.read_beliefs(), off.w.read_beliefs()):       # and nothing else moved
        assert np.array_equal(x, y)


# ---- 7. edge cases ------------------------------------------------------------------------------------------------------------
def test_a_full_log_drops_nothing_silently():
    passes, radii, env, chk, per_pass = _crowd_checked("cross-grid")
    assert len(chk.events) > 4
    w = _bare_world(radii)
    w.env_collisions_enable(env, event_capacity=4)
    _run_crowd(w, passes)
    ev, total, dropped, per = w.env_collisions_read()
    assert total == 4 and len(ev) == 4 and total + dropped == len(chk.events)
    filling = next(p for p in range(len(per_pass)) if sum(per_pass[:p + 1]) > 4)
    before = [e for e in chk.events if e[0] < filling]
    got = _device_events(ev)
    assert got[:len(before)] == before
    rest = got[len(before):]
    assert set(rest) <= {e for e in chk.events if e[0] == filling} and len(set(rest)) == len(rest)
    assert np.array_equal(per, chk.per_robot(len(radii)))


def test_more_contacts_than_slots_is_an_error_with_outputs_filled():
    env = _cross_grid()
    chk = Checker(env)
    radii, pos = [0.5, 12.0], _xyz([(5.0, 5.0), (3.0, 4.0)])               # a tile's centre; a ball over two dozen corner cubes
    gap = signed_gap(chk.cols, chk.verts, pos[:, [0, 2]], radii)
    n_touched = int((gap[1] <= 0).sum())
    assert n_touched > 8 and not (gap[0] <= 0).any() and (np.abs(gap) > 0.05).all()
    chk.step([0, 1], radii, pos)
    w = _bare_world(radii)
    w.env_collisions_enable(env)
    w.env_collisions_update(pos)
    with pytest.raises(hostlib.MgxError, match="more than 8 colliders"):
        w.env_collisions_read()
    ev, total, dropped, per, rc = w.env_collisions_read(strict=False)
    assert rc == -4 and total == n_touched and dropped == 0 and list(per) == [0, n_touched]
    assert _device_events(ev) == chk.events


def test_a_radius_larger_than_a_tile_finds_contacts_in_every_cell():
    rows = ["█████" for _ in range(5)]
    for r, c in ((0, 0), (0, 4), (4, 0), (4, 4), (2, 4)):
        rows[r] = rows[r][:c] + " " + rows[r][c + 1:]
    env = environment.new(rows, 0.5, 1.0, 10.0)
    chk = Checker(env)
    assert len(chk.cols) == 5
    radii = [22.0, 3.0]
    w = _bare_world(radii)
    w.env_collisions_enable(env)
    # colliders in creation order: the filled tiles (0, 0), (0, 4), (2, 4), (4, 0), (4, 4); the ball reaches over two tiles
    for centre, touched in (((0.0, 0.0), [0, 1, 2, 3, 4]), ((-8.0, 0.0), [0, 3]), ((60.0, 0.0), []), ((0.0, 0.0), [0, 1, 2, 3, 4])):
        pos = _xyz([centre, (-100.0, -100.0)])
        assert list(np.nonzero(signed_gap(chk.cols, chk.verts, pos[:, [0, 2]], radii)[0] <= -0.01)[0]) == touched
        w.env_collisions_update(pos)
        chk.step([0, 1], radii, pos)
    ev, total, dropped, per = w.env_collisions_read()
    assert len(chk.events) == 10                       # five, none new, none, five again
    assert _device_events(ev) == chk.events and (total, dropped) == (10, 0) and list(per) == [10, 0]


def test_robots_join_across_the_first_sizing_while_a_contact_is_held():
    """The first sizing (for the two robots of the first pass) leaves room for R + R/4 + 64 per-robot counts, rounded up to a
    multiple of 64, and as many sets of slots.  One robot more than that joins while robot 0 rests on a collider: counts and `touching`
    slots move to the front of longer arrays — no second event for the held contact, one for the new robot, the earlier
    count kept."""
    env = _cross_grid()
    chk = Checker(env)
    first = 2
    n = ((first + first // 4 + 64 + 63) & ~63) + 1     # observers_room: the room the first sizing leaves for the counts; one more
    radii = np.full(n, 0.5, F)
    cuboids = np.nonzero(chk.cols["kind"] == CUBOID)[0]
    held, met = int(cuboids[0]), int(cuboids[-1])
    points = [(-95.0 + 10.0 * (i % 20), -95.0 + 10.0 * (i // 20)) for i in range(n)]   # tile centres: nothing there
    points[0] = (float(chk.cols["tx"][held]), float(chk.cols["tz"][held]))
    points[n - 1] = (float(chk.cols["tx"][met]), float(chk.cols["tz"][met]))
    gap = signed_gap(chk.cols, chk.verts, points, radii)
    assert [list(np.nonzero(g <= 0)[0]) for g in gap] == [[held]] + [[]] * (n - 2) + [[met]] and (np.abs(gap) > 0.05).all()
    pos = _xyz(points)
    w = _bare_world(radii[:first])
    w.env_collisions_enable(env)

    def run(pos, fresh):
        w.env_collisions_update(pos)
        assert chk.step(list(range(len(pos))), radii, pos) == fresh
        ev, total, dropped, per = w.env_collisions_read()
        assert (total, dropped) == (len(chk.events), 0) and _device_events(ev) == chk.events
        assert np.array_equal(per, chk.per_robot(len(pos)))
        return per
    assert list(run(pos[:first], 1)) == [1, 0]
    for r in radii[first:]:
        _add(w, r)
    per = run(pos, 1)
    assert [e[:3] for e in chk.events] == [(0, 0, held), (1, n - 1, met)]
    assert list(per) == [1] + [0] * (n - 2) + [1]


def test_off_means_off():
    import torch
    L = hostlib.lib()
    n = ctypes.c_uint64()
    w = _bare_world([1.0, 1.0])
    torch.cuda.synchronize()
    # no allocation: the device's free memory stands where it stood.  Other processes share the card and may move the figure
    # between the two readings, so the sequence is given five goes and one undisturbed go is asked for — an allocation of
    # this process's own would show in every one of them.
    undisturbed = 0
    for _ in range(5):
        free_before = torch.cuda.mem_get_info()[0]
        assert L.mgx_env_collisions_update(w._w, None) == -4             # MGX_ERR_STATE
        assert L.mgx_env_collisions_read(w._w, 0, None, 0, ctypes.byref(n), ctypes.byref(n), None) == -4
        assert L.mgx_env_collisions_clear(w._w) == -4
        w.env_collisions_enable(None)                                    # off while off: nothing to do
        undisturbed += torch.cuda.mem_get_info()[0] == free_before
    assert undisturbed >= 1
    env = _cross_grid()
    w.env_collisions_enable(env)
    with pytest.raises(hostlib.MgxError):
        w.env_collisions_enable(env)                                     # one map at a time
    w.env_collisions_update(_xyz([(0.0, 0.0), (4.0, 4.0)]))
    assert w.env_collisions_read()[1] >= 1
    w.env_collisions_enable(None)
    assert L.mgx_env_collisions_update(w._w, None) == -4
    w.env_collisions_enable(env)                                         # on again: from everybody Free, an empty log
    assert w.env_collisions_read()[1] == 0
    # the robot-robot pass and the rest of a tick do not notice
    sc = _scenario("Circle Experiment")
    sc["formation"]["formations"][0]["robots"] = 8
    on, off = _engine(sc, True), _engine(sc, False)
    for t in range(15):
        on.tick()
        off.tick()
        assert on.w.last_sweep() == off.w.last_sweep(), t
    for x, y in zip(on.w.read_beliefs(), off.w.read_beliefs()):
        assert np.array_equal(x, y)
    assert np.array_equal(on.translation, off.translation)
    assert json.dumps(on.export(), sort_keys=True) == json.dumps(off.export(), sort_keys=True)   # (a map without colliders)


def test_a_world_with_ghosts_is_refused():
    w = _bare_world([1.0])
    _add(w, 1.0, ghost=True)
    with pytest.raises(hostlib.MgxError, match="unsharded"):
        w.env_collisions_enable(_cross_grid())
    w2 = _bare_world([1.0])
    w2.env_collisions_enable(_cross_grid())
    _add(w2, 1.0, ghost=True)
    assert hostlib.lib().mgx_env_collisions_update(w2._w, _xyz([(0.0, 0.0), (1.0, 1.0)]).ctypes.data) == -4
