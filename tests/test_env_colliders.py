"""mgx_env_colliders (include/mgx.h): the map's colliders as the reference's map generator creates them
(crates/magics/src/environment/map_generator.rs: build_tile_grid :537-1293 piped into build_obstacles :141-514), checked

1. against an independent f64 restatement of that file, written below with line citations, for every environment of
   tests/golden/scenarios.json;
2. against the rasteriser (oracle.env, pinned byte for byte elsewhere): the union of the tile cuboids is the black of the
   image at expansion 0 — which pins the reading of Bevy's Cuboid -> parry2d Cuboid conversion (half extents (x / 2, z / 2)
   at (translation.x, translation.z)), the conversion itself living in a parry fork that is not in the reference's tree;
3. at the ABI: capacity query, invalid environments, header / ctypes agreement, both libraries.

No device is needed by any of it."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from magics_amd import environment, hostlib
from oracle import env as oracle_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALL, CUBOID, POLYGON = hostlib.COLLIDER_BALL, hostlib.COLLIDER_CUBOID, hostlib.COLLIDER_POLYGON


def _scenarios():
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        return json.load(f)


# ---- 1. the f64 restatement ------------------------------------------------------------------------------------------------
def _hull(points):
    """ConvexPolygon::from_convex_hull as a set of vertices: monotone chain, counter-clockwise, collinear points dropped"""
    pts = sorted(set((float(x), float(y)) for x, y in points))
    if len(pts) < 3:
        return pts

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def _tile_cuboids(tile, ox, oz, ts, pw):
    """one tile's vec![(Cuboid::new(x, _, z), Transform (tx, _, tz))] as (x, z, tx, tz), in the vec's order"""
    base = ts * (1.0 - pw) / 2.0                     # :559 base_dim
    po = (pw * ts + base) / 2.0                      # :566 pos_offset
    plug_x, plug_z = (ts / 2.0, pw * ts), (pw * ts, ts / 2.0)   # :663-664 / :765-766
    wide = lambda tz: (ts, base, ox, tz)             # Cuboid::new(tile_size, _, base_dim)
    tall = lambda tx: (base, ts, tx, oz)             # Cuboid::new(base_dim, _, tile_size)
    cube = lambda tx, tz: (base, base, tx, tz)
    return {
        "─": [wide(oz - po), wide(oz + po)], "-": [wide(oz - po), wide(oz + po)],                                   # :582-614
        "│": [tall(ox - po), tall(ox + po)], "|": [tall(ox - po), tall(ox + po)],                                   # :615-648
        "╴": [wide(oz - po), wide(oz + po), plug_x + (ox + ts / 4.0, oz)],                                          # :649-699
        "╶": [wide(oz - po), wide(oz + po), plug_x + (ox - ts / 4.0, oz)],                                          # :700-750
        "╷": [tall(ox - po), tall(ox + po), plug_z + (ox, oz + ts / 4.0)],                                          # :751-801
        "╵": [tall(ox - po), tall(ox + po), plug_z + (ox, oz - ts / 4.0)],                                          # :802-852
        "┌": [cube(ox + po, oz - po), tall(ox - po), wide(oz + po)],                                                # :853-897
        "┐": [cube(ox - po, oz - po), tall(ox + po), wide(oz + po)],                                                # :898-941
        "└": [cube(ox + po, oz + po), tall(ox - po), wide(oz - po)],                                                # :942-986
        "┘": [cube(ox - po, oz + po), tall(ox + po), wide(oz - po)],                                                # :987-1031
        "┬": [cube(ox - po, oz - po), cube(ox + po, oz - po), wide(oz + po)],                                       # :1032-1072
        "┴": [cube(ox - po, oz + po), cube(ox + po, oz + po), wide(oz - po)],                                       # :1073-1113
        "├": [cube(ox + po, oz - po), cube(ox + po, oz + po), tall(ox - po)],                                       # :1114-1154
        "┤": [cube(ox - po, oz - po), cube(ox - po, oz + po), tall(ox + po)],                                       # :1155-1195
        "┼": [cube(ox - po, oz - po), cube(ox + po, oz - po), cube(ox - po, oz + po), cube(ox + po, oz + po)],      # :1196-1244
        " ": [(ts, ts, ox, oz)],                                                                                    # :1245-1255
    }.get(tile, [])                                                                                                 # :1256 _ => None


def _rot(angle, x, y):
    return x * math.cos(angle) - y * math.sin(angle), x * math.sin(angle) + y * math.cos(angle)


def restate(env):
    """[{kind, row, col, obstacle, t, radius | half | verts, mins, maxs}] in f64"""
    grid, st = env["tiles"]["grid"], env["tiles"]["settings"]
    ts, pw = float(np.float32(st["tile-size"])), float(np.float32(st["path-width"]))
    nrows, ncols = len(grid), len(grid[0])
    out = []

    def cuboid(row, col, ob, hx, hz, tx, tz):
        out.append({"kind": CUBOID, "row": row, "col": col, "obstacle": ob, "t": (tx, tz), "half": (hx, hz),
                    "mins": (tx - hx, tz - hz), "maxs": (tx + hx, tz + hz)})

    def polygon(row, col, ob, local, tx, tz, angle):
        # Isometry2::new((tx, tz), angle) applied to the hull of the local points
        world = [tuple(np.add(_rot(angle, x, y), (tx, tz))) for x, y in _hull(local)]
        w = np.array(world)
        out.append({"kind": POLYGON, "row": row, "col": col, "obstacle": ob, "t": (tx, tz), "verts": w,
                    "mins": tuple(w.min(axis=0)), "maxs": tuple(w.max(axis=0))})

    gox, goz = ncols / 2.0 - 0.5, -(nrows / 2.0 - 0.5)                   # :563-564
    for y, row in enumerate(grid):                                       # :570-571
        for x, tile in enumerate(row):
            ox, oz = (x - gox) * ts, (-y - goz) * ts                     # :574-579
            for dx, dz, tx, tz in _tile_cuboids(tile, ox, oz, ts, pw):
                cuboid(y, x, -1, dx / 2.0, dz / 2.0, tx, tz)             # :1280-1287 (Cuboid::new takes full lengths)
    gox, goz = ncols / 2.0 - 0.5, nrows / 2.0 - 0.5                      # :154-155
    for q, ob in enumerate(env.get("obstacles") or []):
        row, col = ob["tile-coordinates"]["row"], ob["tile-coordinates"]["col"]
        ox, oz, po = (col - gox) * ts, (row - goz) * ts, ts / 2.0        # :169-175
        tx, ty, rot, sh = ob["translation"]["x"], ob["translation"]["y"], ob["rotation"], ob["shape"]
        cx = tx * ts + ox - po
        cz_neg = -(ty * ts + oz - po)
        if sh["kind"] == "circle":                                       # :181-208
            cz, r = (1.0 - ty) * ts + oz - po, sh["radius"] * ts
            out.append({"kind": BALL, "row": row, "col": col, "obstacle": q, "t": (cx, cz), "radius": r,
                        "mins": (cx - r, cz - r), "maxs": (cx + r, cz + r)})
        elif sh["kind"] == "triangle":                                   # :209-276; Triangle::points, gbp_environment lib.rs:192-210
            a, b = sh["angles"]
            c = math.pi - (a + b)
            r = sh["radius"]
            pts = [(math.cos(an) * r / math.sin(g), math.sin(an) * r / math.sin(g))
                   for an, g in ((math.pi + a / 2.0, a), (-b / 2.0, b), (math.pi - b - c / 2.0, c))]
            pts = [(-px * ts, py * ts) for px, py in pts]                # :227-229 mirrored in x
            ra = math.pi / 2.0 - rot                                     # :253-255 Quat::from_rotation_y on (x, 0, y), .xz():
            pts = [(px * math.cos(ra) + py * math.sin(ra), -px * math.sin(ra) + py * math.cos(ra)) for px, py in pts]  # :264-272
            polygon(row, col, q, pts, cx, cz_neg, ra - math.pi / 2.0)    # :257-260
        elif sh["kind"] == "regular-polygon":                            # :277-379; point_at, lib.rs:271-287
            n, r = sh["sides"], sh["radius"]
            off = math.pi + (0.0 if n == 4 else (math.pi / 2.0 if n % 2 else -math.pi / 2.0))   # :323-328
            ang = rot + off                                              # :342-344
            pts = []
            for i in range(n):
                th = 2.0 * math.pi / n * i + math.pi / 4.0
                px, py = _rot(ang, math.cos(th) * r, math.sin(th) * r)   # :356
                pts.append((px * ts / 2.0, py * ts / 2.0))               # :348, :360-362
            polygon(row, col, q, pts, cx, cz_neg, ang)                   # :373-376
        elif sh["kind"] == "polygon":                                    # :380-429
            polygon(row, col, q, [(px * ts, py * ts) for px, py in sh["points"]], cx, ty * ts + oz - po, 0.0)
        elif sh["kind"] == "rectangle":                                  # :430-477
            cuboid(row, col, q, sh["width"] * ts / 4.0, sh["height"] * ts / 4.0, cx, cz_neg)
    return out


def _cyclic_distance(a, b):
    """smallest over the rotations of the cycle of the largest coordinate difference (a hull has no first vertex)"""
    return min(np.abs(np.roll(a, k, axis=0) - b).max() for k in range(len(a)))


@pytest.mark.parametrize("name", sorted(_scenarios()))
def test_colliders_equal_the_f64_restatement(name):
    env = _scenarios()[name]["environment"]
    cols, verts = hostlib.env_colliders(env)
    want = restate(env)
    tol = 1e-4 * env["tiles"]["settings"]["tile-size"]   # f32 construction against f64 plus sinf / cosf; not a measurement
    assert len(cols) == len(want)
    assert [int(k) for k in cols["kind"]] == [w["kind"] for w in want]
    assert [(int(c["tile_row"]), int(c["tile_col"]), int(c["obstacle"])) for c in cols] == [(w["row"], w["col"], w["obstacle"]) for w in want]
    used = 0
    for c, w in zip(cols, want):
        assert abs(c["tx"] - w["t"][0]) <= tol and abs(c["tz"] - w["t"][1]) <= tol
        assert np.abs(np.array(c["mins"], dtype=np.float64) - w["mins"]).max() <= tol
        assert np.abs(np.array(c["maxs"], dtype=np.float64) - w["maxs"]).max() <= tol
        if w["kind"] == BALL:
            assert abs(c["radius"] - w["radius"]) <= tol
        elif w["kind"] == CUBOID:
            assert np.abs(np.array(c["half_extents"], dtype=np.float64) - w["half"]).max() <= tol and c["angle"] == 0.0
        else:
            assert int(c["first_vertex"]) == used and int(c["n_vertices"]) == len(w["verts"])
            v = verts[used:used + len(w["verts"])].astype(np.float64)
            used += len(v)
            assert _cyclic_distance(v, w["verts"]) <= tol
            e = np.roll(v, -1, axis=0) - v                                # counter-clockwise and strictly convex
            assert len(v) < 3 or (e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0] > 0).all()
    assert used == len(verts)


def test_the_fixtures_cover_every_kind_and_the_quirks():
    sc = _scenarios()
    kinds = {sh["shape"]["kind"] for s in sc.values() for sh in s["environment"]["obstacles"]}
    assert kinds == {"circle", "regular-polygon", "rectangle", "triangle", "polygon"}
    env = sc["Obstacle Shapes Showcase"]["environment"]
    cols, _ = hostlib.env_colliders(env)
    ts = env["tiles"]["settings"]["tile-size"]
    ob = env["obstacles"]
    k = next(i for i, o in enumerate(ob) if o["shape"]["kind"] == "circle")
    c = cols[cols["obstacle"] == k][0]
    # the circle's z is (1 - y) * tile_size - tile_size / 2 on a one-tile map, NOT negated; its radius is radius * tile_size
    assert abs(c["tz"] - ((1.0 - ob[k]["translation"]["y"]) * ts - ts / 2.0)) < 1e-3 and abs(c["radius"] - ob[k]["shape"]["radius"] * ts) < 1e-4
    k = next(i for i, o in enumerate(ob) if o["shape"]["kind"] == "rectangle")
    c = cols[cols["obstacle"] == k][0]
    assert abs(c["half_extents"][0] - ob[k]["shape"]["width"] * ts / 4.0) < 1e-4 and abs(c["tz"] + (ob[k]["translation"]["y"] * ts - ts / 2.0)) < 1e-3


# ---- 2. tile cuboids against the rasteriser ----------------------------------------------------------------------------------
# every character build_tile_grid handles, except '-' and '|': map_generator.rs:582,615 treats them as '─' and '│', while
# env_to_png's is_tile_obstacle (crates/env_to_png/src/lib.rs:338-479) does not know them and paints the tile free — the
# reference's map and image truly differ there, and the colliders follow map_generator.rs.  '█' is handled by neither.
_GRIDS = {
    "square": (["┌┬┐├", "└┴┘┤", "│─ ┼", "╴╵╶╷"], 0.1325, 50.0),
    "wide": (["╴┌─┬╶█", "╷├┼┤╵ ", "│└┴┘┐┌"], 0.3, 20.0),
}


@pytest.mark.parametrize("which", sorted(_GRIDS))
def test_tile_cuboids_are_the_black_of_the_image(which):
    grid, pw, ts = _GRIDS[which]
    assert {ch for row in _GRIDS["square"][0] + _GRIDS["wide"][0] for ch in row} >= set("─│╴╶╷╵┌┐└┘┬┴├┤┼ ")
    env = environment.new(grid, pw, 1.0, ts)
    res = 40
    img = oracle_env.env_to_image(env, res, 0.0)
    cols, _ = hostlib.env_colliders(env)
    assert len(cols) and (cols["kind"] == CUBOID).all() and (cols["obstacle"] == -1).all()
    nrows, ncols = len(grid), len(grid[0])
    pix = ts / res
    # pixel (i, j)'s centre in the map generator's frame: x grows with the column, z DEcreases with the row (:564, :575)
    x = ((np.arange(ncols * res) + 0.5) * pix - ncols * ts / 2.0)[None, :]
    z = (nrows * ts / 2.0 - (np.arange(nrows * res) + 0.5) * pix)[:, None]
    inside = np.zeros(img.shape, bool)
    edge = np.full(img.shape, np.inf)
    for c in cols:
        dx, dz = np.abs(x - c["tx"]) - c["half_extents"][0], np.abs(z - c["tz"]) - c["half_extents"][1]   # signed, per axis
        within = (dx <= 0) & (dz <= 0)
        inside |= within
        outside = np.hypot(np.maximum(dx, 0), np.maximum(dz, 0))
        edge = np.minimum(edge, np.where(within, np.minimum(-dx, -dz), outside))
    judged = edge > pix
    assert judged.mean() > 0.7
    black = img == 0
    assert black[judged].any() and (~black[judged]).any()
    wrong = judged & (black != inside)
    by_tile = sorted({grid[j // res][i // res] for j, i in zip(*np.nonzero(wrong))})
    assert not wrong.any(), f"tiles whose cuboids are not the image's black: {by_tile}"


# ---- 3. the ABI ----------------------------------------------------------------------------------------------------------------
NAMES = ("mgx_env_colliders", "mgx_env_collisions_enable", "mgx_env_collisions_update", "mgx_env_collisions_read", "mgx_env_collisions_clear")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgx.h")).read(), flags=re.S)


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    return [" ".join(d.split()) for d in body.split(";") if d.strip()]


def test_the_calls_are_declared_bound_and_exported_by_both_libraries():
    declared = set(re.findall(r"\b(mgx_[a-z0-9_]+)\s*\(", _header()))
    for name in NAMES:
        assert name in declared and name in hostlib.SYMBOLS, name
    for path in (hostlib.LIB_PATH, hostlib.FMA_LIB_PATH):
        L = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(L, name), (path, name)


def test_the_records_agree_in_header_ctypes_and_numpy():
    assert _struct_fields("mgx_env_collider") == ["int32_t kind", "int32_t tile_row, tile_col", "int32_t obstacle", "float tx, tz, angle",
                                                  "float radius", "float half_extents[2]", "uint32_t first_vertex, n_vertices",
                                                  "float mins[2], maxs[2]"]
    names = ("kind", "tile_row", "tile_col", "obstacle", "tx", "tz", "angle", "radius", "half_extents", "first_vertex", "n_vertices", "mins", "maxs")
    offsets = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 44, 48, 56]
    dt = hostlib.env_collider_dtype()
    assert ctypes.sizeof(hostlib.EnvCollider) == dt.itemsize == 64
    assert [dt.fields[n][1] for n in names] == offsets and [getattr(hostlib.EnvCollider, n).offset for n in names] == offsets
    assert _struct_fields("mgx_env_collision_event") == ["uint64_t pass", "int32_t robot, collider", "float mins[2], maxs[2]"]
    dt = hostlib.env_collision_event_dtype()
    assert ctypes.sizeof(hostlib.EnvCollisionEvent) == dt.itemsize == 32
    assert [dt.fields[n][1] for n in ("pass", "robot", "collider", "mins", "maxs")] == [0, 8, 12, 16, 24]
    assert [getattr(hostlib.EnvCollisionEvent, n).offset for n in ("pass_", "robot", "collider", "mins", "maxs")] == [0, 8, 12, 16, 24]
    hdr = _header()
    assert [int(re.search(r"#define MGX_COLLIDER_%s (\d+)" % k, hdr).group(1)) for k in ("BALL", "CUBOID", "POLYGON")] == [BALL, CUBOID, POLYGON]


@pytest.mark.parametrize("fma", [False, True], ids=["libmgx", "libmgx_fma"])
def test_capacity_query_and_too_little_room(fma):
    L = hostlib.lib(fma)
    env = _scenarios()["Obstacle Shapes Showcase"]["environment"]
    d = environment._Desc(env)
    n, nv = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.mgx_env_colliders(ctypes.byref(d.desc), None, 0, ctypes.byref(n), None, 0, ctypes.byref(nv)) == 0
    assert n.value == len(env["obstacles"]) and nv.value > 3 * 12
    cols = np.zeros(n.value, hostlib.env_collider_dtype())
    verts = np.full((nv.value + 1, 2), 7.0, np.float32)
    assert L.mgx_env_colliders(ctypes.byref(d.desc), cols.ctypes.data, n.value, None, verts.ctypes.data, nv.value, None) == 0
    assert (verts[-1] == 7.0).all() and not (verts[:-1] == 7.0).all(axis=1).any()
    again, v2 = hostlib.env_colliders(env, fma=fma)
    assert again.tobytes() == cols.tobytes() and v2.tobytes() == verts[:-1].tobytes()
    assert L.mgx_env_colliders(ctypes.byref(d.desc), cols.ctypes.data, n.value - 1, None, verts.ctypes.data, nv.value, None) == -1
    assert L.mgx_env_colliders(ctypes.byref(d.desc), cols.ctypes.data, n.value, None, verts.ctypes.data, nv.value - 1, None) == -1
    assert L.mgx_env_colliders(ctypes.byref(d.desc), None, n.value, None, None, 0, None) == -1


def test_both_libraries_build_the_same_table():
    for name, sc in _scenarios().items():
        a, b = hostlib.env_colliders(sc["environment"], fma=False), hostlib.env_colliders(sc["environment"], fma=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name


def test_invalid_environments_are_refused():
    L = hostlib.lib()
    n = ctypes.c_uint32()

    def rc(env_desc):
        return L.mgx_env_colliders(ctypes.byref(env_desc), None, 0, ctypes.byref(n), None, 0, ctypes.byref(n))
    assert L.mgx_env_colliders(None, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == -1
    good = environment._Desc(environment.circle())
    assert rc(good.desc) == 0
    for field, value in (("n_rows", 0), ("n_cols", 0), ("tiles", None), ("path_width", 1.5), ("path_width", -0.1), ("obstacles", None)):
        d = environment._Desc(environment.circle())
        setattr(d.desc, field, value)
        assert rc(d.desc) == -1, field
        assert L.mgx_last_error()
    for field, value in (("translation_x", 1.5), ("rotation", 7.0), ("rotation", -0.1), ("shape", 9), ("radius", 0.0), ("radius", float("inf")), ("sides", 0)):
        d = environment._Desc(environment.circle())
        setattr(d.obstacles[0], field, value)
        assert rc(d.desc) == -1, field
    d = environment._Desc(environment.circle())
    d.obstacles[3].width = -1.0                                            # the rectangle
    assert rc(d.desc) == -1
    d = environment._Desc(_scenarios()["Merge"]["environment"])
    d.obstacles[0].n_points = 0
    assert rc(d.desc) == -1


def test_a_null_world_is_an_invalid_argument_without_a_device():
    L = hostlib.lib()
    n = ctypes.c_uint64()
    assert L.mgx_env_collisions_enable(None, None, 0) == -1
    assert L.mgx_env_collisions_update(None, None) == -1
    assert L.mgx_env_collisions_read(None, 0, None, 0, ctypes.byref(n), ctypes.byref(n), None) == -1
    assert L.mgx_env_collisions_clear(None) == -1
    assert b"null" in L.mgx_last_error()
