"""The global planner's specification (include/mgx.h, "global planner") restated on the host in numpy / plain Python: the checker
of the device planner (mgx_planner.hip, World.plan_paths), as sim.py:_collide_environment is the checker of the collision pass.

Batched RRT* over the map's colliders: what crates/gbp_global_planner does per robot (rrtstar.rs:15-83, started from
progress_missions, robot.rs:578-633).  The `rrt` crate it calls is a git fork that is absent from the reference's tree, and so is
`rand`: there is nothing to be bit-identical to, so the specification in the header is the specification.  All arithmetic is f64,
every operation rounded on its own (Python floats and numpy ufuncs never fuse a multiply with an add); a point is tested against
the colliders as f32, through sim.environment_contacts.
"""
import math
import struct

import numpy as np

from . import hostlib
from .prng import WyRand

PLAN_OK, PLAN_MAX_ITERATIONS, PLAN_TREE_FULL = 0, 1, 2
STATUS_NAMES = {PLAN_OK: "ok", PLAN_MAX_ITERATIONS: "reached-max-iterations", PLAN_TREE_FULL: "tree-full"}
DEFAULT_HALF_EXTENT, DEFAULT_MAX_NODES, DEFAULT_ITERATIONS_PER_LAUNCH = 2000.0, 8192, 1024
F = np.float32


def params(step_size, neighbourhood_radius, collision_radius, max_iterations, smoothing_enabled=False, smoothing_max_iterations=0,
           smoothing_step=0.0, sample_half_extent=0.0, max_nodes=0, iterations_per_launch=0):
    """mgx_plan_params as a dict (the f32 fields rounded to f32, as RRTSection holds them)"""
    return {"step_size": float(F(step_size)), "neighbourhood_radius": float(F(neighbourhood_radius)), "collision_radius": float(F(collision_radius)),
            "max_iterations": int(max_iterations), "smoothing_enabled": bool(smoothing_enabled),
            "smoothing_max_iterations": int(smoothing_max_iterations), "smoothing_step": float(F(smoothing_step)),
            "sample_half_extent": float(F(sample_half_extent)), "max_nodes": int(max_nodes), "iterations_per_launch": int(iterations_per_launch)}


def params_from_config(cfg, **overrides):
    """config.rrt (RRTSection) -> params; smoothing_step is rrt.step-size, as rrtstar.rs:60 passes it"""
    rrt = cfg["rrt"]
    sm = rrt.get("smoothing", {})
    p = params(rrt["step-size"], rrt["neighbourhood-radius"], rrt["collision-radius"], rrt["max-iterations"],
               smoothing_enabled=sm.get("enabled", False), smoothing_max_iterations=sm.get("max-iterations", 0), smoothing_step=rrt["step-size"])
    p.update(overrides)
    return p


def check_params(p):
    """what mgx_planner_enable refuses"""
    pos = [p["step_size"], p["neighbourhood_radius"]] + ([p["smoothing_step"]] if p["smoothing_enabled"] else [])
    if not all(math.isfinite(v) and v > 0 for v in pos):
        raise ValueError("step_size, neighbourhood_radius (and smoothing_step) must be positive and finite")
    if not (math.isfinite(p["collision_radius"]) and p["collision_radius"] >= 0):
        raise ValueError("collision_radius must be finite and not negative")
    if not (math.isfinite(p["sample_half_extent"]) and p["sample_half_extent"] >= 0):
        raise ValueError("sample_half_extent must be finite and not negative")
    if p["max_iterations"] < 0 or p["max_nodes"] < 0 or p["smoothing_max_iterations"] < 0 or p["max_nodes"] > (1 << 16):
        raise ValueError("counts out of range")


class _Stream(WyRand):
    """a WyRand that counts its draws"""

    def __init__(self, state):
        super().__init__(state)
        self.draws = 0

    def next_u64(self):
        self.draws += 1
        return super().next_u64()


def uniform_from_u64(u, h):
    """v = f64_from_bits((u >> 12) | 0x3FF0000000000000) - 1.0 in [0, 1); v * (2h) + (-h)"""
    v = struct.unpack("<d", struct.pack("<Q", ((int(u) >> 12) | 0x3FF0000000000000) & 0xFFFFFFFFFFFFFFFF))[0] - 1.0
    return v * (2.0 * h) + (-h)


def uniform(rng, h):
    return uniform_from_u64(rng.next_u64(), h)


class Planner:
    """plan(start, end, wyrand_state) over one map.  env: an environment dict, or None for a map without colliders."""

    def __init__(self, env, p, fma=None):
        check_params(p)
        self.p = dict(p)
        if env is None:
            self.colliders, self.vertices = np.zeros(0, hostlib.env_collider_dtype()), np.zeros((0, 2), F)
        else:
            self.colliders, self.vertices = hostlib.env_colliders(env, fma)

    def feasible(self, pts):
        """[n] bool: no collider touches a ball of collision_radius at ((float)x, (float)y)"""
        from .sim import environment_contacts
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
        if not len(self.colliders) or not len(pts):
            return np.ones(len(pts), dtype=bool)
        rad = np.full(len(pts), self.p["collision_radius"], dtype=F)
        return ~environment_contacts(self.colliders, self.vertices, pts.astype(F), rad).any(axis=1)

    def plan(self, start, end, wyrand_state):
        p = self.p
        step, radius = p["step_size"], p["neighbourhood_radius"]
        h = p["sample_half_extent"] or DEFAULT_HALF_EXTENT
        cap = p["max_nodes"] or DEFAULT_MAX_NODES
        r2 = radius * radius
        rng = _Stream(wyrand_state)
        sx, sy, ex, ey = (float(F(v)) for v in (start[0], start[1], end[0], end[1]))
        X, Y, C = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        P = np.full(cap, -1, dtype=np.int32)
        X[0], Y[0] = sx, sy
        n, goal, status, it, rewires = 1, -1, PLAN_MAX_ITERATIONS, 0, 0
        for it in range(1, p["max_iterations"] + 1):
            qx = uniform(rng, h)
            qy = uniform(rng, h)
            dx, dy = X[:n] - qx, Y[:n] - qy
            d2 = dx * dx + dy * dy
            ns = int(np.argmin(d2))                                    # ties: the lowest index
            d = math.sqrt(float(d2[ns]))
            if d == 0.0:
                continue
            if d <= step:
                px, py = qx, qy
            else:
                t = step / d
                px, py = float(X[ns]) + t * (qx - float(X[ns])), float(Y[ns]) + t * (qy - float(Y[ns]))
            if not self.feasible([[px, py]])[0]:
                continue
            dx, dy = X[:n] - px, Y[:n] - py
            d2 = dx * dx + dy * dy
            near = d2 <= r2
            dist = np.sqrt(d2)
            member = near.copy()
            member[ns] = True
            cand = np.where(member, C[:n] + dist, np.inf)
            parent = int(np.argmin(cand))
            cost_new = float(cand[parent])
            if n >= cap:
                status = PLAN_TREE_FULL
                break
            m = n
            X[m], Y[m], P[m], C[m] = px, py, parent, cost_new
            n += 1
            c = cost_new + dist
            better = near & (c < C[:m])
            better[parent] = False
            rewires += int(better.sum())
            P[:m][better] = m
            C[:m][better] = c[better]
            gx, gy = px - ex, py - ey
            if math.sqrt(gx * gx + gy * gy) <= step:
                goal, status = m, PLAN_OK
                break
        out = {"status": status, "n_nodes": n, "smoothing_iterations": 0, "iterations": it if status != PLAN_MAX_ITERATIONS else p["max_iterations"], "cost": 0.0,
               "path": np.zeros((0, 2), F), "rewires": rewires, "tree": (np.stack([X[:n], Y[:n]], axis=1), P[:n].copy(), C[:n].copy())}
        if status == PLAN_OK:
            gx, gy = float(X[goal]) - ex, float(Y[goal]) - ey
            out["cost"] = float(C[goal]) + math.sqrt(gx * gx + gy * gy)
            chain, k = [], goal
            while k >= 0 and len(chain) <= n:
                chain.append(k)
                k = int(P[k])
            if k >= 0:
                raise RuntimeError("the parent chain does not end")
            pts = [(float(X[k]), float(Y[k])) for k in reversed(chain)] + [(ex, ey)]
            out["unsmoothed"] = np.array(pts, dtype=np.float64)
            if p["smoothing_enabled"]:
                pts, out["smoothing_iterations"] = self._smooth(pts, rng)
            out["path64"] = np.array(pts, dtype=np.float64)
            out["path"] = out["path64"].astype(F)
        out["wyrand_state"], out["draws"] = rng.state, rng.draws
        return out

    def chord_points(self, a, b):
        """the points of the chord a -> b the smoothing pass tests: a + (b - a) * ((j * h) / L), j = 1 .. floor(L / h)"""
        hs = self.p["smoothing_step"]
        dx, dy = b[0] - a[0], b[1] - a[1]
        L = math.sqrt(dx * dx + dy * dy)
        cnt = int(math.floor(L / hs))
        return [(a[0] + dx * ((j * hs) / L), a[1] + dy * ((j * hs) / L)) for j in range(1, cnt + 1)]

    def _smooth(self, pts, rng):
        pts, s = list(pts), 0
        while len(pts) >= 3 and s < self.p["smoothing_max_iterations"]:
            a = rng.gen_index(len(pts) - 2)
            b = a + 2 + rng.gen_index(len(pts) - 2 - a)
            if self.feasible(self.chord_points(pts[a], pts[b])).all():
                del pts[a + 1:b]
            s += 1
        return pts, s


def plan_paths(env, requests, p, fma=None):
    """requests: [(start (x, y), end (x, y), wyrand_state)] -> one result dict per request (status, n_nodes, iterations, cost,
    wyrand_state, path [n, 2] f32 — empty unless status is PLAN_OK —, tree, rewires, draws)"""
    pl = Planner(env, p, fma)
    return [pl.plan(s, e, st) for s, e, st in requests]


def slices_needed(result, p, budget):
    """The slice number a request ends in when every advance gives it `budget` iterations (include/mgx.h, mgx_plan_advance):
    PLAN_OK and PLAN_TREE_FULL: ceil((iterations + smoothing_iterations) / budget), never less than 1 — the finish takes no budget;
    PLAN_MAX_ITERATIONS: max_iterations // budget + 1 — the limit is seen at the top of an iteration that still has budget."""
    budget = int(budget)
    if budget <= 0:
        raise ValueError("the budget of a slice is positive")
    if result["status"] == PLAN_MAX_ITERATIONS:
        return int(p["max_iterations"]) // budget + 1
    if result["status"] not in (PLAN_OK, PLAN_TREE_FULL):
        raise ValueError("unknown status %r" % (result["status"],))
    done = int(result["iterations"]) + int(result["smoothing_iterations"])
    return max(1, -(-done // budget))
