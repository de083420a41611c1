"""Runs the reference's OWN metric functions on seeded series and records inputs and results in tests/golden/track_metrics.json
(data only).  tests/test_track_metrics.py holds magics_amd/track_metrics.py against it.

Run in the build container (needs /root/reference, numpy and scipy):  python tests/golden/make_track_metrics.py

Sources, read at generation time and never copied: `ldj` of scripts/ldj.py:17-55; `Line`, `line_from_line_segment`,
`projection_onto_line` and `closest_projection_onto_line_segments` of scripts/perpendicular-path-deviation.py:35-60, and the sum
and "RMSE" of its lines 114-115.  Only the definitions are taken (by `ast`): the modules import plotting and table packages at
the top that need not be installed.

Series: velocities are random walks with noise, rounded to f32 (what the trackers make), n = 3 .. 301 in both parities, at time
stamps t0 + i * dt; routes of 2 .. 8 points whose x grows strictly (no vertical segment, none of zero length: the reference's
slope-intercept form yields inf / NaN there) and f32 positions near them.  f32 values are written in their shortest form: read
them back through numpy.float32.  Every recorded LDJ must be finite and inside the range the reference plots, (-25, 0)."""
import ast
import dataclasses
import json
import os

import numpy as np
import scipy
from scipy.integrate import simpson

REF = "/root/reference/scripts"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "track_metrics.json")
LENGTHS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 17, 18, 25, 26, 33, 40, 51, 64, 65, 80, 99, 100, 101, 128, 150, 201, 250, 301]
MAX_POSITIONS = 24


def definitions(path, names):
    """the named top-level function / class definitions of a file, executed on their own"""
    tree = ast.parse(open(path, encoding="utf-8").read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    ns = {"np": np, "simpson": simpson, "dataclass": dataclasses.dataclass}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def short(a):
    """f32 values as the shortest decimal that reads back to them"""
    return [float(str(x)) for x in np.asarray(a, dtype=np.float32).reshape(-1)]


def main():
    (ldj,) = definitions(os.path.join(REF, "ldj.py"), ["ldj"])
    _, line_from_line_segment, _, closest = definitions(os.path.join(REF, "perpendicular-path-deviation.py"),
                                                        ["Line", "line_from_line_segment", "projection_onto_line", "closest_projection_onto_line_segments"])
    cases = []
    for ci, n in enumerate(LENGTHS):
        seed = 1000 * ci
        while True:  # (the first seed whose LDJ is inside the plotted range: short series need a rough one)
            rng = np.random.default_rng(seed)
            start = rng.uniform(-3.0, 3.0, 2)
            v = f32(start + np.cumsum(rng.normal(0.0, 0.3, (n, 2)), axis=0) + rng.normal(0.0, 0.6, (n, 2)))
            t0, dt = float(np.round(rng.uniform(0.0, 50.0), 3)), float(rng.choice([0.1, 0.1, 0.2, 1.0 / 3.0]))
            value = float(ldj(v.astype(np.float64), t0 + dt * np.arange(n)))
            if np.isfinite(value) and -25.0 < value < 0.0:
                break
            seed += 1
        n_route = 2 + ci % 7
        route = np.round(np.stack([np.cumsum(rng.uniform(2.0, 10.0, n_route)) - 20.0, rng.uniform(-15.0, 15.0, n_route)], axis=1), 3)
        n_pos = min(n, MAX_POSITIONS)
        seg = rng.integers(0, n_route - 1, n_pos)
        along = rng.uniform(-0.2, 1.2, n_pos)[:, None]
        d = route[seg + 1] - route[seg]
        normal = np.stack([-d[:, 1], d[:, 0]], axis=1) / np.linalg.norm(d, axis=1)[:, None]
        pos = f32(route[seg] + along * d + rng.normal(0.0, 0.8, n_pos)[:, None] * normal).astype(np.float64)
        lines = [line_from_line_segment(*a, *b) for a, b in zip(route[:-1], route[1:])]
        proj = np.array([closest(p, lines) for p in pos])
        error = float(np.sum(np.linalg.norm(pos - proj, axis=1)))     # (perpendicular-path-deviation.py:114)
        rmse = float(np.sqrt(error / len(pos)))                      # (:115)
        assert np.isfinite(rmse)
        cases.append({"seed": seed, "n": n, "t0": t0, "dt": dt, "velocities_f32": short(v), "ldj": value,
                      "route": route.reshape(-1).tolist(), "positions_f32": short(pos), "deviation_sum": error, "rmse": rmse})
    doc = {"about": "reference ldj() and closest-projection deviation on seeded series; made by tests/golden/make_track_metrics.py",
           "numpy": np.__version__, "scipy": scipy.__version__, "cases": cases}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(OUT)} bytes, LDJ in [{min(c['ldj'] for c in cases):.3f}, {max(c['ldj'] for c in cases):.3f}]")


if __name__ == "__main__":
    main()
