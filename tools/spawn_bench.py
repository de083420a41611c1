"""What a robot that joins a running world costs (profiles/spawn_in_place.md): wall time from mgx_robot_add to the end of the
next synchronised tick, on a world that asked for head-room (mgx_world_reserve: the robot is appended on the device) and on one
that did not (the device state is pulled and laid out again).

    python tools/spawn_bench.py [--spawns 32] [--shapes 60x12,1000x16]

Two grid worlds with inter-robot factors: 60 robots at Junction Twoway's horizon (K = 12) and 1000 x 16.  Per shape one world
per form, both alive; the forms alternate spawn by spawn, each spawn followed by plain ticks (timed: the baseline a spawn is
compared with).  The new robots stand apart from the grid (no connections), as a formation's do when they appear.  On an engine
without mgx_world_reserve only the unreserved form runs.  One JSON line, and the table of the profile."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from magics_amd import World  # noqa: E402
from magics_amd import scenarios as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spawns", type=int, default=32)
ap.add_argument("--shapes", default="60x12,1000x16")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--between", type=int, default=3, help="plain ticks after every spawn")
a = ap.parse_args()


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return [round(q[0] * 1e6, 1), round(q[2] * 1e6, 1)]


out = {"spawns": a.spawns, "shapes": {}}
for shape in a.shapes.split(","):
    n, K = (int(x) for x in shape.split("x"))
    sc = S.grid_scenario(n, K, interrobot=True, tracking=True, comm_radius=8.0)
    tick = S.tick_inputs(sc)
    forms = ["unreserved"] + (["reserved"] if hasattr(World, "reserve") else [])
    worlds = {}
    for form in forms:
        w = worlds[form] = World(sc["params"])
        if form == "reserved":
            w.reserve(n + a.spawns + 2)
        S.populate(w, sc)
        for _ in range(a.warmup):
            w.tick(steps=sc["steps"], **tick)
        w.synchronize()
    spawn_t, plain_t = {f: [] for f in forms}, {f: [] for f in forms}
    for i in range(a.spawns + 2):  # (the first two: buffers that grow, first use of the kernels)
        rb = sc["robots"][i % n]
        mean0 = rb["mean0"].copy()
        mean0[:, 0] += 500.0 + 20.0 * i
        path = None if rb["path"] is None else rb["path"] + np.float32(500.0 + 20.0 * i) * np.array([1, 0], dtype=np.float32)
        for form in forms:
            w = worlds[form]
            t0 = time.perf_counter()
            w.add_robot(mean0, rb["prior_diag"], rb["dt"], rb["radius"], path=path, order_key=n + i)
            w.tick(steps=sc["steps"], **tick)
            w.synchronize()
            t1 = time.perf_counter()
            for _ in range(a.between):
                w.tick(steps=sc["steps"], **tick)
                w.synchronize()
            t2 = time.perf_counter()
            if i >= 2:
                spawn_t[form].append(t1 - t0)
                plain_t[form].append((t2 - t1) / a.between)
    row = out["shapes"][shape] = {}
    for form in forms:
        row[form] = {"spawn_tick_us": round(statistics.median(spawn_t[form]) * 1e6, 1), "spawn_tick_quartiles_us": quartiles(spawn_t[form]),
                     "plain_tick_us": round(statistics.median(plain_t[form]) * 1e6, 1), "plain_tick_quartiles_us": quartiles(plain_t[form]),
                     "layout_stats": worlds[form].layout_stats()}
        if hasattr(worlds[form], "append_stats"):
            row[form]["append_stats"] = worlds[form].append_stats()
    if "reserved" in row:
        row["reserved_over_unreserved"] = round(row["reserved"]["spawn_tick_us"] / row["unreserved"]["spawn_tick_us"], 3)
print(json.dumps(out))
print("| world | form | add_robot + tick (µs, median, quartiles) | plain tick (µs) |\n|---|---|---|---|")
for shape, row in out["shapes"].items():
    for form in ("unreserved", "reserved"):
        if form in row:
            r = row[form]
            print(f"| {shape} | {form} | {r['spawn_tick_us']} ({r['spawn_tick_quartiles_us'][0]} .. {r['spawn_tick_quartiles_us'][1]}) | {r['plain_tick_us']} |")
