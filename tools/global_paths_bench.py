"""What a burst of global paths costs (profiles/global_paths.md): mgx_apply_global_paths — one call, applied in place on the
device — against the per-robot sequence it replaces (mgx_set_tracking_path, mgx_reset_variables, mgx_reset_tracking_factors for
every robot), each followed by the one tick that pays the re-layout where there is one.

    python tools/global_paths_bench.py [--robots 1000] [--K 16] [--reps 7] [--block 5]

A grid world with inter-robot and tracking factors.  Per burst size (1, 32 and every robot) and per form, `--reps` blocks of
`--block` repetitions of [burst, one tick, synchronise]; a block's figure is its mean repetition minus the mean of a block of
plain ticks measured right before it, the form's figure the median over the blocks; the two forms alternate.  One JSON line, and the table of the profile."""
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
ap.add_argument("--robots", type=int, default=1000)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--block", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()

sc = S.grid_scenario(a.robots, a.K, interrobot=True, tracking=True, comm_radius=8.0)
n, K = len(sc["robots"]), a.K
tick = S.tick_inputs(sc)
rng = np.random.default_rng(5)
means = np.array([rb["mean0"] + rng.normal(0, 0.05, size=(K, 4)) for rb in sc["robots"]])
paths = [np.ascontiguousarray(m[[0, K // 2, K - 1], :2], dtype=np.float32) for m in means]


def one_call(w, robots):
    w.apply_global_paths(robots, [paths[r] for r in robots], means[robots])


def three_calls(w, robots):
    for r in robots:
        w.set_tracking_path(r, paths[r])
        w.reset_variables(r, means[r])
        w.reset_tracking_factors(r)


def block(w, burst, robots):
    t0 = time.perf_counter()
    for _ in range(a.block):
        if burst is not None:
            burst(w, robots)
        w.tick(steps=sc["steps"], **tick)
        w.synchronize()
    return (time.perf_counter() - t0) / a.block


out = {"robots": n, "K": K, "reps": a.reps, "block": a.block, "bursts": {}}
forms = (("one_call", one_call), ("three_calls", three_calls))
worlds = {}
for form, _ in forms:  # one world per form, both alive: the forms alternate block by block, under the same neighbours on the machine
    w = worlds[form] = World(sc["params"])
    S.populate(w, sc)
    for _ in range(a.warmup):
        w.tick(steps=sc["steps"], **tick)
    w.synchronize()
for size in (1, 32, n):
    robots = list(range(0, n, max(n // size, 1)))[:size]
    extra = {form: [] for form, _ in forms}
    for form, burst in forms:
        block(worlds[form], burst, robots)  # (buffers that grow, first use of the kernels)
    for _ in range(a.reps):
        for form, burst in forms:
            plain = block(worlds[form], None, robots)
            extra[form].append(block(worlds[form], burst, robots) - plain)
    row = out["bursts"][str(size)] = {}
    for form, _ in forms:
        row[form + "_us"] = round(statistics.median(extra[form]) * 1e6, 1)
        row[form + "_spread_us"] = [round(min(extra[form]) * 1e6, 1), round(max(extra[form]) * 1e6, 1)]
for form, _ in forms:
    out[form + "_layout_stats"] = worlds[form].layout_stats()
for size, row in out["bursts"].items():
    row["ratio"] = round(row["three_calls_us"] / max(row["one_call_us"], 1e-3), 1)
print(json.dumps(out))
print("| robots in the burst | one call (µs) | per-robot calls + re-layout (µs) | ratio |\n|---|---|---|---|")
for size, row in out["bursts"].items():
    print(f"| {size} | {row['one_call_us']} ({row['one_call_spread_us'][0]} .. {row['one_call_spread_us'][1]}) | "
          f"{row['three_calls_us']} ({row['three_calls_spread_us'][0]} .. {row['three_calls_spread_us'][1]}) | {row['ratio']} |")
