"""What a burst of global plans costs (profiles/global_planner.md): requests x tree size -> milliseconds, the engine's planner
(mgx_plan_paths: one workgroup per request, bounded launches) against the host restatement of the same specification
(magics_amd/global_planner.py), on the Solo GP map.

    python tools/planner_bench.py [--requests 1,8,64] [--iterations 500,2000,8000] [--half-extent 125] [--reps 5] [--host-requests 2]

Every request plans from the scenario's start to a goal no tree reaches (far outside the map), so each one runs exactly
`--iterations` iterations and the tree size is what the sampler grows in them; seeds differ per request.  The device figure is the
median wall time of `--reps` calls after one warm-up call; the restatement is timed on `--host-requests` of the requests and
scaled to the burst (it plans one request after the other).  One JSON line per cell, then the table of the profile."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from magics_amd import World, config, scenarios  # noqa: E402
from magics_amd import global_planner as gp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--requests", default="1,8,64")
ap.add_argument("--iterations", default="500,2000,8000")
ap.add_argument("--half-extent", type=float, default=125.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-requests", type=int, default=2)
ap.add_argument("--slice", type=int, default=0, help="iterations_per_launch (0: the default, 1024)")
a = ap.parse_args()

sc = config.load_scenario(os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP"))
env = sc["environment"]
START, NOWHERE = (-87.5, -70.0), (5000.0, 5000.0)
w = World(scenarios.JUNCTION_PARAMS)
rows = []
for iters in [int(x) for x in a.iterations.split(",")]:
    p = gp.params_from_config(sc["config"], sample_half_extent=a.half_extent, max_iterations=iters, iterations_per_launch=a.slice)
    w.planner_enable(env, p)
    for n in [int(x) for x in a.requests.split(",")]:
        reqs = [(START, NOWHERE, 1000 + i) for i in range(n)]
        res = w.plan_paths(reqs)  # warm-up (sizes the trees, grants the LDS)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = w.plan_paths(reqs)
            times.append(time.perf_counter() - t0)
        assert all(r["status"] == gp.PLAN_MAX_ITERATIONS and r["iterations"] == iters for r in res)
        nodes = statistics.mean(r["n_nodes"] for r in res)
        k = max(1, min(a.host_requests, n))
        t0 = time.perf_counter()
        ref = gp.plan_paths(env, reqs[:k], p)
        host = (time.perf_counter() - t0) / k * n
        assert all(r["n_nodes"] == d["n_nodes"] and r["wyrand_state"] == d["wyrand_state"] for r, d in zip(ref, res))
        row = {"requests": n, "iterations": iters, "mean_nodes": round(nodes, 1), "device_ms": round(1e3 * statistics.median(times), 3),
               "device_us_per_iteration": round(1e6 * statistics.median(times) / iters, 3), "host_ms": round(1e3 * host, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
print("\n| requests | iterations | nodes (mean) | device ms | device us / iteration | host restatement ms |")
print("|---:|---:|---:|---:|---:|---:|")
for r in rows:
    print(f"| {r['requests']} | {r['iterations']} | {r['mean_nodes']} | {r['device_ms']} | {r['device_us_per_iteration']} | {r['host_ms']} |")
