"""What a burst of global plans costs (profiles/global_planner.md): requests x tree size -> milliseconds, the engine's planner
(mgx_plan_paths: one workgroup per request, bounded launches) against the host restatement of the same specification
(magics_amd/global_planner.py), on the Solo GP map.

    python tools/planner_bench.py [--requests 1,8,64] [--iterations 500,2000,8000] [--half-extent 125] [--reps 5] [--host-requests 2]
                                  [--group-set]

    python tools/planner_bench.py --sliced [--ticks 120] [--pending 1,8,64] [--budgets 16,64,256]

--sliced (profiles/planner_sliced.md): what a tick costs while plans ride it.  The tick is tools/dynamic_tick_bench.py's (comms-range
search + factor create / delete + mgx_tick, 1000 x 16); behind every tick goes one mgx_plan_advance when requests are pending, as
mgx_planner_set_tick_budget puts one behind a mission tick.  Wall time per tick as median and quartiles: the plain tick (planner
off), the tick with the planner on and nothing pending, and the tick with 1, 8 and 64 requests pending at budgets 16, 64 and 256
(requests to a goal no tree reaches, so they stay pending for all the ticks measured); beside each, one synchronous mgx_plan_paths
of the same requests.

Every request plans from the scenario's start to a goal no tree reaches (far outside the map), so each one runs exactly
`--iterations` iterations and the tree size is what the sampler grows in them; seeds differ per request.  The device figure is the
median wall time of `--reps` calls after one warm-up call; the restatement is timed on `--host-requests` of the requests and
scaled to the burst (it plans one request after the other).  One JSON line per cell, then the table of the profile.
--group-set (profiles/ensemble_planner.md): every request goes in under group 1, whose parameter set EQUALS the world's
(mgx_planner_set_group_params), so the launch carries the table of sets and every workgroup reads its row: what the sets cost."""
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
ap.add_argument("--group-set", action="store_true", help="every request under a group set equal to the world's parameters")
ap.add_argument("--sliced", action="store_true", help="the cost of a tick while plans ride it")
ap.add_argument("--ticks", type=int, default=120)
ap.add_argument("--pending", default="1,8,64")
ap.add_argument("--budgets", default="16,64,256")
a = ap.parse_args()


def sliced():
    import numpy as np
    from magics_amd import scenarios as S
    sc = config.load_scenario(os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP"))
    env = sc["environment"]
    start, nowhere = (-87.5, -70.0), (5000.0, 5000.0)
    gs = S.grid_scenario(1000, 16, interrobot=True, seed=805)
    gs["ir"] = []
    w = World(gs["params"])
    S.populate(w, gs)
    rng = np.random.default_rng(805)
    base = np.array([[rb["pos"][0], 0.5, rb["pos"][1]] for rb in gs["robots"]], dtype=np.float32)
    tk = S.tick_inputs(gs)
    state = {"next": w.update_topology(base, 8.0, 1)[0]}
    w.iterate(gs["steps"])
    w.synchronize()

    def ticks(n, budget=0):
        """n ticks, each timed on the host from the topology pass to the return of the last enqueue; the device is drained behind
        the block, and the block's wall time per tick (which holds the slices' device time) is returned beside the per-tick times"""
        poss = [base + rng.normal(0, 0.15, size=base.shape).astype(np.float32) for _ in range(n + 5)]
        for pos in poss[:5]:
            state["next"] = w.update_topology(pos, 8.0, state["next"])[0]
            w.tick(steps=gs["steps"], **tk)
        w.synchronize()
        per = []
        t0 = time.perf_counter()
        for pos in poss[5:]:
            b = time.perf_counter()
            state["next"] = w.update_topology(pos, 8.0, state["next"])[0]
            w.tick(steps=gs["steps"], **tk)
            if budget:
                w.plan_advance(budget)
            per.append((time.perf_counter() - b) * 1e6)
        w.synchronize()
        return np.array(per), (time.perf_counter() - t0) / n * 1e6

    def row(name, per, block, **more):
        q1, med, q3 = (float(np.percentile(per, q)) for q in (25, 50, 75))
        r = {"state": name, "tick_us_median": round(med, 1), "tick_us_q1": round(q1, 1), "tick_us_q3": round(q3, 1), "block_us_per_tick": round(block, 1), **more}
        print(json.dumps(r), flush=True)
        return r

    rows = [row("plain tick (planner off)", *ticks(a.ticks))]
    pend = [int(x) for x in a.pending.split(",")]
    budgets = [int(x) for x in a.budgets.split(",")]
    w.planner_enable(env, gp.params_from_config(sc["config"], sample_half_extent=a.half_extent, max_iterations=1000, max_nodes=8192))
    rows.append(row("planner on, nothing pending", *ticks(a.ticks, budget=64)))
    for n in pend:
        reqs = [(start, nowhere, 1000 + i) for i in range(n)]
        for b in budgets:
            # the requests outlast the ticks measured (warm-up ticks included) and end at the limit two slices later
            iters = (a.ticks + 7) * b
            w.planner_enable(env, gp.params_from_config(sc["config"], sample_half_extent=a.half_extent, max_iterations=iters, max_nodes=8192))
            w.plan_paths(reqs)  # warm-up
            t0 = time.perf_counter()
            res = w.plan_paths(reqs)
            sync_ms = (time.perf_counter() - t0) * 1e3
            tickets = w.plan_submit(reqs)
            per, block = ticks(a.ticks, budget=b)
            still = w.plan_pending()
            ended = w.plan_collect(wait=True, capacity=n, point_capacity=1)
            for t in set(tickets) - {d["ticket"] for d in ended}:
                w.plan_cancel(t)
            rows.append(row("%d pending, budget %d" % (n, b), per, block, pending_after=still, slices=a.ticks + 5,
                            synchronous_plan_paths_ms=round(sync_ms, 2), synchronous_iterations=int(res[0]["iterations"]),
                            synchronous_status=sorted({int(r["status"]) for r in res}), synchronous_mean_nodes=round(float(np.mean([r["n_nodes"] for r in res])), 1)))
    rows.append(row("plain tick again (planner on, nothing pending)", *ticks(a.ticks)))
    print("\n| state | tick us, median | q1 | q3 | block us / tick | one synchronous mgx_plan_paths of the same requests, ms |")
    print("|---|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['state']} | {r['tick_us_median']} | {r['tick_us_q1']} | {r['tick_us_q3']} | {r['block_us_per_tick']} | {r.get('synchronous_plan_paths_ms', '')} |")


if a.sliced:
    sliced()
    sys.exit(0)

sc = config.load_scenario(os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP"))
env = sc["environment"]
START, NOWHERE = (-87.5, -70.0), (5000.0, 5000.0)
w = World(scenarios.JUNCTION_PARAMS)
rows = []
for iters in [int(x) for x in a.iterations.split(",")]:
    p = gp.params_from_config(sc["config"], sample_half_extent=a.half_extent, max_iterations=iters, iterations_per_launch=a.slice)
    w.planner_enable(env, p)
    if a.group_set:
        w.planner_set_group_params(1, p)
    for n in [int(x) for x in a.requests.split(",")]:
        reqs = [(START, NOWHERE, 1000 + i) for i in range(n)]
        groups = {"groups": [1] * n} if a.group_set else {}
        res = w.plan_paths(reqs, **groups)  # warm-up (sizes the trees, grants the LDS)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = w.plan_paths(reqs, **groups)
            times.append(time.perf_counter() - t0)
        assert all(r["status"] == gp.PLAN_MAX_ITERATIONS and r["iterations"] == iters for r in res)
        nodes = statistics.mean(r["n_nodes"] for r in res)
        k = max(1, min(a.host_requests, n))
        t0 = time.perf_counter()
        ref = gp.plan_paths(env, reqs[:k], p)
        host = (time.perf_counter() - t0) / k * n
        assert all(r["n_nodes"] == d["n_nodes"] and r["wyrand_state"] == d["wyrand_state"] for r, d in zip(ref, res))
        row = {**({"group_set": True} if a.group_set else {}), "requests": n, "iterations": iters, "mean_nodes": round(nodes, 1), "device_ms": round(1e3 * statistics.median(times), 3),
               "device_us_per_iteration": round(1e6 * statistics.median(times) / iters, 3), "host_ms": round(1e3 * host, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
print("\n| requests | iterations | nodes (mean) | device ms | device us / iteration | host restatement ms |")
print("|---:|---:|---:|---:|---:|---:|")
for r in rows:
    print(f"| {r['requests']} | {r['iterations']} | {r['mean_nodes']} | {r['device_ms']} | {r['device_us_per_iteration']} | {r['host_ms']} |")
