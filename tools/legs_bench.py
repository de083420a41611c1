"""Diagnostics for missions of several legs (profiles/mission_legs.md is written from this script's output).
(a) what the legs cost a run that has none: ticks / s of a legless mission run — the shape of tools/scenario_profile.py, Junction
    Twoway for 30 simulated seconds through Simulation.run — for the build named by MGX_LIB (default: the product), one fresh world
    per repetition in one process.  With --parent LIB the script runs itself in fresh child processes, product and LIB in turn, so
    that both are measured in the same call on the same machine, and prints both medians and each build's spread.
(b) the two-leg scenario of the tests (tests/sim_legs_common.py): the ticks between a leg's end and the robot's activation on the
    next leg, and the wall time of those ticks, for global_planner=True and "sliced" at plan_budget=64 — one world per variant.
usage: python tools/legs_bench.py a [repetitions]  |  b  |  --parent LIB [repetitions] [rounds]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def legless(reps, secs=30.0):
    import torch  # noqa: F401
    from magics_amd import World, config, sim
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        sc = json.load(f)["Junction Twoway"]
    rates = []
    for rep in range(reps + 1):  # (the first run warms the process up and is not counted)
        s = sim.Simulation(sc, World(config.world_params(sc["config"])))
        t0 = time.perf_counter()
        s.run(max_time=secs)
        s.w.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            rates.append(s.tick_no / dt)
    print(json.dumps({"lib": os.environ.get("MGX_LIB", "product"), "ticks_per_s": [round(r, 1) for r in rates]}), flush=True)


def between_legs():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from magics_amd import World, config, sim
    from sim_legs_common import BUDGET, OVERRIDES, scenario
    for mode in (True, "sliced"):
        sc = scenario()
        s = sim.Simulation(sc, World(config.world_params(sc["config"])), global_planner=mode, planner_overrides=OVERRIDES, plan_budget=BUDGET)
        ended = woke = None
        wall = 0.0
        while not s.finished() and s.tick_no < 600:
            t0 = time.perf_counter()
            s.tick()
            s.w.synchronize()
            dt = time.perf_counter() - t0
            r = s.robots[0]
            if ended is None and r["leg"] == 1:
                ended = s.tick_no - 1          # the tick the first leg ended in
            if ended is not None and woke is None:
                if r["idle"]:
                    wall += dt                 # the leg-ending tick and every tick the robot waited through
                else:
                    woke = s.tick_no - 1       # the tick whose start handed the next leg over
        print(json.dumps({"global_planner": mode, "plan_budget": BUDGET, "leg_ended_in_tick": ended, "active_from_tick": woke,
                          "ticks_between": None if woke is None else woke - ended, "wall_ms_of_those_ticks": round(wall * 1e3, 3),
                          "mission_ticks": s.tick_no}), flush=True)


def versus(parent, reps, rounds):
    rates = {"product": [], parent: []}
    for _ in range(rounds):
        for lib in ("product", parent):
            env = dict(os.environ)
            env.pop("MGX_LIB", None)
            if lib != "product":
                env["MGX_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "a", str(reps)], env=env, check=True, capture_output=True, text=True, timeout=600)
            rates[lib] += json.loads(out.stdout.strip().splitlines()[-1])["ticks_per_s"]
    res = {lib: {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v), "spread": round(max(v) - min(v), 1), "runs": v}
           for lib, v in rates.items()}
    res["product_not_worse_than_parent_by_more_than_its_spread"] = res["product"]["median"] >= res[parent]["median"] - res[parent]["spread"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--parent":
        versus(a[1], int(a[2]) if len(a) > 2 else 5, int(a[3]) if len(a) > 3 else 2)
    elif a and a[0] == "b":
        between_legs()
    else:
        legless(int(a[1]) if len(a) > 1 else 5)
