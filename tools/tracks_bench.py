"""What the device trackers cost and save (profiles/tracks.md).  Runs on the GPU, everything in ONE process, the two sides of each
comparison in alternating blocks after a warm-up:

    python tools/tracks_bench.py --part tick        # mission ticks of a 1000 x 16 grid world with inter-robot factors,
                                                    # the tracker pass on / off, blocks of more than a second, each the
                                                    # same ticks of a fresh world
    python tools/tracks_bench.py --part scenarios   # Junction Twoway and Circle Experiment as tools/run_scenarios.py runs them,
                                                    # device trackers against --host-trackers (Simulation(device_trackers=False))

    python tools/tracks_bench.py --part tick --metrics [--no-log]
                                                    # the same with the run metrics carried by the pass of the "on" side (every
                                                    # robot measured against the line from its start to its goal), and with the
                                                    # sample log switched off (profiles/track_metrics.md)

One JSON line per part: medians, the spread (min / max) of the blocks, and the ratio of the medians."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from magics_amd import World, config, sim  # noqa: E402
from magics_amd import scenarios as S  # noqa: E402
from magics_amd.driver import DeviceDriver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["tick", "scenarios", "both"], default="both")
ap.add_argument("--robots", type=int, default=1000)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--ticks", type=int, default=7000, help="per block: more than a second's worth, fewer than the 10000 a robot needs to arrive")
ap.add_argument("--blocks", type=int, default=7, help="per side")
ap.add_argument("--warmup", type=int, default=60)
ap.add_argument("--max-time", type=float, default=60.0, help="simulated seconds per scenario run")
ap.add_argument("--reps", type=int, default=7, help="scenario runs per side")
ap.add_argument("--metrics", action="store_true", help="tick part: the run metrics on in the blocks that have the trackers on")
ap.add_argument("--no-log", action="store_true", help="tick part: the sample log off in the blocks that have the trackers on (needs --metrics)")
a = ap.parse_args()
if a.no_log and not a.metrics:
    ap.error("--no-log needs --metrics (nothing else would be left of the samples)")


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def part_tick():
    sc = S.grid_scenario(a.robots, a.K, interrobot=True, comm_radius=8.0)
    sc["ir"] = []  # the topology pass of the ticks connects who is in range
    n = len(sc["robots"])

    def block(tracks):
        """a fresh world (the robots drive apart as the ticks go by: every block does the same ticks of the same run — the trackers
        do not change a trajectory — so the two sides differ by the pass alone), a warm-up, then the timed ticks"""
        w = World(sc["params"])
        S.populate(w, sc)
        # (the grid's goals, five times as far: 5 km at 5 m/s are 10000 ticks, so nobody arrives inside a block)
        d = DeviceDriver(w, n, a.K, waypoints=[[tuple(rb["pos"] + 5.0 * (rb["goal"] - rb["pos"]))] for rb in sc["robots"]], radii=[rb["radius"] for rb in sc["robots"]],
                         t0=[rb["t0"] for rb in sc["robots"]], steps=sc["steps"], comms_radius=8.0, target_speed=sc["target_speed"])
        if tracks:  # (hz = 10: a sample per robot and tick — room for all of them, nothing is taken inside the timed ticks)
            w.tracks_enable(True, period_ns=100_000_000, tick_ns=100_000_000, next_tick=0, sample_capacity=n * (a.ticks + a.warmup))
            if a.metrics:
                w.track_metrics_enable(True, max_route_points=2)
                for r, rb in enumerate(sc["robots"]):
                    w.track_metrics_set_route(r, [[float(rb["pos"][0]), float(rb["pos"][1])], [float(rb["goal"][0]), float(rb["goal"][1])]])
                if a.no_log:
                    w.tracks_set_logging(False)
        for _ in range(a.warmup):
            d.tick()
        w.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.ticks):
            d.tick()
        w.synchronize()
        wall = time.perf_counter() - t0
        taken = 0
        if tracks:
            got, _, dropped, dist = w.tracks_take()
            assert not dropped and (dist > 0).all()
            taken = len(got)
            assert taken == (0 if a.no_log else n * (a.ticks + a.warmup))
            if a.metrics:
                rec = w.track_metrics_read()
                assert (rec["n_positions"] == a.ticks + a.warmup).all() and (rec["flags"] == 3).all() and (rec["dimensionless_jerk"] >= 0).all()
        assert (d.finished_at < 0).all()  # (nobody has arrived: all robots move in every tick)
        return a.ticks / wall, wall, taken, list(w.last_sweep())
    block(True)  # (code objects, allocator, clocks)
    rates, walls = {"on": [], "off": []}, []
    for _ in range(a.blocks):
        for side in ("off", "on"):
            rate, wall, taken, sweep = block(side == "on")
            rates[side].append(rate)
            walls.append(wall)
    on, off = spread(rates["on"]), spread(rates["off"])
    print(json.dumps({"part": "tick", "robots": n, "K": a.K, "ticks_per_block": a.ticks, "block_seconds_min": round(min(walls), 2),
                      "unit": "mission ticks/s", "metrics": a.metrics, "sample_log": not a.no_log, "trackers_off": off, "trackers_on": on, "on_over_off": round(on["median"] / off["median"], 4),
                      "off_spread_rel": round((off["max"] - off["min"]) / off["median"], 4),
                      "on_spread_rel": round((on["max"] - on["min"]) / on["median"], 4), "samples_per_block": taken,
                      "last_sweep": sweep}), flush=True)


def part_scenarios():
    with open(os.path.join(ROOT, "tests", "golden", "scenarios.json"), encoding="utf-8") as f:
        known = json.load(f)
    for name in ("Junction Twoway", "Circle Experiment"):
        sc = known[name]

        def run(device_trackers):
            t0 = time.perf_counter()
            s = sim.Simulation(sc, World(config.world_params(sc["config"])), device_trackers=device_trackers)
            s.run(max_time=a.max_time)
            s.export()
            wall = time.perf_counter() - t0
            return wall, s
        run(True)  # warm-up: allocations, code objects, clocks
        walls = {"device": [], "host": []}
        for _ in range(a.reps):
            for side in ("host", "device"):
                wall, s = run(side == "device")
                walls[side].append(wall)
        dev, host = spread(walls["device"]), spread(walls["host"])
        trav = [r["travelled"] for r in s.robots]
        print(json.dumps({"part": "scenario", "scenario": name, "simulated_s": round(s.elapsed(), 1), "ticks": s.tick_no, "robots": len(s.robots),
                          "unit": "wall s per run (construction, run, export)", "host_trackers": host, "device_trackers": dev,
                          "device_over_host": round(dev["median"] / host["median"], 4),
                          "host_spread_rel": round((host["max"] - host["min"]) / host["median"], 4),
                          "mean_distance": round(sum(trav) / max(1, len(trav)), 2)}), flush=True)


if a.part in ("tick", "both"):
    part_tick()
if a.part in ("scenarios", "both"):
    part_scenarios()
