"""Runs the reference's scenarios (parsed form: tests/golden/scenarios.json, or directories given on the command
line) headless on the engine and prints what the reference's export would say about them: makespan, robots
finished, distance travelled (with --environment-collisions also the robot-environment contacts, counted on the device).
--global-planner [device|host|sliced] lets `planning-strategy: rrt-star` robots run: their paths come from the engine's planner (or its
host restatement; sliced: the engine's planner with the plans riding the ticks, --plan-budget N iterations per tick and request,
default 64); --planner-half-extent H and --planner-max-iterations N replace the reference's +-2000 sampler and
config.rrt.max-iterations.  Without it those scenarios are left out (named explicitly, they raise).
--host-trackers keeps the position / velocity samples on the host (every tick's Transforms come back, and no distance is
accumulated: mean_distance stays 0): for A/B runs against the device's trackers, which are the default.
--metrics prints the run metrics after each scenario's line — per robot the LDJ, the path deviation figures, distance and mission
duration, then the per-run summaries (Simulation.metrics(); carried on the device unless --host-trackers); with --no-sample-log no
sample is logged on the device and the robots' positions / velocities lists stay empty.
--goal-areas junction|FILE.json records the first arrival of every robot in every goal area (on the device; goal_area.rs:67-103):
"junction" is the two exits of the reference's junction scenario, FILE.json holds a list of boxes [[x0, z0], [x1, z1]]; each
scenario's line then carries the arrivals per area and the throughput the reference's analyse-junction-scenario.py reads out of an
export (robots that started within 50 s and arrived, per second).  --export DIR writes each scenario's export to DIR/<name>.json.
--ensemble-seeds A,B,.. [--ensemble-failure-rates X,Y,..] [--ensemble-comms-radii R1,R2,..] [--ensemble-schedules KIND:INTERNAL:EXTERNAL,..]
[--ensemble-tracking on,off] [--ensemble-sigma-tracking S1,S2,..] [--ensemble-rrt-collision-radii R1,R2,..] [--ensemble-masked-resident]
runs the cross product of ONE scenario — every seed with every failure rate, every comms radius, every GBP iteration schedule
(KIND: centered, soon-as-possible, late-as-possible, interleave-evenly, half-beginning-half-end), gbp.factors-enabled.tracking
on / off, every gbp.sigma-factor-tracking and every rrt.collision-radius (default each: the scenario's own) — as one Ensemble (magics_amd/ensemble.py):
the members are robot groups of one world, one launch per schedule and one synchronisation per tick for all of them, each member
identical to the same run alone.  One line per member — with --environment-collisions, --goal-areas and --metrics (with or
without --no-sample-log) it carries the member's contacts, arrivals and the means of its run metrics; with --export DIR one
export per member, DIR/<name>.seed<A>.rate<X>.radius<R>[.<kind>-<internal>-<external>][.tracking-<on|off>][.sigma-tracking<S>][.rrt-collision-radius<R>].json.
An Ensemble runs `planning-strategy: rrt-star` scenarios with --global-planner sliced (the members' plans ride the world's ticks,
each member's rrt.* a parameter set of its group) or --global-planner host; the synchronous `device` mode and host trackers do
not run in an Ensemble.
--ensemble-masked-resident: members that differ in tracking on / off or in sigma-factor-tracking make the world masked; with this switch its ticks run as resident
launches all the same (Ensemble(masked_resident=True), mgx_set_group_resident) — same results.
usage: python tools/run_scenarios.py [--max-time S] [--goal-areas junction|FILE.json] [--export DIR] [--environment-collisions] [--host-trackers] [--metrics [--no-sample-log]] [--global-planner [device|host|sliced]]
           [--plan-budget N] [--planner-half-extent H] [--planner-max-iterations N]
           [--ensemble-seeds A,B,.. [--ensemble-failure-rates X,Y,..] [--ensemble-comms-radii R1,R2,..] [--ensemble-schedules KIND:I:E,..] [--ensemble-tracking on,off] [--ensemble-sigma-tracking S1,S2,..] [--ensemble-rrt-collision-radii R1,R2,..]
            [--ensemble-masked-resident]]
           [scenario-dir | name ...]"""
import copy
import json
import os
import sys
import time

sys.path.insert(0, ".")
from magics_amd import World, config, sim  # noqa: E402

args = sys.argv[1:]
max_time = 60.0
if "--max-time" in args:
    i = args.index("--max-time")
    max_time = float(args[i + 1])
    del args[i:i + 2]
env_collisions = "--environment-collisions" in args
if env_collisions:
    args.remove("--environment-collisions")
host_trackers = "--host-trackers" in args
if host_trackers:
    args.remove("--host-trackers")
metrics = "--metrics" in args
if metrics:
    args.remove("--metrics")
no_sample_log = "--no-sample-log" in args
if no_sample_log:
    args.remove("--no-sample-log")
if no_sample_log and (not metrics or host_trackers):
    sys.exit("--no-sample-log needs --metrics on the device's trackers")
goal_areas = None
if "--goal-areas" in args:
    i = args.index("--goal-areas")
    goal_areas = args[i + 1]
    if goal_areas != "junction":
        with open(goal_areas, encoding="utf-8") as f:
            goal_areas = json.load(f)
    del args[i:i + 2]
export_dir = None
if "--export" in args:
    i = args.index("--export")
    export_dir = args[i + 1]
    del args[i:i + 2]
global_planner, overrides, mode = None, {}, None
if "--global-planner" in args:
    i = args.index("--global-planner")
    mode = args[i + 1] if i + 1 < len(args) and args[i + 1] in ("device", "host", "sliced") else None
    global_planner = mode if mode in ("host", "sliced") else True
    del args[i:i + (2 if mode else 1)]
plan_budget = 64
if "--plan-budget" in args:
    i = args.index("--plan-budget")
    plan_budget = int(args[i + 1])
    del args[i:i + 2]
for flag, key, kind in (("--planner-half-extent", "sample_half_extent", float), ("--planner-max-iterations", "max_iterations", int)):
    if flag in args:
        i = args.index(flag)
        overrides[key] = kind(args[i + 1])
        del args[i:i + 2]
ensemble_seeds, ensemble_rates, ensemble_radii = None, None, None
if "--ensemble-seeds" in args:
    i = args.index("--ensemble-seeds")
    ensemble_seeds = [int(x) for x in args[i + 1].split(",")]
    del args[i:i + 2]
if "--ensemble-failure-rates" in args:
    i = args.index("--ensemble-failure-rates")
    ensemble_rates = [float(x) for x in args[i + 1].split(",")]
    del args[i:i + 2]
if "--ensemble-comms-radii" in args:
    i = args.index("--ensemble-comms-radii")
    ensemble_radii = [float(x) for x in args[i + 1].split(",")]
    del args[i:i + 2]
ensemble_schedules = None
if "--ensemble-schedules" in args:
    i = args.index("--ensemble-schedules")
    ensemble_schedules = []
    for word in args[i + 1].split(","):
        kind, internal, external = word.split(":")
        if kind not in config.SCHEDULE_KINDS:
            sys.exit(f"--ensemble-schedules: {kind!r} is none of {sorted(config.SCHEDULE_KINDS)}")
        ensemble_schedules.append({"schedule": kind, "internal": int(internal), "external": int(external)})
    del args[i:i + 2]
ensemble_tracking = None
if "--ensemble-tracking" in args:
    i = args.index("--ensemble-tracking")
    words = args[i + 1].split(",")
    if not words or any(x not in ("on", "off") for x in words):
        sys.exit("--ensemble-tracking: a list of on / off")
    ensemble_tracking = [x == "on" for x in words]
    del args[i:i + 2]
ensemble_sigma_tracking = None
if "--ensemble-sigma-tracking" in args:
    i = args.index("--ensemble-sigma-tracking")
    ensemble_sigma_tracking = [config.f32(float(x)) for x in args[i + 1].split(",")]   # (f32 as the config file's own, parse_config)
    if any(not (0.0 < x < float("inf")) for x in ensemble_sigma_tracking):
        sys.exit("--ensemble-sigma-tracking: a list of positive finite sigmas")
    del args[i:i + 2]
ensemble_rrt_radii = None
if "--ensemble-rrt-collision-radii" in args:
    i = args.index("--ensemble-rrt-collision-radii")
    ensemble_rrt_radii = [config.f32(float(x)) for x in args[i + 1].split(",")]   # (f32 as the config file's own, parse_config)
    if any(not (0.0 <= x < float("inf")) for x in ensemble_rrt_radii):
        sys.exit("--ensemble-rrt-collision-radii: a list of finite radii, none negative")
    del args[i:i + 2]
ensemble_masked_resident = "--ensemble-masked-resident" in args
if ensemble_masked_resident:
    args.remove("--ensemble-masked-resident")
if (ensemble_rates or ensemble_radii or ensemble_schedules or ensemble_tracking or ensemble_sigma_tracking or ensemble_rrt_radii or ensemble_masked_resident) and not ensemble_seeds:
    sys.exit("--ensemble-failure-rates, --ensemble-comms-radii, --ensemble-schedules, --ensemble-tracking, --ensemble-sigma-tracking, "
             "--ensemble-rrt-collision-radii and --ensemble-masked-resident need --ensemble-seeds")
if ensemble_seeds and global_planner is True:
    sys.exit("--ensemble-seeds: --global-planner " + ("device" if mode else "without a mode") + " plans synchronously, which would hold every member's "
             "ticks for the slowest plan: it does not run in an Ensemble; --global-planner sliced does (or host, the restatement)")
if ensemble_rrt_radii and not global_planner:
    sys.exit("--ensemble-rrt-collision-radii needs --global-planner sliced or host")
if ensemble_seeds and host_trackers:
    sys.exit("--ensemble-seeds: host trackers do not run in an Ensemble (magics_amd/ensemble.py says why)")
with open(os.path.join("tests", "golden", "scenarios.json"), encoding="utf-8") as f:
    known = json.load(f)
if ensemble_seeds:
    from magics_amd import ensemble  # noqa: E402
    if len(args) != 1:
        sys.exit("--ensemble-seeds runs ONE scenario: name it")
    base = config.load_scenario(args[0]) if os.path.isdir(args[0]) else known[args[0]]
    members = []
    for rrt_radius, sigma_trk, tracking in [(c, s, t) for c in ensemble_rrt_radii or [None] for s in ensemble_sigma_tracking or [None]
                                            for t in ensemble_tracking or [None]]:
        for schedule in ensemble_schedules or [None]:
            for radius in ensemble_radii or [base["config"]["robot"]["communication"]["radius"]]:
                for rate in ensemble_rates or [base["config"]["robot"]["communication"]["failure-rate"]]:
                    for seed in ensemble_seeds:
                        sc = copy.deepcopy(base)
                        sc["config"]["simulation"]["prng-seed"] = seed
                        sc["config"]["robot"]["communication"]["failure-rate"] = rate
                        sc["config"]["robot"]["communication"]["radius"] = radius
                        if schedule is not None:
                            sc["config"]["gbp"]["iteration-schedule"].update(schedule)
                        if tracking is not None:
                            sc["config"]["gbp"]["factors-enabled"]["tracking"] = tracking
                        if sigma_trk is not None:
                            sc["config"]["gbp"]["sigma-factor-tracking"] = sigma_trk
                        if rrt_radius is not None:
                            sc["config"]["rrt"]["collision-radius"] = rrt_radius
                        members.append((seed, rate, radius, sc))
    t0 = time.perf_counter()
    e = ensemble.Ensemble([sc for *_, sc in members], World(config.world_params(base["config"])), environment_collisions=env_collisions,
                          device_metrics=metrics, sample_log=not no_sample_log, goal_areas=goal_areas, masked_resident=ensemble_masked_resident,
                          **({"global_planner": global_planner, "planner_overrides": overrides, "plan_budget": plan_budget} if global_planner else {}))
    e.run(max_time=max_time)
    wall = time.perf_counter() - t0
    stem = os.path.basename(os.path.normpath(base.get("name", args[0])))
    for (seed, rate, radius, sc), m in zip(members, e.members):
        s = m.sim
        done = [r for r in s.robots if r["completed"]]
        trav = [r["travelled"] for r in s.robots]
        figures = m.metrics() if metrics or env_collisions or goal_areas else None
        sch = sc["config"]["gbp"]["iteration-schedule"]
        print(json.dumps({"scenario": sc.get("name", args[0]), "seed": seed, "failure_rate": rate, "comms_radius": radius,
                          **({"schedule": f"{sch['schedule']}:{sch['internal']}:{sch['external']}"} if ensemble_schedules else {}),
                          **({"tracking": sc["config"]["gbp"]["factors-enabled"]["tracking"]} if ensemble_tracking else {}),
                          **({"sigma_tracking": sc["config"]["gbp"]["sigma-factor-tracking"]} if ensemble_sigma_tracking else {}),
                          **({"rrt_collision_radius": sc["config"]["rrt"]["collision-radius"]} if ensemble_rrt_radii else {}),
                          **({"plans": len(s._plan_log), "plans_failed": sum(q["status"] != 0 for q in s._plan_log)} if global_planner else {}),
                          "simulated_s": round(s.elapsed(), 1),
                          "robots": len(s.robots), "finished": len(done), "all_finished": s.finished(), "K": s.K,
                          "mean_distance": round(sum(trav) / max(1, len(trav)), 1),
                          "last_finish_s": round(max((r["finished_at"] for r in done), default=0.0), 1), "topology_events": len(s.events),
                          **({"environment_collisions": figures["collisions"]["environment"]} if env_collisions else {}),
                          **({"goal_arrivals": figures["goal_areas"]["arrivals"], "goal_flow": figures["goal_areas"]["flow"]} if goal_areas else {}),
                          **({"makespan": figures["makespan"], "collisions": figures["collisions"],
                              **{f"mean_{c}": figures["summary"][c]["mean"] for c in ("ldj", "path_deviation", "distance_travelled", "duration")}}
                             if metrics else {})}), flush=True)
        if export_dir:
            os.makedirs(export_dir, exist_ok=True)
            tail = f".{sch['schedule']}-{sch['internal']}-{sch['external']}" if ensemble_schedules else ""
            if ensemble_tracking:
                tail += ".tracking-on" if sc["config"]["gbp"]["factors-enabled"]["tracking"] else ".tracking-off"
            if ensemble_sigma_tracking:
                tail += f".sigma-tracking{sc['config']['gbp']['sigma-factor-tracking']:g}"
            if ensemble_rrt_radii:
                tail += f".rrt-collision-radius{sc['config']['rrt']['collision-radius']:g}"
            with open(os.path.join(export_dir, f"{stem}.seed{seed}.rate{rate:g}.radius{radius:g}{tail}.json"), "w", encoding="utf-8") as f:
                json.dump(m.export(), f)
    mixed_calls, mixed_launches, sat_out = e.world.group_schedule_stats()
    masked_plans, masked_launches = e.world.group_enabled_stats()
    print(json.dumps({"ensemble": len(members), "ticks": e.tick_no, "mixed_calls": mixed_calls, "mixed_launches": mixed_launches, "sat_out": sat_out,
                      "masked_plans": masked_plans, "masked_launches": masked_launches, "member_ticks": sum(m.tick_no for m in e.members), "wall_s": round(wall, 2),
                      "member_ticks_per_s": round(sum(m.tick_no for m in e.members) / wall, 1)}), flush=True)
    sys.exit(0)
names = args or [n for n, sc in sorted(known.items())
                 if (global_planner or all(f["planning-strategy"] == "only-local" for f in sc["formation"]["formations"])) and sum(f["robots"] for f in sc["formation"]["formations"])]
for name in names:
    sc = config.load_scenario(name) if os.path.isdir(name) else known[name]
    t0 = time.perf_counter()
    s = sim.Simulation(sc, World(config.world_params(sc["config"])), environment_collisions=env_collisions,
                       global_planner=global_planner, planner_overrides=overrides, plan_budget=plan_budget,
                       device_trackers=False if host_trackers else None, device_metrics=metrics and not host_trackers, sample_log=not no_sample_log,
                       goal_areas=goal_areas)
    s.run(max_time=max_time)
    wall = time.perf_counter() - t0
    done = [r for r in s.robots if r["completed"]]
    trav = [r["travelled"] for r in s.robots]
    print(json.dumps({"scenario": sc.get("name", name), "simulated_s": round(s.elapsed(), 1), "wall_s": round(wall, 2), "robots": len(s.robots),
                      "finished": len(done), "all_finished": s.finished(), "K": s.K,
                      "mean_distance": round(sum(trav) / max(1, len(trav)), 1),
                      "last_finish_s": round(max((r["finished_at"] for r in done), default=0.0), 1),
                      "topology_events": len(s.events),
                      **({"plans": len(s._plan_log), "plans_failed": sum(q["status"] != 0 for q in s._plan_log)} if global_planner else {}),
                      **({"environment_collisions": sum(h["times"] for h in s.environment_collisions.values())} if env_collisions else {}),
                      **({"goal_arrivals": s.metrics()["goal_areas"]["arrivals"], "goal_flow": s.metrics()["goal_areas"]["flow"]} if goal_areas else {})}),
          flush=True)
    if export_dir:
        os.makedirs(export_dir, exist_ok=True)
        s.export_json(os.path.join(export_dir, os.path.basename(os.path.normpath(sc.get("name", name))) + ".json"))
    if metrics:
        m = s.metrics()
        cols = ("ldj", "path_deviation", "mean_deviation", "max_deviation", "distance_travelled", "duration")
        print("  " + "robot".rjust(8) + "".join(c.rjust(20) for c in cols))
        for rid, row in m["robots"].items():
            print("  " + rid.rjust(8) + "".join(f"{row[c]:20.6f}" for c in cols))
        for stat in ("robots", "mean", "median", "largest", "smallest", "variance", "stdev"):
            print("  " + stat.rjust(8) + "".join((f"{m['summary'][c][stat]:20d}" if stat == "robots" else f"{m['summary'][c][stat]:20.6f}") for c in cols))
        print("  " + json.dumps({"makespan": m["makespan"], "collisions": m["collisions"]}), flush=True)
