"""Many scenario runs as ONE Ensemble against the same runs one after another (profiles/ensemble.md).

Five workloads, all from tests/golden/scenarios.json: the reference's communications-failure experiment as its script runs it — 5
seeds x 8 failure rates, 21 robots per run: 40 members —, the Environment Obstacles Experiment with 32 seeds, and the Varying Network
Connectivity Experiment as its script runs it — 5 seeds x comms radii 20 / 40 / 60 / 80, 30 robots per run: 20 members that differ in
their comms radius —, and a subset of the Iteration Amount Experiment as its script runs it — the script's 5 seeds x internal 1 / 5 / 21
x external 1 / 5 / 21 of its 1, 2, 3, 5, 8, 13, 21, 34 each, 25 robots per run: 45 members that differ in their GBP iteration
schedule, so the ensemble's ticks run MIXED (launches per tick and the workgroups that sat launches out are reported) —, and the
Structured Junction Twoway experiment as its script runs it — seed 0, tracking factors on and off x failure rates 0.0 .. 0.7: 16
members that differ in gbp.factors-enabled, so the world is MASKED and every tick a group plan (mgx_group_enabled_stats).  For each:
  ensemble   the members as robot groups of one world (magics_amd/ensemble.py): wall time, member ticks per second, the kernel the
             neighbour search ran, the resident schedule launches (ran / declined);
  solo       the same members one after another, each a Simulation on a world of its own: run(chunk=1) and run(chunk=256).
Every figure is a host clock around a whole run that ends in a device synchronisation, world creation and set-up included (that is
what a sweep of runs pays); one untimed warm-up run in front, --reps timed repetitions (default 5): median, min, max.
The solo part needs nothing of the ensemble: `--solo` runs it alone, also from the root of an older checkout
(python <this file> --solo), which is how the figures of the parent commit are taken.

--only WORD keeps the workloads whose name contains WORD.  --observers runs the ensemble with environment_collisions=True,
device_metrics=True, sample_log=False (the figures the Environment Obstacles analysis reads), for a run against the same without.

--ensemble-sigma-tracking S1,S2,.. adds a sixth workload: Structured Junction Twoway, every gbp.sigma-factor-tracking of the list x
5 seeds (the sigma sweep of the reference's Collaborative GP experiment on a scenario without the global planner) — members that
differ in a factor sigma, so the world runs as a masked one does (mgx_set_group_sigmas).

--ensemble-masked-resident adds the form `ensemble_masked_resident`: the ensemble with masked_resident=True, whose masked world runs
the ticks its members share a schedule in as resident launches (mgx_set_group_resident); its row reports the launches of the masked
form, the schedules posted into them and the fall-backs.  --by-turns runs the timed repetitions of all forms by turns (one of each,
then the next of each) instead of form after form.

usage: python tools/ensemble_bench.py [--solo | --ensemble] [--ensemble-masked-resident] [--ensemble-sigma-tracking S1,S2,..] [--by-turns] [--only WORD] [--observers] [--reps N]
       [--max-time S] [--out FILE.json]"""
import copy
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
from magics_amd import World, config, sim  # noqa: E402

args = sys.argv[1:]


def option(flag, kind, default):
    if flag in args:
        i = args.index(flag)
        v = kind(args[i + 1])
        del args[i:i + 2]
        return v
    return default


reps, max_time, out_file = option("--reps", int, 5), option("--max-time", float, 30.0), option("--out", str, None)
only, observers = option("--only", str, ""), "--observers" in args
only_solo, only_ensemble = "--solo" in args, "--ensemble" in args
masked_resident, by_turns = "--ensemble-masked-resident" in args, "--by-turns" in args
sigma_tracking = option("--ensemble-sigma-tracking", lambda text: [config.f32(float(x)) for x in text.split(",")], None)   # (f32 as the config file's own)
OBSERVERS = {"environment_collisions": True, "device_metrics": True, "sample_log": False} if observers else {}
with open(os.path.join("tests", "golden", "scenarios.json"), encoding="utf-8") as f:
    known = json.load(f)


def members(name, seeds, rates, radii=(None,), amounts=(None,), tracking=(None,), sigma_trk=(None,)):
    out = []
    for sig, trk, amount in [(s, t, a) for s in sigma_trk for t in tracking for a in amounts]:
        for radius in radii:
            for rate in rates:
                for seed in seeds:
                    sc = copy.deepcopy(known[name])
                    sc["config"]["simulation"]["prng-seed"] = seed
                    if trk is not None:
                        sc["config"]["gbp"]["factors-enabled"]["tracking"] = trk
                    if sig is not None:
                        sc["config"]["gbp"]["sigma-factor-tracking"] = sig
                    if rate is not None:
                        sc["config"]["robot"]["communication"]["failure-rate"] = rate
                    if radius is not None:
                        sc["config"]["robot"]["communication"]["radius"] = radius
                    if amount is not None:
                        sc["config"]["gbp"]["iteration-schedule"].update({"internal": amount[0], "external": amount[1]})
                    out.append(sc)
    return out


WORKLOADS = {
    "comms-failure 5 seeds x 8 rates": lambda: members("Communications Failure Experiment", [0, 31, 227, 252, 805], [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7]),
    "environment-obstacles 32 seeds": lambda: members("Environment Obstacles Experiment", list(range(100, 132)), [None]),
    "network-connectivity 5 seeds x 4 radii": lambda: members("Varying Network Connectivity Experiment", [0, 31, 227, 252, 805], [None],
                                                              [20.0, 40.0, 60.0, 80.0]),
    "iteration-amount 5 seeds x 3 internal x 3 external": lambda: members("Iteration Amount Experiment", [0, 31, 227, 252, 805], [None],
                                                                          amounts=[(i, e) for i in (1, 5, 21) for e in (1, 5, 21)]),
    "structured-junction-twoway tracking on / off x 8 rates": lambda: members("Structured Junction Twoway", [0], [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7],
                                                                              tracking=[True, False]),
}


if sigma_tracking:
    WORKLOADS["structured-junction-twoway sigma-tracking " + " / ".join(f"{x:g}" for x in sigma_tracking) + " x 5 seeds"] = lambda: members(
        "Structured Junction Twoway", [0, 31, 227, 252, 805], [None], sigma_trk=sigma_tracking)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs), "runs": [round(x, 4) for x in xs]}


def run_solo(scs, chunk):
    ticks = 0
    t0 = time.perf_counter()
    for sc in scs:
        s = sim.Simulation(copy.deepcopy(sc), World(config.world_params(sc["config"])), **OBSERVERS)
        s.run(max_time=max_time, chunk=chunk)
        s.w.synchronize()
        ticks += s.tick_no
    return time.perf_counter() - t0, ticks, {}


def run_ensemble(scs, knob=False):
    from magics_amd import ensemble
    t0 = time.perf_counter()
    e = ensemble.Ensemble([copy.deepcopy(sc) for sc in scs], World(config.world_params(scs[0]["config"])), **({"masked_resident": True} if knob else {}),
                          **OBSERVERS)
    e.run(max_time=max_time)
    e.world.synchronize()
    wall = time.perf_counter() - t0
    ran, declined, _ = e.world.resident_stats()
    lingered, posted = e.world.linger_stats()[:2]
    mixed = {}
    if hasattr(e.world, "group_enabled_stats"):
        plans, launches = e.world.group_enabled_stats()
        if plans:   # (a masked world: every tick's schedule a group plan, launch by launch)
            mixed = {"masked_plans": plans, "masked_launches": launches, "launches_per_masked_plan": round(launches / plans, 2)}
    if knob:
        launches, posts, fallbacks = e.world.group_resident_stats()
        mixed = {**mixed, "masked_resident_launches": launches, "masked_resident_posts": posts, "masked_resident_fallbacks": fallbacks}
    if hasattr(e.world, "group_schedule_stats"):
        calls, launches, sat_out = e.world.group_schedule_stats()
        if calls:   # (workgroup launches: one per robot on the device and launch — the world's robots at the end stand for all of them)
            most = launches * e.world.num_robots()[0]
            mixed = {**mixed, "mixed_calls": calls, "mixed_launches": launches, "launches_per_mixed_call": round(launches / calls, 2), "sat_out": sat_out,
                     "workgroup_launches_at_most": most, "sat_out_share_at_least": round(sat_out / max(most, 1), 4)}
    # (mgx_last_search names the kernel of the last search that launched one: the last tick with robots alive)
    return wall, sum(m.tick_no for m in e.members), {"world_ticks": e.tick_no, "robots": e.world.num_robots()[0], "search_kernel": e.world.last_search()[0],
                                                      "resident_launches": ran, "resident_declined": declined, "lingered_launches": lingered,
                                                      "schedules_posted": posted, **mixed}


result = {"max_time": max_time, "reps": reps, "observers": observers, "workloads": {}}
for name, make in WORKLOADS.items():
    if only not in name:
        continue
    scs = make()
    row = {"members": len(scs)}
    forms = []
    if not only_solo:
        forms.append(("ensemble", lambda: run_ensemble(scs)))
        if masked_resident:
            forms.append(("ensemble_masked_resident", lambda: run_ensemble(scs, True)))
    if not only_ensemble:
        forms += [("solo_chunk1", lambda: run_solo(scs, 1)), ("solo_chunk256", lambda: run_solo(scs, 256))]
    taken = {form: ([], [], {}, 0) for form, _ in forms}
    for form, run in ([] if not by_turns else forms):
        run()   # warm-up: code objects, the environment's rasteriser, the allocator
    for form, run in (forms if not by_turns else forms * reps):
        if not by_turns:
            run()   # warm-up, as above
        walls, rates, _, _ = taken[form]
        for _ in range(1 if by_turns else reps):
            gc.collect()   # (untimed: the run before leaves cycles behind, and the run that follows would pay for collecting them)
            wall, ticks, extra = run()
            walls.append(wall)
            rates.append(ticks / wall)
            taken[form] = (walls, rates, extra, ticks)
    for form, _ in forms:
        walls, rates, extra, ticks = taken[form]
        row[form] = {"wall_s": spread(walls), "member_ticks_per_s": spread(rates), "member_ticks": ticks, **extra}
        print(json.dumps({name: {form: row[form]}}), flush=True)
    result["workloads"][name] = row
if out_file:
    os.makedirs(os.path.dirname(out_file) or ".", exist_ok=True)
    with open(out_file, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1)
