"""What the scenario tests of missions of several legs share (tests/test_gpu_sim_legs.py, tests/test_gpu_ensemble_legs.py): Solo
GP's scenario with its one formation's waypoints extended, in memory, to THREE taskpoints — an intermediate one placed so that both
legs are short (35 m up the first corridor, then some 30 m round one corner: about a hundred ticks for the whole mission) — and
what the host restatement of the planner gives for each leg."""
import copy
import os

from magics_amd import config, environment, spawner
from magics_amd import global_planner as gp
from magics_amd.prng import WyRand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLO_GP = os.path.join(ROOT, "tests", "golden", "scenario_files", "Solo GP")
# the planner overrides of the Solo GP tests (tests/test_gpu_sim_global_planner.py says why)
OVERRIDES = {"sample_half_extent": 125.0, "max_iterations": 20000}
BUDGET = 64
# the formation starts at (0.15, 0.1) of the map; these follow, in its relative coordinates
WAYPOINTS = ((0.15, 0.3), (0.25, 0.37))
SEEDS = (805, 12)   # the scenario's own, and another whose legs the planner also finds at the first attempt


def scenario(seed=SEEDS[0]):
    sc = copy.deepcopy(config.load_scenario(SOLO_GP))
    sc["config"]["simulation"]["prng-seed"] = seed
    f = sc["formation"]["formations"][0]
    f["waypoints"] = [{"shape": {"kind": "line-segment", "points": ((x, y), (x, y))}, "projection-strategy": f["waypoints"][0]["projection-strategy"]}
                      for x, y in WAYPOINTS]
    return sc


def expected(sc):
    """on the CPU: the robot the formation spawns (its taskpoints as f32 states, its forked stream's state) and, per leg, the request
    progress_missions makes and what the host restatement plans for it"""
    rng = WyRand(sc["config"]["simulation"]["prng-seed"])
    desc = spawner.spawn_formation(sc["formation"]["formations"][0], sc["config"], environment.world_size(sc["environment"]), rng)[0]
    tps = [tuple(float(v) for v in s[:2]) for s in desc["waypoints"]]
    p = gp.params_from_config(sc["config"], **OVERRIDES)
    legs = []
    for k in range(len(tps) - 1):
        request = (tps[k], tps[k + 1], desc["rng"].state)
        result = gp.plan_paths(sc["environment"], [request], p)[0]
        legs.append({"request": request, "result": result, "slices": gp.slices_needed(result, p, BUDGET)})
    return {"taskpoints": tps, "legs": legs, "params": p}
