"""Runs the reference's OWN throughput function on a few small exports and records inputs and results in
tests/golden/goal_area_flow.json (data only).  tests/test_goal_areas.py holds magics_amd.sim.goal_flow against it.

Run in the build container (needs /root/reference):  python tests/golden/make_goal_area_fixtures.py

Source, read at generation time and never copied: `extract_data_from_file` (and the `flatten` it calls) of
scripts/analyse-junction-scenario.py:49-109.  Only the two definitions are taken (by `ast`): the module imports plotting
packages at the top that need not be installed, and asserts that a results directory exists.

Exports: only the fields that function reads — goal_areas[*].history, robots[*].mission.started_at, makespan — written by hand
so that every branch of the count is met: a robot that started at exactly the window (left out: `>=`), one that started after
it, a robot in two histories (counted once), a robot in none, a history key that is no robot of the export (never looked at),
counts whose quotient 1 / (50 / n) is not n / 50 in f64.  An export in which nobody arrives is not recorded: the reference's
function divides by zero there."""
import ast
import itertools
import json
import os
import tempfile
from typing import Iterable

REF = "/root/reference/scripts/analyse-junction-scenario.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "goal_area_flow.json")


def definitions(path, names):
    """the named top-level function definitions of a file, executed on their own"""
    tree = ast.parse(open(path, encoding="utf-8").read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    ns = {"json": json, "itertools": itertools, "Iterable": Iterable}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def export(started, histories, makespan):
    """started: robot key -> started_at; histories: per area {robot key: seconds}"""
    box = {"mins": [0.0, 0.0], "maxs": [1.0, 1.0]}
    return {"makespan": makespan, "robots": {k: {"mission": {"started_at": t}} for k, t in started.items()},
            "goal_areas": {str(a): {"aabb": box, "history": h} for a, h in enumerate(histories)}}


def cases():
    out = {}
    # three robots, all early, all arrived: 1 / (50 / 3)
    out["three_of_three"] = export({"0": 0.0, "1": 0.5, "2": 1.0}, [{"0": 7.0, "2": 8.0}, {"1": 7.400000095367432}], 15.0)
    # the window's edge and beyond, a robot in both areas, one in none, a stranger in a history
    out["edges"] = export({"0": 0.0, "1": 49.900000000000006, "2": 50.0, "3": 50.1, "4": 12.0, "5": 3.0, "6": 4.5},
                          [{"0": 7.0, "1": 57.0, "2": 57.5, "4": 19.0, "99": 1.0}, {"0": 9.0, "3": 58.0, "6": 11.5}], 60.0)
    # one robot
    out["one"] = export({"7": 2.0, "8": 2.5}, [{}, {"8": 9.600000381469727}], 10.0)
    # forty-nine early robots that arrived and a fiftieth that did not: a count whose two divisions round
    started = {str(i): i * 1.0 for i in range(60)}
    out["forty_nine"] = export(started, [{str(i): i + 7.0 for i in range(0, 49, 2)}, {str(i): i + 7.5 for i in range(1, 49, 2)}], 70.0)
    return out


if __name__ == "__main__":
    extract, _ = definitions(REF, ["extract_data_from_file", "flatten"])
    extract.__globals__["flatten"] = _
    recorded = {}
    for name, exp in cases().items():
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump(exp, f)
        try:
            value = extract(f.name)
        finally:
            os.unlink(f.name)
        recorded[name] = {"export": exp, "flow": value, "window": 50.0}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"source": "scripts/analyse-junction-scenario.py:49-109 (extract_data_from_file)", "cases": recorded}, f, indent=1)
    print({k: v["flow"] for k, v in recorded.items()})
