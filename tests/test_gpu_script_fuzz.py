"""Cross-feature script fuzz: every world mutator in one seeded script (tests/script_fuzz.py), engine against the extended CPU
oracle, bit for bit — beliefs, connection sets, message counts, robot counts and the topology passes' return values at every
compare point.  The scripts, their seeds and what they are known to contain are pinned on the oracle alone by
tests/test_script_fuzz_recipes.py.

Much of the engine's host code is a choice between code paths that depends on the world's history (in place or laid out again,
appended or rebuilt, posted or launched, frozen or thawing).  The runner writes down which of them every stretch of a script
took (script_fuzz.Probe: reads that cost nothing where they are made), and the last test asserts that the scripts crossed every
path they are meant to cross: a generator or an engine that stops reaching one fails here, it does not pass vacuously.

What the scripts found when they were written — robots that join while a factor kind is switched off, the completion handler
while dynamics factors are off and before the world's first iteration — is fixed in the engine and pinned by named tests in
tests/test_gpu_spawn_in_place.py and tests/test_gpu_global_paths.py."""
import collections

import pytest

import script_fuzz as F
from test_script_fuzz_recipes import SEEDS

pytestmark = pytest.mark.gpu

SEGMENTS, RESIDENT, POSTED = 0, 1, 2   # MGX_SWEEP_FORM_*
IR_NONE, IR_STAGED = 0, 2              # MGX_SWEEP_IR_*
EN_IR = 2                              # MGX_FACTOR_INTERROBOT
TALLY = collections.Counter()          # path -> stretches of a script that took it
DECLINED = collections.Counter()       # seed -> resident launches the residency census declined (shared device)

def _tally(script, res):
    for rec in res.records:
        kinds, tags = rec["kinds"], rec["tags"]
        if rec["schedules"]:
            TALLY[{SEGMENTS: "form: launch per segment", RESIDENT: "form: resident", POSTED: "form: posted"}.get(rec["form"], f"form {rec['form']}")] += 1
            if rec["ir_mode"] == IR_STAGED:
                TALLY["inter-robot mode: staged"] += 1
            if rec["ir_mode"] == IR_NONE:
                TALLY["inter-robot mode: none"] += 1
                if not rec["mask"] & EN_IR:  # (the generator's mask)
                    TALLY["inter-robot mode: none after a switch-off"] += 1
            if rec["thawing"]:
                TALLY["a schedule entered while thawing"] += 1
        if "late_add" in kinds:
            appended, _, fell_back = rec["d_append"]
            if appended and not rec["d_layout"][0]:
                TALLY["late add: appended in place"] += 1
            if script.reserve and "outgrows" in tags and fell_back and rec["d_layout"][0]:
                TALLY["late add: full layout, the reserved world outgrew its room"] += 1
            if not script.reserve and rec["d_layout"][0] and not appended:
                TALLY["late add: full layout, unreserved world"] += 1
        if "handler" in kinds:
            if "handler_no_switch_before" in tags and rec["d_layout"] == (0, 0):
                TALLY["apply_global_paths: in place"] += 1
            if "handler_after_switch" in tags and rec["d_layout"][0] and rec["d_layout"][1]:
                TALLY["apply_global_paths: fallback after a switch"] += 1
        plans, schedules, _ = rec["d_post"]
        if schedules > plans:
            TALLY["post merge: several schedules in one plan"] += 1
    if res.batch_end is not None:
        schedules, launches = res.batch_end
        assert schedules == sum(1 for op in script.ops if op.steps is not None), (schedules, script.describe())  # (a tick is no recorded schedule)
        if launches < schedules:
            TALLY["batch: schedules merged into fewer launches"] += 1


def run_one(seed):
    script = F.make_script(seed)
    eng, ref = F.build_worlds(script)
    res = F.run(script, eng, ref)
    assert all(res.finite) and res.n_compared == len(script.compare_after)
    DECLINED[seed] = eng.resident_stats()[1]
    _tally(script, res)
    print(f"[script fuzz {seed}] {script.scenario['name']}, dress {script.dress}, reserve {script.reserve}: {len(res.records)} stretches, "
          f"forms {dict(collections.Counter(r['form'] for r in res.records if r['schedules']))}, linger {eng.linger_stats()}, "
          f"post merge {eng.post_merge_stats()}, layouts {eng.layout_stats()}, appends {eng.append_stats()}, batch {res.batch_end}")


@pytest.mark.parametrize("seed", SEEDS)
def test_script(seed):
    run_one(seed)


REQUIRED = ["form: launch per segment", "form: resident", "form: posted", "inter-robot mode: none after a switch-off", "inter-robot mode: staged",
            "late add: appended in place", "late add: full layout, the reserved world outgrew its room", "late add: full layout, unreserved world",
            "apply_global_paths: in place", "apply_global_paths: fallback after a switch", "a schedule entered while thawing",
            "batch: schedules merged into fewer launches"]
# Resident and posted depend on the shared device granting the launch.  So does the batch figure, a deviation from the issue that
# lets only those two skip: mgx_batch_end reports schedules and launches, a batch merges schedules into ONE resident launch, and
# launch by launch there are never fewer launches than schedules.
NEEDS_THE_LAUNCH_GRANTED = ("form: resident", "form: posted", "batch: schedules merged into fewer launches")


def test_the_scripts_crossed_every_path():
    print("paths crossed: " + ", ".join(f"{k} x {TALLY[k]}" for k in sorted(TALLY)))
    assert len(DECLINED) == len(SEEDS), "run with the scripts: this test reads what they wrote down"
    hard = [k for k in REQUIRED if not TALLY[k] and k not in NEEDS_THE_LAUNCH_GRANTED]
    assert not hard, (hard, dict(TALLY))
    soft = [k for k in NEEDS_THE_LAUNCH_GRANTED if not TALLY[k]]
    if soft:
        declined = sum(DECLINED.values())
        assert declined, (soft, dict(TALLY))  # (nothing was declined: the scripts themselves never got there)
        pytest.skip(f"{soft}: {declined} resident launch(es) declined by the residency census (shared GPU); every other path was crossed")
