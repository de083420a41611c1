"""The cross-feature scripts of tests/script_fuzz.py on the extended CPU oracle alone: what tests/test_gpu_script_fuzz.py relies
on is pinned here, so that the GPU half can fail only because of the engine.

* every listed script keeps the oracle's beliefs finite at every compare point and at the end.  Worlds with inter-robot AND
  tracking factors leave the finite range by the reference's own arithmetic on many inputs; a seed that does is
  not in SEEDS — it is never kept with a weaker comparison.  SEEDS was found by running test_finite_throughout over 0 .. 63 (13 of the 64 left);
* over SEEDS every kind of operation occurs often enough and every ordered pair of MUST_MEET occurs within one script;
* for every kind there is a listed script that ends elsewhere when the calls of that kind are left out;
* the dress is engine-only: on the oracle a dress operation does nothing."""
import collections

import numpy as np
import pytest

import script_fuzz as F

SEEDS = [0, 1, 2, 3, 5, 7, 8, 9, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 23, 24, 25, 27, 29, 30, 31, 33, 34, 35, 37, 39, 41, 42, 43, 44, 45,
         47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 59, 60, 61, 62, 63]

# (name, first, second, within): `first` before `second` in one script, at most `within` operations later (None: anywhere later);
# first None: `second` occurs at all.  A key is a kind or a tag of the generator (script_fuzz.make_script).
MUST_MEET = [
    ("switch -> late add", "switch", "late_add", None),
    ("late add -> multiplier", "late_add", "multiplier", None),
    ("switch -> completion handler", "switch", "handler_after_switch", None),
    ("completion handler with no switch before it", None, "handler_no_switch_before", None),
    ("connect while off -> switch on", "connect_off", "ir_on", None),
    ("remove -> late add", "remove", "late_add", None),
    ("switch on -> switch off within two ops (thaw interrupted)", "switch_on", "switch_off", 2),
    ("multiplier while off -> switch on", "multiplier_off", "ir_on", None),
    ("tracking path -> switch of the tracking kind", "tracking_path", "switch_tracking", None),
    ("topology pass -> completion handler", "topology", "handler", None),
    ("late add -> topology pass", "late_add", "topology", None),
    ("late add -> completion handler", "late_add", "handler", None),
    ("remove -> topology pass", "remove", "topology", None),
    ("topology pass while off -> switch on", "topology_off", "ir_on", None),
    ("a switch before the first iteration", None, "before_first_iteration", None),
    ("a late add that outgrows the reservation", None, "outgrows", None),
]

_RUNS = {}


def _oracle_run(seed):
    """the script of `seed` on the oracle, once per session: (script, Result)"""
    if seed not in _RUNS:
        sp = F.make_script(seed)
        _, ref = F.build_worlds(sp, engine=False)
        _RUNS[seed] = (sp, F.run(sp, None, ref))
    return _RUNS[seed]


def _final(script):
    _, ref = F.build_worlds(script, engine=False)
    return F.run(script, None, ref).final


def _has(op, key):
    return op.kind == key or key in op.tags


def meets(script, first, second, within):
    ops = [op for op in script.ops if not op.dress]
    for j, b in enumerate(ops):
        if not _has(b, second):
            continue
        if first is None:
            return True
        lo = 0 if within is None else max(0, j - within)
        if any(_has(a, first) for a in ops[lo:j]):
            return True
    return False


def test_the_list_is_long_enough_and_the_generator_deterministic():
    assert len(SEEDS) >= 24 and len(set(SEEDS)) == len(SEEDS)
    for seed in SEEDS[:4]:
        a, b = F.make_script(seed), F.make_script(seed)
        assert a.describe() == b.describe() and a.compare_after == b.compare_after and a.dress == b.dress and a.reserve == b.reserve


def test_scenarios_are_the_small_ones():
    seen = collections.Counter()
    for seed in SEEDS:
        sp, _ = _oracle_run(seed)
        sc = sp.scenario
        assert 6 <= len(sc["robots"]) <= 12 and sc["K"] in F.KS and len(sp.first["robots"]) == len(sc["robots"]) - F.HELD_BACK
        assert bool(sc["params"]["enable_mask"] & 8) == (seed % 2 == 0)
        assert len(sp.first["ir"]) < len([c for c in sc["ir"] if max(c[:2]) < len(sp.first["robots"])])  # ragged
        assert bool(sp.first["ir"]) == (seed % 4 != 3)  # (every fourth world starts unconnected)
        assert max(sp.compare_after) == len(sp.ops) - 1
        seen[sc["K"]] += 1
        seen["reserved" if sp.reserve else "unreserved"] += 1
        seen["batch" if sp.dress["batch"] else "no batch"] += 1
        seen[f"resident {sp.dress['resident']}"] += 1
        seen[f"linger {sp.dress['linger']}"] += 1
        seen[f"post merge {sp.dress['post_merge']}"] += 1
        seen[f"{len(sp.compare_after)} compare points" if len(sp.compare_after) <= 2 else "compared along the way"] += 1
    print(dict(seen))
    for key in (*F.KS, "reserved", "unreserved", "batch", "no batch", "resident on", "resident off", "resident off_then_on", "resident on_then_off",
                "linger 0", "linger None", "post merge 0", "post merge 1", "post merge 2", "compared along the way"):
        assert seen[key] > 0, (key, dict(seen))
    assert seen["1 compare points"] + seen["2 compare points"] > 0, dict(seen)  # (end only: nothing read in between ends a launch)


@pytest.mark.parametrize("seed", SEEDS)
def test_finite_throughout(seed):
    sp, res = _oracle_run(seed)
    assert len(res.finite) == len(sp.compare_after)
    assert all(res.finite), f"seed {seed}: the oracle's beliefs are not finite at compare points {[i for i, f in enumerate(res.finite) if not f]}"
    assert all(np.isfinite(x).all() for x in res.final)


def test_every_kind_occurs():
    count = collections.Counter()
    for seed in SEEDS:
        count.update(_oracle_run(seed)[0].kinds())
    print({k: count[k] for k in F.KINDS})
    assert set(count) == set(F.KINDS)
    assert all(count[k] >= 5 for k in F.KINDS), dict(count)


@pytest.mark.parametrize("name,first,second,within", MUST_MEET, ids=[m[0] for m in MUST_MEET])
def test_must_meet(name, first, second, within):
    where = [seed for seed in SEEDS if meets(_oracle_run(seed)[0], first, second, within)]
    print(f"{name}: seeds {where}")
    assert where, name


@pytest.mark.parametrize("kind", F.KINDS)
def test_each_kind_matters(kind):
    """the same script without the calls of one kind ends elsewhere — for at least one listed script"""
    tried = 0
    for seed in SEEDS:
        sp, res = _oracle_run(seed)
        if kind not in sp.kinds():
            continue
        tried += 1
        final = _final(sp.without(kind))
        if not F._same_beliefs(final, res.final):
            print(f"{kind}: seed {seed} ends elsewhere without it ({tried} tried)")
            return
    raise AssertionError(f"{kind}: none of the {tried} listed scripts that use it ends elsewhere without it")


def test_leaving_nothing_out_changes_nothing():
    sp, res = _oracle_run(SEEDS[0])
    assert F._same_beliefs(_final(sp.without("no such kind")), res.final)


def test_dress_is_engine_only():
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"a dress operation called {name} on the oracle")
    n_dress = 0
    for seed in SEEDS:
        sp, _ = _oracle_run(seed)
        for op in sp.ops:
            if op.dress:
                sp.reset("oracle")
                op.apply(Untouchable(), "oracle")
                n_dress += 1
    assert n_dress >= 3 * len(SEEDS)
    seed = next(s for s in SEEDS if _oracle_run(s)[0].dress["batch"])
    sp, res = _oracle_run(seed)
    bare = sp.undressed()
    assert len(bare.ops) < len(sp.ops) and not any(op.dress for op in bare.ops) and len(bare.compare_after) == len(sp.compare_after) - 1
    assert F._same_beliefs(_final(bare), res.final)
