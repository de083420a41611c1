"""The grouped seeded scripts of tests/group_fuzz.py on the CPU oracles alone: what tests/test_gpu_group_fuzz.py relies on is pinned
here, so that the GPU half can fail only because of the engine.

* the three scripts of a world share the horizon, the kinds of factors and the obstacle image, carry no dress and none of the
  kinds that cannot run per group, and have their topology passes at the same steps;
* their schedules are ragged — not the same number of segments — at no fewer than half of the steps, so the calls are mixed;
* every kept kind occurs over WORLDS;
* every oracle's beliefs are finite at every compare point and at the end.  Worlds with inter-robot AND tracking factors leave the
  finite range by the reference's own arithmetic on many inputs: a seed that does is not in WORLDS — found by
  running test_finite_throughout over the seeds 0 .. 23 of every horizon (an even seed has tracking factors; K = 21 keeps none
  of those finite)."""
import collections

import numpy as np
import pytest

import group_fuzz as G
import script_fuzz as SF

# (seed, K): two worlds for each of four constant-K kernels and the run-time-K horizon 13
WORLDS = [(0, 10), (1, 10), (1, 12), (2, 12), (1, 13), (10, 13), (1, 16), (10, 16), (1, 21), (3, 21)]

_RUNS = {}


def oracle_runs(seed, K):
    """the three scripts of a world and their oracles' runs, once per session: (scripts, [(Result, held)] per group)"""
    if (seed, K) not in _RUNS:
        scripts = G.make_scripts(seed, K)
        _RUNS[(seed, K)] = (scripts, [G.reference(sp) for sp in scripts])
    return _RUNS[(seed, K)]


def test_worlds_cover_the_horizons():
    assert collections.Counter(K for _, K in WORLDS) == {10: 2, 12: 2, 13: 2, 16: 2, 21: 2} and len(set(WORLDS)) == 10
    assert {seed % 2 for seed, _ in WORLDS} == {0, 1}   # with and without tracking factors


def test_forcing_nothing_leaves_a_seed_its_script():
    """make_script's K and tracking keywords: None is the seed's own script, and a forced value changes nothing else"""
    for seed in (0, 3, 8):
        a, b = SF.make_script(seed), SF.make_script(seed, K=None, tracking=None)
        assert a.describe() == b.describe() and a.compare_after == b.compare_after and a.scenario["K"] == b.scenario["K"]
        c = SF.make_script(seed, K=a.scenario["K"], tracking=seed % 2 == 0)
        assert a.describe() == c.describe() and a.compare_after == c.compare_after


@pytest.mark.parametrize("seed,K", WORLDS)
def test_three_scripts_share_a_world(seed, K):
    scripts, _ = oracle_runs(seed, K)
    assert len(scripts) == G.M and len({sp.seed for sp in scripts}) == G.M
    assert all(sp.scenario["K"] == K and sp.scenario["params"] == scripts[0].scenario["params"] for sp in scripts)
    assert all(sp.scenario["sdf"] is scripts[0].scenario["sdf"] and sp.first["sdf"] is scripts[0].scenario["sdf"] for sp in scripts)
    n_ops = len(scripts[0].ops)
    for sp in scripts:
        assert len(sp.ops) == n_ops and not any(op.dress for op in sp.ops)
        assert not any(op.kind in G.LEFT_OUT and op.call is not None for op in sp.ops)
    for k in range(n_ops):   # a topology pass is one call over all groups
        passes = [op.kind == "topology" or "aligned_topology" in op.tags for op in (sp.ops[k] for sp in scripts)]
        assert all(passes) or not any(passes), (k, passes)
    assert 2 * G.ragged_steps(scripts) >= n_ops, (G.ragged_steps(scripts), n_ops)


def test_every_kept_kind_occurs():
    seen = collections.Counter()
    for seed, K in WORLDS:
        for sp in G.make_scripts(seed, K) if (seed, K) not in _RUNS else _RUNS[(seed, K)][0]:
            seen.update(op.kind for op in sp.ops if op.call is not None or op.kind == "iterate")
    assert set(G.LEFT_OUT) <= set(SF.KINDS) and not set(G.LEFT_OUT) & set(seen)
    missing = [k for k in G.KEPT if not seen[k]]
    assert not missing, (missing, dict(seen))


@pytest.mark.parametrize("seed,K", WORLDS)
def test_finite_throughout(seed, K):
    scripts, runs = oracle_runs(seed, K)
    for g, (sp, (res, held)) in enumerate(zip(scripts, runs)):
        assert res.finite and all(res.finite), (seed, K, g, sp.seed, res.finite)
        assert all(np.isfinite(x).all() for x in res.final)
        assert sorted(held) == sorted(sp.compare_after | {len(sp.ops) - 1})
        for at in held.values():
            assert all(np.isfinite(b).all() for b in at["beliefs"])
