"""Post merging (include/mgx.h: mgx_set_post_merge): mgx_iterate calls issued back to back into a launch that lingers are recorded
while the launch is behind and go out together as ONE posted plan.  The bar is the one of every other path — beliefs AND message
counts of the CPU oracle bit for bit, whatever is put between the schedules — and the bookkeeping keeps its meaning: posts and
re-runs count schedules, a merged submission is one launch.  Exact counts are asked of mode 2 only (record whenever a launch
lingers and the plan fits, whatever the device has taken): nothing here depends on how fast the device is."""
import time

import numpy as np
import pytest

import oracle
from magics_amd import MgxError, World, hostlib, scenarios as S

pytestmark = pytest.mark.gpu

SHAPES = [(36, 10), (48, 16), (24, 9)]  # (robots, K): two constant-K kernels and the run-time-K one
MEAN = np.array([0.5, 0.25, 1.0, -1.0])


def _scenario(n, K):
    """robots on a grid with up to eight neighbours each; K = 9 has no entry in the scenarios' horizon table"""
    added = K not in S.HORIZON_FOR_K
    if added:
        S.HORIZON_FOR_K[K] = next(h for h in range(1, 400) if len(hostlib.variable_timesteps(h, 3)) == K)
    try:
        return S.grid_scenario(n, K, interrobot=True, pitch=2.5, comm_radius=4.5)
    finally:
        if added:
            del S.HORIZON_FOR_K[K]


# ---- what is put between the schedules: (name, what it does to a world — the engine or the oracle) ----
def _tick(w, sc, engine):
    w.tick(steps=sc["steps"], **S.tick_inputs(sc))


def _change_priors(w, sc, engine):
    w.change_priors([1, 5], [sc["K"] - 1, 2], np.stack([MEAN, -MEAN]))


def _read(w, sc, engine):
    return w.get_belief(3, sc["K"] - 1)["mean"].copy()


def _explicit_batch(w, sc, engine):
    if engine:
        with w.batch() as b:
            w.iterate(sc["steps"])
            w.iterate(sc["steps"])
        assert (b.schedules, b.launches) == (2, 1), (b.schedules, b.launches)  # (its counters start clean: what was recorded went out first)
    else:
        w.iterate(sc["steps"])
        w.iterate(sc["steps"])


def _linger_off(w, sc, engine):
    if engine:
        w.set_linger(0)


def _sleep(w, sc, engine):
    if engine:
        time.sleep(0.004)  # (the group runs under a bound of 500 us: the launch has gone, what was recorded runs as a launch)


def _unpostable(w, sc, engine):
    w.iterate([2, 3, 3])          # opens with an external iteration: follows in a merge (mode 2) or runs as a launch of its own
    w.iterate(sc["steps"] * 4)    # 41 segments: never recorded, two launches


OPS = [("tick", _tick), ("change_priors", _change_priors), ("belief read", _read), ("explicit batch", _explicit_batch),
       ("set_linger(0)", _linger_off), ("sleep past the bound", _sleep), ("unpostable schedules", _unpostable)]


def _group(w, sc, engine, op):
    """three schedules, the call, three schedules; what the call returned (the belief read: the mean it read)"""
    for _ in range(3):
        w.iterate(sc["steps"])
    got = op(w, sc, engine)
    for _ in range(3):
        w.iterate(sc["steps"])
    return got


_REFERENCE = {}


def _reference(shape):
    """the oracle's beliefs after seven schedules, after every group of the script, and its message counts at the end: once per shape"""
    if shape not in _REFERENCE:
        sc = _scenario(*shape)
        ref = oracle.OracleWorld(sc["params"])
        S.populate(ref, sc)
        for _ in range(7):
            ref.iterate(sc["steps"])
        snaps, returned = [ref.read_beliefs()], []
        for _, op in OPS:
            returned.append(_group(ref, sc, False, op))
            snaps.append(ref.read_beliefs())
        counts = [ref.message_counts(r) for r in range(len(sc["robots"]))]
        _REFERENCE[shape] = (sc, snaps, counts, returned)
    return _REFERENCE[shape]


def _same(got, want, what):
    for name, a, b in zip(("eta", "lam", "mean"), got, want):
        assert np.array_equal(a, b, equal_nan=True), f"{what}: {name} differs from the oracle in {(~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()} elements"


def _engine(shape, mode):
    """the whole script on the engine in `mode`: seven schedules and a read, then every group; the oracle's beliefs after each"""
    sc, snaps, counts, returned = _reference(shape)
    eng = World(sc["params"])
    S.populate(eng, sc)
    eng.set_linger(20000)  # (a bound no host jitter reaches: what is posted and what is launched follows from the calls alone)
    eng.set_post_merge(mode)
    for _ in range(7):
        eng.iterate(sc["steps"])
    assert eng.last_launch_count() == 1  # (a query: it submits what is recorded — ONE post, however many schedules ride in it)
    after_seven = eng.linger_stats(), eng.post_merge_stats()
    _same(eng.read_beliefs(), snaps[0], f"{shape}, mode {mode}: seven schedules")
    for k, (name, op) in enumerate(OPS):
        eng.set_linger(500 if op is _sleep else 20000)
        got = _group(eng, sc, True, op)
        _same(eng.read_beliefs(), snaps[k + 1], f"{shape}, mode {mode}: {name} between the schedules")
        if op is _read:
            assert np.array_equal(got, returned[k])
        if op is _sleep:  # (how many launches and re-runs the pause made of the group is the host's timing: printed, not asked)
            print(f"[post merge {shape}, mode {mode}] after the pause: linger stats {eng.linger_stats()}")
    for r in range(len(sc["robots"])):
        assert eng.message_counts(r) == counts[r], (shape, mode, r)
    return eng, after_seven


@pytest.mark.parametrize("shape", SHAPES)
def test_mode_2_counts_and_interleavings(shape):
    """seven mgx_iterate and a read: launch; three recorded, submitted by the fifth as ONE plan; three more, submitted by the read.
    Then every kind of call between the schedules — each group the oracle's, bit for bit; message counts at the end."""
    eng, (linger, merge) = _engine(shape, 2)
    launches, posts, reruns, ended = linger
    assert launches == 1 and posts + reruns == 6 and ended == 0, linger
    assert merge == (2, 6, 3), merge
    if shape[1] == 9:
        assert eng.last_sweep()[0] == 0  # the run-time-K kernel
    plans, schedules, largest = eng.post_merge_stats()
    assert largest == 3 and schedules > plans


@pytest.mark.parametrize("shape", SHAPES)
def test_modes_0_and_1_compute_the_same(shape):
    """mode 0 (every schedule its own post) and mode 1 (the default: merged while the launch is behind, however far that is) on
    the same script: the oracle's beliefs and message counts, hence each other's; one schedule per plan in mode 0"""
    off, (linger, merge) = _engine(shape, 0)
    assert linger[0] == 1 and linger[1] + linger[2] == 6 and merge[0] == merge[1] == 6 and merge[2] == 1, (linger, merge)
    plans, schedules, largest = off.post_merge_stats()
    assert plans == schedules and largest == 1
    auto, (linger, merge) = _engine(shape, 1)
    assert linger[0] == 1 and linger[1] + linger[2] == 6 and merge[1] == 6 and 2 <= merge[0] <= 6, (linger, merge)
    for a, b in zip(off.read_beliefs(), auto.read_beliefs()):
        assert np.array_equal(a, b, equal_nan=True)


def test_a_bad_step_fails_at_the_call_that_issues_it():
    """... in a call that would only have been recorded too; the world goes on as if the call had not been made"""
    shape = SHAPES[0]
    sc, snaps, _, _ = _reference(shape)
    eng = World(sc["params"])
    S.populate(eng, sc)
    eng.set_linger(20000)
    eng.set_post_merge(2)
    for k in range(7):
        eng.iterate(sc["steps"])
        if k in (0, 2, 5):  # behind the launch (the next call would be recorded), with schedules recorded, behind a merged post
            with pytest.raises(MgxError, match="bad step 1"):
                eng.iterate([3, 8, 3])
    assert eng.post_merge_stats() == (2, 6, 3)
    _same(eng.read_beliefs(), snaps[0], "seven schedules with refused calls in between")
