"""The divisions by invariant divisors (gbp_math.h: sdf_value, obstacle_slope, interrobot_slopes) inside the sweep kernels:
one small world that meets every branch of them, against the CPU oracle bit for bit after 1, 2 and 12 iterations — through a
resident launch with lingering on, and launch by launch.

The world (6 robots x 8 variables, obstacle and inter-robot factors, robots 0 .. 4 connected to each other):
  robots 0, 1   at the same position.  Their factors keep the reference's tiny offset (1e-6 x the factor's number), so r is about
                1e-6, not 0: the short form runs.  r == 0 exactly (the guard's division, cl = -inf) poisons every robot it
                touches with NaNs and is left to tests/test_invariant_divisions.py on the CPU — this world does not reach it
  robots 2, 3   1 m apart: inside the safety distance (2.2 m)
  robot  4      more than 4 m from everyone: outside it
  robot  5      far away, a prior mean of 1e308 on its last variable: its beliefs leave the finite range
  the image     a 6 x 6 m map under robots that spread over 12 m (taps outside the image), with red = 0 and red = 255
                pixels and a ramp of every value in between under the robots' paths
"""
import numpy as np
import pytest

import oracle
from magics_amd import World, hostlib, scenarios as S

pytestmark = pytest.mark.gpu

K = 8
EXT_INT = 3  # one external + one internal iteration


def _scenario():
    S.HORIZON_FOR_K[K] = next(h for h in range(1, 200) if len(hostlib.variable_timesteps(h, 3)) == K)
    try:
        sc = S.grid_scenario(6, K, interrobot=True, comm_radius=1000.0, obstacles=False, pitch=2.0)
    finally:
        del S.HORIZON_FOR_K[K]
    starts = [(-1.0, 0.5), (-1.0, 0.5), (1.0, -1.0), (1.0, 0.0), (-5.5, 5.0), (30.0, 30.0)]
    for rb, (x, y) in zip(sc["robots"], starts):
        m = np.array(rb["mean0"], dtype=np.float64)
        m[:, 0] += x - m[0, 0]
        m[:, 1] += y - m[0, 1]
        rb["mean0"] = m
    sc["robots"][5]["mean0"][K - 1, 0] = 1e308
    # robots 0 .. 4 all hear each other; robot 5 is out of range (its NaNs stay its own, the others keep numbers to compare)
    sc["positions"] = np.array(starts)
    sc["ir"] = S.number_ir_pairs(S.neighbour_pairs(sc["positions"], 9.0), K)
    # the map: a horizontal ramp over all 256 values (four pixel columns each would be 1024 px: one column each, 256 px wide),
    # a black and a white band on top
    ramp = np.tile(np.arange(256, dtype=np.uint8), (64, 1))
    ramp[:8, :] = 0
    ramp[8:16, :] = 255
    rgb = np.stack([ramp, np.zeros_like(ramp), np.zeros_like(ramp)], axis=2)
    sc["sdf"] = dict(rgb=rgb, world_w=6.0, world_h=6.0)
    return sc


@pytest.fixture(scope="module")
def world_and_oracle():
    sc = _scenario()
    ref = oracle.OracleWorld(sc["params"])
    S.populate(ref, sc)
    beliefs = []
    for steps in ([EXT_INT], [EXT_INT], [EXT_INT] * 10):  # after 1, 2 and 12 iterations
        ref.iterate(steps)
        beliefs.append([a.copy() for a in ref.read_beliefs()])
    return sc, beliefs


class _Frozen:
    def __init__(self, beliefs):
        self._b = beliefs

    def read_beliefs(self):
        return self._b


@pytest.mark.parametrize("form", ["resident_lingering", "launch_per_segment"])
def test_small_world_bit_identical(world_and_oracle, form):
    sc, beliefs = world_and_oracle
    eng = World(sc["params"])
    S.populate(eng, sc)
    if form == "launch_per_segment":
        eng.set_resident_launches(False)
    else:
        eng.set_linger(50000)
    declined0 = eng.resident_stats()[1]
    rows = 5 * K  # robots 0 .. 4; robot 5's variables follow
    for n, steps, want in zip((1, 2, 12), ([EXT_INT], [EXT_INT], [EXT_INT] * 10), beliefs):
        eng.iterate(steps)
        if form != "launch_per_segment" and eng.resident_stats()[1] != declined0:
            pytest.skip(f"{form}: resident launch declined by the residency census (shared GPU)")
        nonfinite = 0
        for name, a, b in zip(("eta", "lam", "mean"), eng.read_beliefs(), want):
            # robots 0 .. 4: the same bits, no allowance (NaNs, if any, in the same places)
            assert np.array_equal(a[:rows], b[:rows], equal_nan=True), f"{form}, {n} iterations: {name} of robots 0..4 differs"
            # robot 5, whose beliefs leave the finite range: identical wherever the oracle holds a number or an infinity; where the
            # oracle holds a NaN the engine may hold a number (it never multiplies by a Jacobian's structural zeros)
            a5, b5 = a[rows:], b[rows:]
            assert np.array_equal(a5[~np.isnan(b5)], b5[~np.isnan(b5)]), f"{form}, {n} iterations: {name} of robot 5 differs where the oracle holds a number"
            nonfinite += int((~np.isfinite(b5)).sum())
        if n == 12:
            assert nonfinite > 0, "robot 5 was meant to leave the finite range"
    form_ran = eng.last_sweep()[2]
    assert form_ran in ((0,) if form == "launch_per_segment" else (1, 2)), eng.last_sweep()
