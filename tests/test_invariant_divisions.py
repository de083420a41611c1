"""CPU checks of the divisions by invariant divisors in magics_amd/csrc/gbp_math.h (divide3, divide_by_invariant,
obstacle_inv_delta / obstacle_slope, interrobot_slopes): every short form against the plain f64 division it replaces, bit for bit
(memcmp of the doubles), through a test-only g++ build (tests/cpu_math/division_harness.cpp, which also keeps the old forms of
the functions).  Each check returns its number of disagreements; none is tolerated."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from magics_amd import scenarios as S

HERE = os.path.dirname(os.path.abspath(__file__))
N = 10_000_000  # random numerators per divisor
THREADS = min(8, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def D():
    src = os.path.join(HERE, "cpu_math", "division_harness.cpp")
    out = os.path.join(HERE, "cpu_math", "libdivision_harness.so")
    hdr = os.path.join(HERE, "..", "magics_amd", "csrc", "gbp_math.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.d_check_255.restype = C.c_long
    lib.d_check_divisor.restype = C.c_long
    lib.d_check_divisor.argtypes = [C.c_double, C.c_uint64, C.c_long, C.c_int]
    lib.d_short_form_taken.restype = C.c_long
    lib.d_short_form_taken.argtypes = [C.c_double, C.c_uint64, C.c_long]
    lib.d_check_random_divisors.restype = C.c_long
    lib.d_check_random_divisors.argtypes = [C.c_uint64, C.c_int, C.c_long, C.c_int]
    lib.d_check_obstacle_delta.restype = C.c_long
    lib.d_check_obstacle_delta.argtypes = [C.c_double, C.POINTER(C.c_double)]
    lib.d_check_slopes.restype = C.c_long
    lib.d_check_slopes.argtypes = [C.c_uint64, C.c_long, C.c_int]
    lib.d_check_interrobot.restype = C.c_long
    lib.d_check_interrobot.argtypes = [C.c_uint64, C.c_long, C.c_int]
    lib.d_check_obstacle.restype = C.c_long
    lib.d_check_obstacle.argtypes = [C.c_double, C.c_uint64, C.c_long]
    return lib


def _deltas():
    """jacobian_delta = (world_w / image_w + world_h / image_h) / 2 of the worlds the suite and the benchmark build: every committed
    scenario's map (tests/golden/scenarios.json: tile-size metres over `resolution` pixels per tile, whatever the grid), the
    synthetic worlds of scenarios.grid_scenario at the robot counts of BASELINE.json's configs and of the suite, and the circle
    scenario's.  (Every delta a world is ever committed with is also checked by the host itself, against all 65 536 numerators:
    obstacle_inv_delta.)"""
    import json
    out = set()
    with open(os.path.join(HERE, "golden", "scenarios.json")) as fh:
        for sc in json.load(fh).values():
            st = sc["environment"]["tiles"]["settings"]
            for tiles in (1, 2, 3, 5):  # world = tiles x tile-size, image = tiles x resolution: the quotient is rounded per grid
                w, px = tiles * float(st["tile-size"]), tiles * int(st["sdf"]["resolution"])
                out.add((w / px + w / px) / 2.0)
    with open(os.path.join(HERE, "..", "BASELINE.json")) as fh:
        text = fh.read()
    import re
    counts = {int(n) for n in re.findall(r"(\d+) robots", text)} | {4, 6, 8, 9, 12, 16, 100}
    # scenarios.grid_scenario: side = 5 m x robots per side + 50 m; ten pixels per metre with obstacles (scenarios.synthetic_sdf),
    # one white 16 x 16 image without
    for n in sorted(counts):
        for pitch in (5.0, 2.5, 2.0, 1.2):
            world = math.ceil(math.sqrt(n)) * pitch + 50.0
            for px in (int(round(world * 10)), 16):
                out.add((world / px + world / px) / 2.0)
    out.add((200.0 / 200 + 200.0 / 200) / 2.0)  # scenarios.circle_scenario: 4 x radius 50 over 200 px
    out.add((40.0 / 160 + 24.0 / 96) / 2.0)     # the suite's non-square map
    out.add(1.0)                                # no image at all
    return sorted(out)


def _d_safes():
    """safety distances, safety_multiplier x radius: every committed scenario's multiplier (tests/golden/scenarios.json) and the
    two parameter sets of scenarios.py, times the ends and the middle of the scenario's radius range (and four radii drawn
    inside it: the formations draw theirs at random) and the synthetic worlds' radius 1"""
    import json
    f = S.f32w
    out = set()
    rng = np.random.default_rng(5)
    with open(os.path.join(HERE, "golden", "scenarios.json")) as fh:
        for sc in json.load(fh).values():
            rb = sc["config"]["robot"]
            mult, lo, hi = rb["inter-robot-safety-distance-multiplier"], rb["radius"]["min"], rb["radius"]["max"]
            for r in [lo, hi, (lo + hi) / 2.0] + list(rng.uniform(lo, hi, size=4)):
                out.add(float(f(mult) * f(r)))
    for params in (S.JUNCTION_PARAMS, S.CIRCLE_PARAMS):
        for r in (0.5, 1.0, 2.0, 2.5, 3.0):
            out.add(float(params["safety_multiplier"] * f(r)))
    return sorted(out)


def test_red_over_255_all_numerators(D):
    assert D.d_check_255() == 0


@pytest.mark.parametrize("b", _deltas() + _d_safes(), ids=lambda b: f"{b!r}")
def test_divide_by_invariant_scenario_divisors(D, b):
    """jacobian_delta and d_safe values of the committed scenarios and BASELINE.json's configs (their 1 / sigma^2 scalings are
    multiplications already: no division was replaced there): 10^7 random numerators over every exponent, +-0, the extreme
    normals, denormals, +-inf, NaNs, small multiples of the divisor and their neighbours"""
    assert D.d_short_form_taken(b, 3, 100000) > 30000  # the short form is what most of them exercise
    assert D.d_check_divisor(b, 1, N, THREADS) == 0


def test_divide_by_invariant_random_divisors(D):
    """200 random divisors (three in four inside the range that gets a reciprocal, the others anywhere: denormals, huge, inf,
    NaN), each with the same numerator set"""
    assert D.d_check_random_divisors(2, 200, N, THREADS) == 0


@pytest.mark.parametrize("delta", _deltas() + [1e-300, 1e300, 5e-324, 0.0, math.inf, math.nan, -0.1, 3.0, 1.0 / 3.0],
                         ids=lambda b: f"{b!r}")
def test_obstacle_slope_every_sample_pair(D, delta):
    """(h_i - h_0) / delta for all 257 x 257 pairs of samples, with what obstacle_inv_delta answers for that delta (0: no
    reciprocal — the host does not commit such a world, only the dividing form of obstacle_message is compared)"""
    inv = C.c_double(0.0)
    assert D.d_check_obstacle_delta(delta, C.byref(inv)) == 0
    if 1e-3 <= delta <= 1e3:
        assert inv.value == 1.0 / delta  # the worlds' deltas all take the short form
    assert D.d_check_obstacle(delta, 4, 20000) == 0  # whole functions, old against new


def test_interrobot_slopes(D):
    """h0, cl, ch against 1 - r / d_safe, -1 / d_safe / r, 1 / d_safe / r as written, and ch == -cl wherever cl is a number:
    10^7 random (d_safe, r), r == 0, infinite and NaN r, d_safe of every kind"""
    assert D.d_check_slopes(6, N, THREADS) == 0


def test_interrobot_functions_old_against_new(D):
    assert D.d_check_interrobot(7, 2_000_000, THREADS) == 0
