"""The grouped seeded scripts of tests/group_fuzz.py on the engine: three scripts over the mutator surface are the three groups of
ONE world, their schedules go as one per-group call a step (mixed at most steps: the scripts' segment counts are ragged), and at
every script's own compare points its group is compared — beliefs bit for bit, connections, message counts, the topology passes'
return values — with the oracle that ran that script alone.  What the scripts have to be is pinned on the CPU in
tests/test_group_fuzz_recipes.py."""
import pytest

import group_fuzz as G
from test_group_fuzz_recipes import WORLDS, oracle_runs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,K", WORLDS)
def test_three_scripts_in_one_world(seed, K):
    scripts, runs = oracle_runs(seed, K)
    held = [h for _, h in runs]
    world, compared = G.run_shared(seed, scripts, held)
    assert compared == sum(len(h) for h in held)
    calls, launches, sat_out = world.group_schedule_stats()
    print(f"[group fuzz {seed}, K = {K}] {compared} comparisons, {calls} mixed calls, {launches} launches, {sat_out} workgroups sat out")
    assert calls > 0
    assert 2 * calls >= len(scripts[0].ops), (calls, len(scripts[0].ops))   # (ragged at no fewer than half of the steps)
