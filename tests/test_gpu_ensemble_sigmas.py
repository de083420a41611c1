"""Members of an Ensemble that differ in gbp.sigma-factor-tracking — the sigma sweep of the reference's Collaborative GP experiment
(scripts/run-collaborative-gp-experiment.fish: seeds x tracking off / on x sigma-factor-tracking 0.15 / 0.5) on a scenario that
needs no global planner — as ONE world (mgx_set_group_sigmas): every member against the same scenario run by a Simulation on a
world of its own, json.dumps(export) and json.dumps(metrics) EQUAL, no tolerance, on the pattern of
tests/test_gpu_ensemble_factors.py.  The scenario is Structured Junction Twoway brought within reach of a short run: every
formation spawns twice, 80 ticks.  Members are sigma-factor-tracking (the scenario's own, 0.15, 0.5) x seeds (0, 31) — the scenario's
own IS 0.15, so two members per seed hold the world's sigmas and agree, and the third differs.  Once as group plans and once with
masked_resident=True, against the same solo runs."""
import copy
import json

import pytest

from magics_amd import config, sim
from magics_amd.ensemble import SIGMAS, Ensemble
from test_gpu_ensemble_factors import SEEDS, TICKS, _dump, _scenario, _world

pytestmark = pytest.mark.gpu

SIGMA_TRACKING = (None, 0.15, 0.5)     # None: the scenario's own


def _member(seed, sigma):
    sc = _scenario(seed, 0.0, True)
    if sigma is not None:
        sc["config"]["gbp"]["sigma-factor-tracking"] = config.f32(sigma)   # (f32, as parse_config reads it)
    return sc


def _sigma_of(sc):
    return config.world_params(sc["config"])["sigma_tracking"]


KEYS = [(sigma, seed) for sigma in SIGMA_TRACKING for seed in SEEDS]


@pytest.fixture(scope="module")
def solos():
    """every member run by a Simulation on a world of its own, once: (export, metrics) as text"""
    out = {}
    for key in KEYS:
        sc = _member(key[1], key[0])
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc)).run(max_ticks=TICKS)
        assert len(solo.robots) > 2 and solo.tick_no == TICKS
        out[key] = (_dump(solo.export()), _dump(solo.metrics()))
    own = json.loads(out[(None, SEEDS[0])][0])
    assert own                                           # (something was exported)
    for seed in SEEDS:                                   # the same seed under two sigmas: two different runs
        assert out[(0.15, seed)][0] != out[(0.5, seed)][0], seed
        values = {_sigma_of(_member(seed, sigma)) for sigma in SIGMA_TRACKING}
        assert len({out[(sigma, seed)][0] for sigma in SIGMA_TRACKING}) == len(values) >= 2, seed
    return out


@pytest.mark.parametrize("masked_resident", [False, True], ids=["group-plans", "masked-resident"])
def test_sigma_tracking_sweep_as_one_world(solos, masked_resident):
    scs = [_member(seed, sigma) for sigma, seed in KEYS]
    own = _sigma_of(scs[0])
    assert own != config.f32(0.5), "some member differs from member 0"
    ens = Ensemble([copy.deepcopy(sc) for sc in scs], _world(scs[0]), masked_resident=masked_resident).run(max_ticks=TICKS)
    for m, (key, sc) in enumerate(zip(KEYS, scs)):
        p = config.world_params(sc["config"])
        assert ens.world.group_sigmas(m) == {k: p["sigma_" + k] for k in SIGMAS}, (m, key)
        assert ens.world.group_sigmas(m)["tracking"] == (own if key[0] is None else config.f32(key[0])), (m, key)
        assert ens.world.group_enabled(m) == config.enable_mask(sc["config"]), (m, key)      # (the kinds agree: no masks)
        assert ens.members[m].tick_no == TICKS, m
        assert _dump(ens.members[m].export()) == solos[key][0], (m, key)
        assert _dump(ens.members[m].metrics()) == solos[key][1], (m, key)
    plans, launches = ens.world.group_enabled_stats()
    res_launches, posts, fallbacks = ens.world.group_resident_stats()
    assert ens.world.group_schedule_stats() == (0, 0, 0)
    if masked_resident:
        assert res_launches > 0 and ens.world.resident_stats()[0] >= res_launches, (res_launches, posts, fallbacks)
        assert plans == fallbacks                          # what still ran as a group plan is counted as a fall-back
    else:
        assert plans > 0 and launches > plans              # the ticks ran as group plans, launch by launch
        assert (res_launches, posts, fallbacks) == (0, 0, 0) and ens.world.resident_stats()[0] == 0
