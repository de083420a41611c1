"""The Ensemble of tests/test_gpu_ensemble_factors.py — Structured Junction Twoway, tracking on and off x failure rates x seeds, 8
members, 80 ticks — with masked_resident=True: the masked world's ticks run as resident launches of the masked form
(mgx_set_group_resident) instead of group plans, and every member still equals the same scenario run by a Simulation on a world of
its own: json.dumps(export) and json.dumps(metrics) EQUAL, no tolerance.  Plain, and with the device's environment-collision pass
and run metrics switched on.  The same ensemble with the switch off, run here, says what the switch saved."""
import copy

import pytest

from magics_amd import config, sim
from magics_amd.ensemble import Ensemble
from test_gpu_ensemble_factors import RATES, SEEDS, TICKS, _dump, _scenario, _world

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("options", [{}, {"environment_collisions": True, "device_metrics": True}], ids=["plain", "observers"])
def test_tracking_on_and_off_as_one_world_with_resident_launches(options):
    keys = [(tracking, rate, seed) for tracking in (True, False) for rate in RATES for seed in SEEDS]
    scs = [_scenario(seed, rate, tracking) for tracking, rate, seed in keys]
    ens = Ensemble([copy.deepcopy(sc) for sc in scs], _world(scs[0]), masked_resident=True, **options).run(max_ticks=TICKS)
    assert [ens.world.group_enabled(m) for m in range(len(scs))] == [config.enable_mask(sc["config"]) for sc in scs]
    assert len(set(ens.world.group_enabled(m) for m in range(len(scs)))) == 2           # a masked world
    for m, (key, sc) in enumerate(zip(keys, scs)):
        solo = sim.Simulation(copy.deepcopy(sc), _world(sc), **options).run(max_ticks=TICKS)
        assert len(solo.robots) > 2
        assert ens.members[m].tick_no == solo.tick_no == TICKS, m
        assert _dump(ens.members[m].export()) == _dump(solo.export()), (m, key)
        assert _dump(ens.members[m].metrics()) == _dump(solo.metrics()), (m, key)
    launches, posts, fallbacks = ens.world.group_resident_stats()
    assert launches + posts > 0, (launches, posts, fallbacks)
    assert ens.world.resident_stats()[0] >= launches > 0
    off = Ensemble([copy.deepcopy(sc) for sc in scs], _world(scs[0]), **options).run(max_ticks=TICKS)
    assert off.world.group_resident_stats() == (0, 0, 0) and off.world.resident_stats()[0] == 0
    assert ens.world.group_enabled_stats()[1] < off.world.group_enabled_stats()[1], (ens.world.group_enabled_stats(), off.world.group_enabled_stats())
    assert ens.world.group_enabled_stats()[0] == fallbacks                                # what still ran as a group plan is counted as a fall-back
    for a, b in zip(ens.members, off.members):                                            # ... and changed nothing
        assert _dump(a.export()) == _dump(b.export())
