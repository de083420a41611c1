"""Factor sigmas per robot group (mgx_set_group_sigmas) on EVERY launch-per-segment instantiation of the sweep kernel and on the
masked resident form of every horizon, against the CPU oracle.

A world in which some group has sigmas of its own is run as a masked world is: every schedule goes through run_group_plan
(mgx_world_launch.inc) and every !PERSIST instantiation of k_robot_sweep reads its group's {1 / sigma_obstacle^2,
1 / sigma_interrobot^2, 1 / sigma_tracking^2} from DevWorld::group_sigma beside the group's segment record (mgx_sweep.h), in place
of the launch-wide scalars; with mgx_set_group_resident the masked form (SWEEP_F_GRP) reads them once per workgroup.
sigma_dynamics is in the dyn_m of the group's robots.  The twelve horizon variants x {no, staged, unstaged} inter-robot messages
are the cells of tests/test_gpu_groups_factors_kernel_matrix.py (layouts none / near / dense, tracking paths), the resident cells
those of tests/test_gpu_groups_factors_resident_matrix.py and the run-time-K kernel at K = 8: one shared World of four groups
against one oracle.OracleWorld per group, created with that group's sigmas.

The groups (the world's sigmas are 0.1 / 0.01 / 0.01 / 0.01): the world's; tracking 0.15 — the same robots as group 0; obstacle
0.05 and inter-robot 0.05; dynamics 0.05 and tracking 0.5.  Groups 0 and 1 run the same schedules throughout, so that they end
with different beliefs is what group 1's sigma does (the tracking factors start at the tenth factor iteration: in the second
round).

Segment cells, two rounds: a MIXED call (groups 0 and 1 alike), then an EQUAL schedule — a group plan as well, counted by
mgx_group_enabled_stats.  Resident cells: an equal schedule — one resident launch of the masked form — and a tick posted into it.
Which kernel ran is read back from the engine.  Finiteness of every oracle is asserted as a condition on the inputs."""
import numpy as np
import pytest

import oracle
from magics_amd import scenarios as S
from test_gpu_groups_factors_resident_matrix import MASKED_FORM, _launch_then_post
from test_gpu_groups_kernel_matrix import PER_GROUP, SEEDS, SPAWN_GROUP, OraclePair, group_scenario, group_schedules
from test_gpu_groups_schedules import Pair, segments
from test_gpu_kernel_matrix import CONST_K, FORM_K, FORMS, IR_NONE, SEGMENTS, _crowd

LAYOUT = {"seg_none": "none", "seg_staged": "near", "seg_global": "dense"}
NAMES = ("dynamics", "interrobot", "obstacle", "tracking")
OWN = ({}, {"tracking": 0.15}, {"obstacle": 0.05, "interrobot": 0.05}, {"dynamics": 0.05, "tracking": 0.5})


def cell_scenarios(layout, K, crowd=0):
    """OraclePair's scenarios with tracking paths, each with its group's sigmas in its params: (scs, sizes, radius, sigmas)"""
    sizes, scs, radius = [PER_GROUP] * len(SEEDS), [], None
    for g, seed in enumerate(SEEDS):
        if g == 0 and crowd:   # group 0 is the dense crowd: the world-wide inter-robot mode follows the most crowded robot
            sc, radius = group_scenario("dense", K, crowd, seed, True)
            sizes[0] = crowd
        else:
            sc, r = group_scenario(layout, K, sizes[g] + 1, seed, True)
            radius = radius if crowd else r
        assert sc["K"] == K
        scs.append(sc)
    world = {k: scs[0]["params"]["sigma_" + k] for k in NAMES}
    sigmas = [dict(world, **{k: S.f32w(v) for k, v in own.items()}) for own in OWN]
    assert sigmas[0] == world and len({tuple(sorted(s.items())) for s in sigmas}) == 4
    for sc, s in zip(scs, sigmas):
        assert sc["params"]["enable_mask"] & S.EN_TRK
        sc["params"] = dict(sc["params"], **{"sigma_" + k: v for k, v in s.items()})
    return scs, sizes, radius, sigmas


class SigmaOraclePair(OraclePair):
    """OraclePair whose groups have sigmas of their own: set on the shared world before the first robot goes in, in the params of
    the groups' oracles.  resident: mgx_set_group_resident before the first robot as well"""

    def __init__(self, layout, K, crowd=0, resident=False):
        scs, sizes, radius, self.sigmas = cell_scenarios(layout, K, crowd)
        self.masks = (scs[0]["params"]["enable_mask"],) * len(scs)
        self._pending, self._resident = True, resident
        Pair.__init__(self, scs=scs, sizes=sizes, radius=radius, spawn_group=SPAWN_GROUP, reserve=1,
                      alone=lambda params: oracle.OracleWorld(params, threads=8 if crowd and params is scs[0]["params"] else 1))
        if resident:
            self.shared.set_linger(1000000)   # (the post must find the launch there however slow the host is)
            self.shared.set_post_merge(0)

    def add(self, g, i):
        if self._pending:
            self._pending = False
            if self._resident:
                self.shared.set_group_resident(True)
            for q, s in enumerate(self.sigmas):
                self.shared.set_group_sigmas(self.gid[q], **s)
        super().add(g, i)


CELLS = [(f"K{K}-{form}", K, variant, form) for variant, K in FORM_K.items() for form in ("seg_none", "seg_staged", "seg_global")]
RESIDENT_CELLS = [(f"K{K}", K, variant) for variant, K in {**{k: k for k in CONST_K}, -1: 34, 0: 8}.items()]


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,variant,form", CELLS, ids=[c[0] for c in CELLS])
def test_group_sigmas_on_every_instantiation(name, K, variant, form):
    sch = group_schedules()
    ir_mode, sweep_form = FORMS[form]
    want = (variant, ir_mode, sweep_form)
    p = SigmaOraclePair(LAYOUT[form], K, crowd=_crowd(K) if form == "seg_global" else 0)
    assert [p.shared.group_sigmas(g) for g in range(4)] == p.sigmas
    if ir_mode == IR_NONE:
        assert not p.masks[0] & S.EN_IR
    else:
        p.topology()
        assert p.created > 0
    # round 1: a mixed call, groups 0 and 1 under the same schedule, every group under its own sigmas
    most, sat = p.mixed([sch[0], sch[0], sch[2], sch[3]], (name, "mixed"), want)
    assert p.shared.group_schedule_stats() == (1, most, sat) and p.shared.group_enabled_stats() == (0, 0)
    # round 2: one schedule for all — on such a world a group plan in which every group has the same segments
    p.iterate([sch[1]] * 4)
    n = len(segments(sch[1]))
    assert p.shared.last_launch_count() == n and p.shared.last_sweep()[:3] == want, (name, p.shared.last_sweep())
    assert p.shared.group_enabled_stats() == (1, n) and p.shared.group_schedule_stats() == (1, most, sat)
    assert p.shared.resident_stats()[0] == 0
    p.finite((name, "equal"))
    p.same((name, "equal"))
    if p.sizes[0] == p.sizes[1]:   # the same robots, the same schedules: sigma_tracking 0.01 and 0.15
        assert not np.array_equal(p.beliefs()[2][p.ids[0]], p.beliefs()[2][p.ids[1]]), (name, "group 1's sigma makes no difference")


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,variant", RESIDENT_CELLS, ids=[c[0] for c in RESIDENT_CELLS])
def test_group_sigmas_on_the_masked_form_of_every_horizon(name, K, variant):
    sch = group_schedules()
    p = SigmaOraclePair("near", K, resident=True)
    assert [p.shared.group_sigmas(g) for g in range(4)] == p.sigmas
    p.topology()
    assert p.created > 0 and sum(len(x) for x in p.ids) == 12
    # (an equal schedule: a resident launch of the masked form; a tick right behind it: a post; groups 0 and 1 have to differ)
    _launch_then_post(p, name, variant, sch[1], sch[0])
    assert p.shared.last_sweep_features() == MASKED_FORM


def test_the_cells_are_the_segment_kernels_and_the_masked_forms():
    assert len(CELLS) == 36 and len({c[0] for c in CELLS}) == 36
    assert {(v, *FORMS[f]) for _, _, v, f in CELLS} == {(v, ir, SEGMENTS) for v in FORM_K for ir in (0, 1, 2)}
    assert any(4 * (K - 2) <= 64 for _, K, _, _ in CELLS) and any(K >= 34 for _, K, _, _ in CELLS)
    assert len(RESIDENT_CELLS) == 12 and {v for _, _, v in RESIDENT_CELLS} == set(FORM_K)
    assert all(v == (K if K in CONST_K else (0 if 2 * (K - 1) <= 64 else -1)) for _, K, v in RESIDENT_CELLS)
    assert len({tuple(sorted(o.items())) for o in OWN}) == 4 and OWN[0] == {} and OWN[1] != OWN[0]
