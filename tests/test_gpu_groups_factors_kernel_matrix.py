"""Enabled factor kinds per robot group (mgx_set_group_enabled) on EVERY launch-per-segment instantiation of the sweep kernel,
against the CPU oracle.

On a masked world every schedule runs through run_group_plan (mgx_world_launch.inc), and every !PERSIST instantiation of
k_robot_sweep reads its group's kinds from DevWorld::group_enable beside the group's segment record (mgx_sweep.h) — where it read
the kernel's scalar for the dynamic, obstacle and tracking guards and for obs_rows, the choice between four lanes per obstacle
factor and one.  The twelve horizon variants x {no, unstaged, staged} inter-robot messages are the cells of
tests/test_gpu_groups_kernel_matrix.py, whose OraclePair and vocabulary this file uses: one shared World of four groups against
one oracle.OracleWorld per group, created with that group's mask.

Every cell's world has tracking paths and mask W = dynamic | obstacle | tracking (| inter-robot); the groups run under W, W without
tracking, W without obstacle, W without dynamic.  So groups with tracking on (obstacle factors one lane each, tracking lanes
beside them) and group 1 with tracking off (four lanes per obstacle factor where 4 (K - 2) <= 64) run in the same launch, and at
K >= 34 the second tracking lane of the wide kernels runs beside workgroups that have none.  Groups 0 and 1 hold the same robots.

Two rounds per cell: the four MIXED schedules, then an EQUAL schedule — which a masked world runs as a group plan too, never
resident (mgx_group_enabled_stats counts it).  Which kernel ran is read back from the engine (last_sweep)."""
import numpy as np
import pytest

import oracle
from magics_amd import scenarios as S
from test_gpu_groups_kernel_matrix import PER_GROUP, SEEDS, SPAWN_GROUP, OraclePair, group_scenario, group_schedules
from test_gpu_groups_schedules import Pair, segments
from test_gpu_kernel_matrix import FORM_K, FORMS, IR_NONE, SEGMENTS, _crowd

LAYOUT = {"seg_none": "none", "seg_staged": "near", "seg_global": "dense"}


def group_masks(world_mask):
    """the world's, without tracking, without obstacle, without dynamic"""
    return (world_mask, world_mask & ~S.EN_TRK, world_mask & ~S.EN_OBS, world_mask & ~S.EN_DYN)


def cell_scenarios(layout, K, crowd=0):
    """OraclePair's scenarios with tracking paths, each with its group's mask in its params: (scs, sizes, radius, masks)"""
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
    masks = group_masks(scs[0]["params"]["enable_mask"])
    assert masks[0] & S.EN_TRK and len(set(masks)) == 4
    for sc, mask in zip(scs, masks):
        sc["params"] = dict(sc["params"], enable_mask=mask)
    return scs, sizes, radius, masks


class MaskedOraclePair(OraclePair):
    """OraclePair whose groups have masks of their own: set on the shared world before the first robot goes in, in the params of
    the groups' oracles"""

    def __init__(self, layout, K, crowd=0):
        scs, sizes, radius, self.masks = cell_scenarios(layout, K, crowd)
        self._masks_pending = True
        Pair.__init__(self, scs=scs, sizes=sizes, radius=radius, spawn_group=SPAWN_GROUP, reserve=1,
                      alone=lambda params: oracle.OracleWorld(params, threads=8 if crowd and params is scs[0]["params"] else 1))

    def add(self, g, i):
        if self._masks_pending:
            self._masks_pending = False
            for q, mask in enumerate(self.masks):
                self.shared.set_group_enabled(self.gid[q], mask)
        super().add(g, i)


CELLS = [(f"K{K}-{form}", K, variant, form) for variant, K in FORM_K.items() for form in ("seg_none", "seg_staged", "seg_global")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,variant,form", CELLS, ids=[c[0] for c in CELLS])
def test_group_kinds_on_every_instantiation(name, K, variant, form):
    sch = group_schedules()
    ir_mode, sweep_form = FORMS[form]
    want = (variant, ir_mode, sweep_form)
    p = MaskedOraclePair(LAYOUT[form], K, crowd=_crowd(K) if form == "seg_global" else 0)
    assert [p.shared.group_enabled(g) for g in range(4)] == list(p.masks)
    if ir_mode == IR_NONE:
        assert not p.masks[0] & S.EN_IR
    else:
        p.topology()
        assert p.created > 0
    # round 1: the four mixed schedules, every group under its own kinds
    most, sat = p.mixed(sch, (name, "mixed"), want)
    assert p.shared.group_schedule_stats() == (1, most, sat) and p.shared.group_enabled_stats() == (0, 0)
    if p.sizes[0] == p.sizes[1]:   # the same robots, tracking on and off
        assert not np.array_equal(p.beliefs()[2][p.ids[0]], p.beliefs()[2][p.ids[1]])
    # round 2: one schedule for all — on a masked world a group plan in which every group has the same segments
    p.iterate([sch[1]] * 4)
    n = len(segments(sch[1]))
    assert p.shared.last_launch_count() == n and p.shared.last_sweep()[:3] == want, (name, p.shared.last_sweep())
    assert p.shared.group_enabled_stats() == (1, n) and p.shared.group_schedule_stats() == (1, most, sat)
    assert p.shared.resident_stats()[0] == 0
    p.finite((name, "equal"))
    p.same((name, "equal"))


def test_the_cells_are_the_thirty_six_segment_kernels():
    assert len(CELLS) == 36 and len({c[0] for c in CELLS}) == 36
    assert {(v, *FORMS[f]) for _, _, v, f in CELLS} == {(v, ir, SEGMENTS) for v in FORM_K for ir in (0, 1, 2)}
    assert any(4 * (K - 2) <= 64 for _, K, _, _ in CELLS) and any(K >= 34 for _, K, _, _ in CELLS)
