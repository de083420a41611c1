"""The masked form of the resident sweep kernel (SWEEP_F_GRP: mgx_set_group_resident) on EVERY horizon variant, against the CPU
oracle.

The form exists once per horizon — the ten constant ones and the two run-time-K kernels (mgx_sweep_inst.hip, MGX_FEAT 7) — and
reads its workgroup's enabled internal kinds from DevWorld::group_enable where the other resident forms read the kernel's scalar:
for the dynamic, obstacle and tracking guards and for obs_rows, the choice between four lanes per obstacle factor and one.  Every
cell is the four-group world of tests/test_gpu_groups_factors_kernel_matrix.py (12 robots, its masks: the world's W = dynamic |
obstacle | tracking | inter-robot, W without tracking, W without obstacle, W without dynamic; groups 0 and 1 the same robots)
against one oracle.OracleWorld per group, created with that group's mask.

Two rounds per cell, nothing read in between: one equal schedule — a resident launch — and one tick, whose prior changes ride in
the POST into the launch that lingers.  Which kernel ran and in which form is read back from the engine.

Two cells more on the open layout (where the tracking factors keep the oracle finite) with a schedule of ten internal and ten
external iterations, so that the tracking factors of the groups that have them act (they start at the tenth factor iteration)
beside a group that has none and a group without dynamic factors: at K = 12 and at K = 8, the run-time-K kernel."""
import numpy as np
import pytest

import oracle
from magics_amd import hostlib, scenarios as S
from test_gpu_groups_factors_kernel_matrix import group_masks
from test_gpu_groups_kernel_matrix import PER_GROUP, SEEDS, SPAWN_GROUP, OraclePair, group_scenario, group_schedules
from test_gpu_groups_schedules import Pair
from test_gpu_kernel_matrix import CONST_K, IR_STAGED, POSTED, RESIDENT

MASKED_FORM = 7   # MGX_SWEEP_F_GROUP_KINDS | MGX_SWEEP_F_TRACKING | MGX_SWEEP_F_UPDATES
HZ = 10.0


class ResidentOraclePair(OraclePair):
    """the masked four-group world with mgx_set_group_resident on, both before the first robot; the groups' oracles have their
    masks in their params"""

    def __init__(self, layout, K):
        scs, radius = [], None
        for seed in SEEDS:
            sc, radius = group_scenario(layout, K, PER_GROUP + 1, seed, True)
            assert sc["K"] == K
            scs.append(sc)
        self.masks = group_masks(scs[0]["params"]["enable_mask"])
        assert self.masks[0] & S.EN_TRK and self.masks[0] & S.EN_IR and len(set(self.masks)) == 4
        for sc, mask in zip(scs, self.masks):
            sc["params"] = dict(sc["params"], enable_mask=mask)
        self._pending = True
        Pair.__init__(self, scs=scs, sizes=[PER_GROUP] * len(SEEDS), radius=radius, spawn_group=SPAWN_GROUP, reserve=1,
                      alone=lambda params: oracle.OracleWorld(params, threads=1))
        self.shared.set_linger(1000000)   # (the post must find the launch there however slow the host is)
        self.shared.set_post_merge(0)

    def add(self, g, i):
        if self._pending:
            self._pending = False
            self.shared.set_group_resident(True)
            for q, mask in enumerate(self.masks):
                self.shared.set_group_enabled(self.gid[q], mask)
        super().add(g, i)


CELLS = [(f"K{K}", K, variant) for variant, K in {**{k: k for k in CONST_K}, -1: 34}.items()]


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,variant", CELLS, ids=[c[0] for c in CELLS])
def test_the_masked_form_on_every_horizon(name, K, variant):
    sch = group_schedules()
    p = ResidentOraclePair("near", K)
    w = p.shared
    assert [w.group_enabled(g) for g in range(4)] == list(p.masks)
    p.topology()
    assert p.created > 0 and sum(len(x) for x in p.ids) == 12
    _launch_then_post(p, name, variant, sch[1], sch[0])


def _launch_then_post(p, name, variant, first, second):
    """round 1: one schedule for all — a resident launch of the masked form; round 2 right behind it: a tick — its prior changes
    ride in the post.  The oracles run the same two rounds, and every group has to equal its own."""
    w = p.shared
    w.iterate([first] * 4)
    ran = w.last_launch_count(), w.last_sweep()[:3], w.last_sweep_features()
    by_id = {p.ids[g][i]: rb for g in range(p.n) for i, rb in enumerate(p.robots(g))}
    every = {"robots": [by_id[r] for r in sorted(by_id)], "target_speed": p.scs[0]["target_speed"]}
    w.tick(steps=second, **dict(S.tick_inputs(every, HZ), robots=np.array(sorted(by_id), dtype=np.int32)))
    posted = w.last_launch_count(), w.last_sweep()[:3], w.last_sweep_features()
    assert ran == (1, (variant, IR_STAGED, RESIDENT), MASKED_FORM), (name, "ran", ran)
    assert posted == (1, (variant, IR_STAGED, POSTED), MASKED_FORM), (name, "posted", posted)
    assert w.group_resident_stats() == (1, 1, 0) and w.group_enabled_stats() == (0, 0), name
    w.flush()
    for g, solo in enumerate(p.alone):
        solo.iterate(first)
        solo.tick(steps=second, **S.tick_inputs({"robots": p.robots(g), "target_speed": p.scs[g]["target_speed"]}, HZ))
    p.finite(name)
    p.same(name)
    assert not np.array_equal(p.beliefs()[2][p.ids[0]], p.beliefs()[2][p.ids[1]]), (name, "the same robots, tracking on and off")
    assert w.linger_stats()[2] == 0, (name, "the post was taken, not taken back")


@pytest.mark.gpu
@pytest.mark.parametrize("K,variant", [(12, 12), (8, 0)], ids=["K12", "K8"])
def test_tracking_factors_act_beside_groups_without(K, variant):
    """a group with tracking factors, one without, one without dynamic factors, past the tenth factor iteration"""
    p = ResidentOraclePair("open", K)
    assert p.masks[0] & S.EN_TRK and not p.masks[1] & S.EN_TRK and not p.masks[3] & S.EN_DYN
    p.topology()
    assert p.created > 0 and sum(len(x) for x in p.ids) == 12
    long = hostlib.schedule(hostlib.SCHEDULE_INTERLEAVE_EVENLY, 10, 10)
    assert sum(1 for s in long if s & hostlib.STEP_INTERNAL) + sum(1 for s in long if s & hostlib.STEP_EXTERNAL) == 20   # factor iterations: past ten in round 1
    _launch_then_post(p, f"K{K}-tracking", variant, long, long)


def test_the_cells_are_the_masked_instantiations():
    """static: every horizon of the three sets (mgx_sweep_inst.hip), the run-time-K kernels included, has a cell"""
    import re
    from test_gpu_kernel_matrix import INST
    src = open(INST).read()
    variants = []
    for m in re.finditer(r"#define MGX_K_LIST\(DO\)(.*)", src):
        variants += [int(v) for v in re.findall(r"DO\((-?\d+)\)", m.group(1))]
    assert sorted(variants) == sorted(list(CONST_K) + [0, -1])
    assert {v for _, _, v in CELLS} | {0} == set(variants)            # (variant 0: the K = 8 cell above, and tests/test_gpu_groups_factors_resident.py)
    assert all(v == (K if K in CONST_K else -1) and (K in CONST_K or K >= 34) for _, K, v in CELLS)
    assert "MGX_FEAT == 3 || MGX_FEAT == 7" in src                    # the masked form is built for the whole list, like the full one
