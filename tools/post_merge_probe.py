"""Diagnostics: what merging back-to-back schedules into one post buys (mgx_set_post_merge).  20 and 200 back-to-back ticks of the
10 / 10 schedule at 1000 x 16 + inter-robot factors, one mgx_iterate each, between two mgx_synchronize: us per iteration (best of
the repetitions) and mgx_post_merge_stats of the timed blocks.  MGX_POST_MERGE / MGX_LIB in the environment choose what runs; a
library without the entry point (an older build named by MGX_LIB) prints no stats."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa
from magics_amd import World, scenarios as S
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
sc = S.grid_scenario(n, 16, interrobot=True)
w = World(sc["params"]); S.populate(w, sc)
steps = bytes(sc["steps"])
has_stats = hasattr(w._L, "mgx_post_merge_stats")
for _ in range(60): w.iterate(steps)
w.synchronize()
for ticks in (20, 200, 20, 200):
    best, merged = 1e9, None
    for _ in range(8):
        s0 = w.post_merge_stats() if has_stats else None
        l0 = w.linger_stats()
        w.synchronize(); t0 = time.perf_counter()
        for _ in range(ticks): w.iterate(steps)
        w.synchronize(); dt = (time.perf_counter() - t0) / (ticks * len(steps)) * 1e6
        if dt < best:
            s1, l1 = (w.post_merge_stats() if has_stats else None), w.linger_stats()
            best = dt
            merged = ([b - a for a, b in zip(s0[:2], s1[:2])] + [s1[2]] if has_stats else None, [b - a for a, b in zip(l0, l1)])
    per_plan = (merged[0][1] / max(merged[0][0], 1)) if has_stats else float("nan")
    print(os.environ.get("MGX_LIB", "product"), "post_merge", os.environ.get("MGX_POST_MERGE", "default"), f"{ticks} ticks back to back:",
          "us/iteration %.3f" % best, "| plans posted, schedules in them, largest ever:", merged[0], "schedules/plan %.2f" % per_plan,
          "| linger launches, posts, reruns, ended by device:", merged[1], flush=True)
