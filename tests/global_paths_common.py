"""What the global-path tests share (tests/test_global_paths.py on the CPU oracle, tests/test_gpu_global_paths.py on the engine):
the mission scenario in which robots wait for a path and then follow it."""
import numpy as np

from magics_amd import scenarios as S

F32 = np.float32


def mission_scenario():
    """six robots on a circle of 10 m heading for the antipode, tracking their straight line, no fixed connections"""
    n, K = 6, 10
    sc = S.circle_scenario(n, K, circle_radius=10.0, n_internal=10, n_external=10)
    sc["ir"] = []
    sc["params"] = dict(sc["params"], enable_mask=sc["params"]["enable_mask"] | S.EN_TRK)
    for rb in sc["robots"]:
        rb["path"] = np.array([rb["pos"], rb["goal"]], dtype=F32)
    return sc, n, K


def mission_kwargs(sc, idle):
    return dict(waypoints=[[tuple(rb["goal"])] for rb in sc["robots"]], radii=[rb["radius"] for rb in sc["robots"]],
                t0=[rb["t0"] for rb in sc["robots"]], steps=sc["steps"], comms_radius=10.0, target_speed=sc["target_speed"], idle=idle)


def replanned_path(rb):
    mid = (rb["pos"] + rb["goal"]) / 2 + np.array([3.0, -2.0])
    return np.array([rb["pos"], mid, rb["goal"]], dtype=F32)
