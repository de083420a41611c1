"""What the tests of missions of several legs share (tests/test_mission_legs_cpu.py on the CPU oracle,
tests/test_gpu_mission_legs.py on the engine): the scenario, the script of paths handed in when a leg ends, and one run of it.

    robot 0   two legs     (-15, -4) -> (-4, -4) -> (4, -4)              paths handed in: axis-aligned
    robot 1   three legs   (12, 6) -> (5, 3) -> (-1, 7) -> (-8, 4)       paths handed in: oblique
    robot 2   no legs      (12, -14) -> (6, -12) -> (0, -14)             a plain route of two waypoints
    (within each other's comms radius most of the time, and never in each other's way)
    pair=True adds robots 3 and 4, mirror images of each other in the x axis and out of everybody's comms radius: 3 has one
    leg left when it reaches (68, 30), 4 completes at (68, -30) — in the same tick, being mirror images."""
import numpy as np

from magics_amd import scenarios as S

F32 = np.float32
K = 10
COMMS_RADIUS = 15.0
PLANNING_HORIZON = 3.0
# per robot: the taskpoints of its legs (robot 2: its plain route) and how many legs follow the first
TASKPOINTS = [[(-15.0, -4.0), (-4.0, -4.0), (4.0, -4.0)],
              [(12.0, 6.0), (5.0, 3.0), (-1.0, 7.0), (-8.0, 4.0)],
              [(12.0, -14.0), (6.0, -12.0), (0.0, -14.0)],
              [(60.0, 30.0), (68.0, 30.0), (76.0, 30.0)],
              [(60.0, -30.0), (68.0, -30.0)]]
LEGS = [1, 2, 0, 1, 0]
# ticks a robot waits between the end of leg k and the hand-over of leg k + 1 (0: before the very next tick)
WAIT = {(0, 1): 0, (1, 1): 3, (1, 2): 0, (3, 1): 2}


def legs_scenario(pair=False):
    n = 5 if pair else 3
    sc = S.circle_scenario(n, K, circle_radius=50.0, n_internal=10, n_external=10)
    sc["ir"] = []
    sc["params"] = dict(sc["params"], enable_mask=sc["params"]["enable_mask"] | S.EN_TRK)
    ts = S.timesteps_for_K(K)
    speed = sc["target_speed"]
    for r, rb in enumerate(sc["robots"]):
        tp = TASKPOINTS[r]
        if r == 4:
            rb["radius"] = sc["robots"][3]["radius"]  # the mirror image
        d = np.array(tp[1]) - np.array(tp[0])
        v = speed * d / np.hypot(*d)
        start, goal = (*tp[0], *v), (*tp[1], *v)
        rb["mean0"], rb["prior_diag"], rb["dt"] = S.robot_initial_state(start, goal, ts, rb["radius"], speed, PLANNING_HORIZON)
        rb["pos"], rb["goal"] = np.array(tp[0]), np.array(tp[1])
        rb["t0"] = F32(rb["radius"]) / F32(2.0) / F32(speed)
        rb["path"] = np.array(tp[:2] if LEGS[r] else tp, dtype=F32)
    sc["positions"] = np.array([rb["pos"] for rb in sc["robots"]])
    return sc, n


def driver_kwargs(sc, n, legs=True, **more):
    """the arguments of Driver / DeviceDriver: the first route of every robot, and the legs that follow it (legs: True — LEGS; a
    list — that; False / None — the argument is left out)"""
    kw = dict(waypoints=[TASKPOINTS[r][1:2] if LEGS[r] else TASKPOINTS[r][1:] for r in range(n)], radii=[rb["radius"] for rb in sc["robots"]],
              t0=[rb["t0"] for rb in sc["robots"]], steps=sc["steps"], comms_radius=COMMS_RADIUS, target_speed=sc["target_speed"], **more)
    if legs is True:
        kw["legs"] = LEGS[:n]
    elif legs not in (False, None):
        kw["legs"] = list(legs)
    return kw


def leg_path(robot, leg):
    """the path the test hands in for leg `leg` (1 ..) of `robot`: from taskpoint `leg` to taskpoint `leg + 1` through a point
    off their line (robot 0 and the pair: on it — axis-aligned)"""
    a, b = np.array(TASKPOINTS[robot][leg]), np.array(TASKPOINTS[robot][leg + 1])
    mid = (a + b) / 2 + (np.array([0.75, -0.5]) if robot == 1 else 0.0)
    return np.array([a, mid, b], dtype=F32)


class Script:
    """who gets which path before which tick: robots that ended leg k - 1 in tick t are handed leg k before tick t + 1 + WAIT"""

    def __init__(self):
        self.leg = {}        # robot -> legs it has ended
        self.due = {}        # tick -> [(robot, leg)]
        self.handed = []     # (tick, robot, leg) in the order they were handed in

    def ended(self, tick, robots):
        for r in robots:
            k = self.leg[r] = self.leg.get(r, 0) + 1
            self.due.setdefault(tick + 1 + WAIT[(r, k)], []).append((r, k))

    def hand_over(self, tick, *drivers):
        for r, k in self.due.pop(tick, []):
            for d in drivers:
                d.global_path(r, leg_path(r, k), PLANNING_HORIZON)
            self.handed.append((tick, r, k))
