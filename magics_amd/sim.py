"""Headless run of a reference scenario directory (config.toml + environment.yaml + formation.yaml,
unmodified) on a World-like backend — the HIP engine (`magics_amd.World`) in the product, the CPU
oracle in the tests.  One `tick()` is one FixedUpdate of the reference at `simulation.hz`, preceded
by the frame's Update systems that matter to the path (the formation spawners):

    advance_time + spawn_formation          crates/magics/src/planner/spawner.rs:386-649   (Update)
    reached_waypoint                        planner/robot.rs:2080-2176                     \\
    update_robot_neighbours / delete_ / create_interrobot_factors   robot.rs:1362-1586      |
    update_failed_comms                     robot.rs:1593-1601                               > FixedUpdate
    update_prior_of_horizon_state / update_prior_of_current_state_v3   robot.rs:2182-2338   |
    iterate_gbp_v2                          robot.rs:1769-1861                              /
    export                                  crates/magics/src/export.rs:249-262,283-620

The reference runs its Update systems at the display's frame rate against virtual time, so the
interleaving of spawns with fixed ticks is not reproducible there; here a frame is exactly one
fixed tick long.  Rendering and picking are outside the path (SURVEY §8 out of scope); goal areas (goal_area.rs:67-103) are
recorded on request (`goal_areas=`: the reference spawns none, the caller hands them in); RRT* planning
(`planning-strategy: rrt-star`) is rejected unless a global planner is asked for (`global_planner=`: the engine's, or its host
restatement, magics_amd/global_planner.py).  Robot-environment collisions (planner/collisions.rs:368-438) are counted on request
(`environment_collisions=True`) against the map's colliders (hostlib.env_colliders) with the contact include/mgx.h
specifies: parry2d's own shape queries are third party and absent, so contacts within rounding of tangency are not pinned.
"""
import json

import numpy as np

from . import config as _config
from . import environment as _environment
from . import hostlib, spawner
from . import track_metrics as _metrics
from .prng import WyRand
from .scenarios import robot_initial_state

F = np.float32


def environment_contacts(colliders, vertices, pos, rad):
    """The contact of include/mgx.h ("specification of a contact") in numpy f32, every operation rounded on its own: [n, m] bool,
    robot i (pos [n, 2] = Transform (x, z), rad [n]) touches collider j of hostlib.env_colliders.  The checker of the device pass
    (mgx_collisions.hip, env_touches)."""
    pos, rad = np.ascontiguousarray(pos, dtype=F).reshape(-1, 2), np.ascontiguousarray(rad, dtype=F).reshape(-1)
    out = np.zeros((len(pos), len(colliders)), dtype=bool)
    x, z, r = pos[:, 0:1], pos[:, 1:2], rad[:, None]
    with np.errstate(all="ignore"):
        b = np.nonzero(colliders["kind"] == hostlib.COLLIDER_BALL)[0]
        if len(b):
            dx, dz, rs = x - colliders["tx"][b][None], z - colliders["tz"][b][None], r + colliders["radius"][b][None]
            out[:, b] = dx * dx + dz * dz <= rs * rs
        c = np.nonzero(colliders["kind"] == hostlib.COLLIDER_CUBOID)[0]
        if len(c):
            h = colliders["half_extents"][c]
            ex = np.maximum(np.abs(x - colliders["tx"][c][None]) - h[None, :, 0], F(0))
            ez = np.maximum(np.abs(z - colliders["tz"][c][None]) - h[None, :, 1], F(0))
            out[:, c] = ex * ex + ez * ez <= r * r
        for j in np.nonzero(colliders["kind"] == hostlib.COLLIDER_POLYGON)[0]:
            nv = int(colliders["n_vertices"][j])
            if nv == 0:
                continue
            a = vertices[int(colliders["first_vertex"][j]):int(colliders["first_vertex"][j]) + nv].astype(F)
            e = np.roll(a, -1, axis=0) - a                                      # edge i: v_i -> v_(i+1)
            q = pos[:, None, :] - a[None]
            inside = (e[None, :, 0] * q[..., 1] - e[None, :, 1] * q[..., 0] >= 0).all(axis=1) & (nv >= 3) & (rad == rad)
            len2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])[None]
            t = np.where(len2 == 0, F(0), (q[..., 0] * e[None, :, 0] + q[..., 1] * e[None, :, 1]) / len2).astype(F)
            t = np.minimum(np.maximum(t, F(0)), F(1))
            d0, d1 = q[..., 0] - t * e[None, :, 0], q[..., 1] - t * e[None, :, 1]
            d2 = d0 * d0 + d1 * d1
            bad = np.isnan(t).any(axis=1) | np.isnan(d2).any(axis=1)
            out[:, j] = (inside | (d2.min(axis=1) <= rad * rad)) & ~bad
    return out


# setup_goal_areas_for_junction_scenario (goal_area.rs:105-119; commented out of the reference's plugin): the two exits of the
# junction.  The first box is written with its second coordinates swapped, as there
JUNCTION_GOAL_AREAS = (((-8.0, -48.0), (8.0, -52.0)), ((48.0, -8.0), (52.0, 8.0)))


def goal_area_boxes(areas):
    """boxes ((x0, z0), (x1, z1)) -> (mins [m, 2], maxs [m, 2]) in f32 with the corners sorted per axis (include/mgx.h, AREA)"""
    a = np.asarray(areas, dtype=F).reshape(-1, 2, 2)
    return np.minimum(a[:, 0], a[:, 1]), np.maximum(a[:, 0], a[:, 1])


def goal_area_contacts(areas, pos, rad):
    """The contact of a goal area (include/mgx.h, "goal areas": the cuboid line of the specification of a contact with the box's
    centre and half extents) in numpy f32, every operation rounded on its own: [n, m] bool, robot i (pos [n, 2] = Transform
    (x, z), rad [n]) touches box j of `areas` (((x0, z0), (x1, z1)), corners in either order).  A NaN anywhere: no contact.  The
    checker of the device pass (mgx_goal_areas.hip)."""
    pos, rad = np.ascontiguousarray(pos, dtype=F).reshape(-1, 2), np.ascontiguousarray(rad, dtype=F).reshape(-1)
    lo, hi = goal_area_boxes(areas)
    with np.errstate(all="ignore"):
        c, h = (lo + hi) * F(0.5), (hi - lo) * F(0.5)
        dx = np.abs(pos[:, 0:1] - c[None, :, 0]) - h[None, :, 0]
        dz = np.abs(pos[:, 1:2] - c[None, :, 1]) - h[None, :, 1]
        ex, ez = np.maximum(dx, F(0)), np.maximum(dz, F(0))          # (np.maximum keeps a NaN: the comparison below is then false)
        return ex * ex + ez * ez <= (rad * rad)[:, None]


def goal_flow(export, window=50.0):
    """The throughput scripts/analyse-junction-scenario.py:52-109 reads out of an export: the robots that started before
    `window` seconds and are in some goal area's history, per second of the window — written as there, 1 / (window / n), and
    0.0 where that divides by zero (n == 0)."""
    reached = set()
    for area in export["goal_areas"].values():
        reached.update(area["history"].keys())
    n = sum(1 for rid, r in export["robots"].items() if not r["mission"]["started_at"] >= window and rid in reached)
    return 1 / (window / n) if n else 0.0


def _box(lo, hi):
    return {"mins": [float(lo[0]), float(lo[1])], "maxs": [float(hi[0]), float(hi[1])]}


def _edges(table, now, aabb):
    """one step of the Free / Colliding state machine (CollisionHistory, collisions.rs:455-495) over table: key -> {"colliding",
    "times", "aabbs"}.  now: key -> whatever aabb(key, value) needs to give (mins, maxs) of a contact that begins."""
    for key, h in table.items():                                    # Colliding -> Free (also: a robot is gone)
        if h["colliding"] and key not in now:
            h["colliding"] = False
    for key, what in now.items():                                   # Free -> Colliding: one collision, with its AABB
        h = table.setdefault(key, {"colliding": False, "times": 0, "aabbs": []})
        if not h["colliding"]:
            h["colliding"] = True
            h["times"] += 1
            h["aabbs"].append(_box(*aabb(key, what)))


def _take_in(table, read, a, b, what):
    """the new events of a device log (World.collisions_read / env_collisions_read from the cursor on) into table; the new cursor"""
    ev, total, dropped = read[:3]
    if dropped:
        raise hostlib.MgxError(f"the device's {what} log was full: {dropped} events were not stored")
    for e in ev:
        h = table.setdefault((int(e[a]), int(e[b])), {"colliding": True, "times": 0, "aabbs": []})
        h["times"] += 1
        h["aabbs"].append(_box(e["mins"], e["maxs"]))
    return total


class Simulation:
    def __init__(self, scenario, world, neighbours_method=hostlib.NEIGHBOURS_AUTO, device_missions=None, device_collisions=None,
                 environment_collisions=False, global_planner=None, planner_overrides=None, plan_budget=64, device_trackers=None,
                 device_metrics=False, sample_log=True, goal_areas=None, device_goal_areas=None):
        """scenario: `config.load_scenario(dir)` (or a dict of the same shape); world: a fresh
        World-like object created with `config.world_params(scenario["config"])`.
        device_missions (default: whenever the world offers them, i.e. the engine): routes, reached-when rules and
        Transforms live on the device (include/mgx.h, mgx_mission_*) and a tick is two calls around the comms draws with
        ONE synchronisation and no belief read-back; otherwise this loop does all of it on the host (the CPU oracle's
        path, and the checker of the other one: tests/test_gpu_sim.py).
        device_collisions (default: whenever the missions live on the device and the world offers collisions_enable): the
        robot-robot collision pass runs on the device at the end of every tick (mgx_collisions_*) and `collisions` is filled
        from its event log when somebody asks; otherwise _collide below runs on the host every tick (the checker).
        environment_collisions (default off: the export keeps 0 / []): True — robot-environment collisions are counted, on the
        device (mgx_env_collisions_*) whenever the missions live there, otherwise by _collide_environment on the host; "host" —
        the host pass whatever the missions do (the checker of the device pass).
        device_trackers (default: whenever the missions live on the device and the world offers tracks_enable): the position /
        velocity samples and the distance travelled are made on the device at the end of every tick (mgx_tracks_*) and taken
        into the robots' `positions` / `velocities` / `travelled` when somebody asks; no tick then brings Transforms to the
        host unless a host collision pass needs them.  False: _track / _tracks below on the host (the checker).
        device_metrics (default off; needs device trackers): the run metrics — dimensionless jerk and path deviation per robot —
        are carried on the device by the tracker pass (mgx_track_metrics_*), every robot's route being exactly what export() gives
        as its mission's routes[0]["waypoints"]: set at spawn, and again when a global path replaces it.  metrics() then reads
        the device's records; otherwise it computes the same figures on the host from the robots' lists (the checker).
        sample_log (default on; False needs device_metrics): False switches the device's sample log off
        (mgx_tracks_set_logging) — the robots' `positions` / `velocities` lists, in export() too, then STAY EMPTY: the run's
        figures are in metrics() and nothing per sample ever leaves the device.
        goal_areas (default None: the export's goal_areas stays {}, as in the reference, whose plugin spawns none): a list of boxes
        ((x0, z0), (x1, z1)) in world (x, z), or "junction" (JUNCTION_GOAL_AREAS) — the first tick in which every robot's ball
        touches every box is recorded (goal_area::detect_collisions, goal_area.rs:67-103) and written into export() and metrics().
        device_goal_areas (default: whenever the missions live on the device and the world offers goal_areas_enable): the pass
        runs on the device at the end of every tick (mgx_goal_areas_*) and is read when somebody asks; False: _goal_areas_host
        below on the host every tick (the checker).
        global_planner (default None: `planning-strategy: rrt-star` raises NotImplementedError): True — robots of that strategy spawn
        Idle (RobotBundle::new, robot.rs:1195, 1294), their requests (taskpoints[0] -> taskpoints[1], a clone of the robot's forked
        stream, config.rrt) are planned in the tick they spawn, all of a tick in ONE mgx_plan_paths, and the paths are applied by ONE
        mgx_apply_global_paths at the start of the next tick — the earliest the reference's poll could see a result; "host" — the
        same with the host restatement (the checker).  Both need an engine world with device missions.  A request that fails
        leaves its robot Idle and is reported in the export; it is not retried (the reference retries with the same cloned
        stream, which can only fail again).  planner_overrides: fields of global_planner.params that replace what config.rrt
        gives (sample_half_extent, max_iterations ...).
        global_planner "sliced": the engine's planner, but a plan rides the ticks instead of holding one up (mgx_plan_submit /
        _collect, mgx_planner_set_tick_budget): the requests are submitted in the tick their robots spawn, every tick ends with one
        slice of at most plan_budget iterations per pending request (default 64: about 160 us of device time at the 2.5 us an
        iteration was measured at outside a tick), and the start of a tick collects — waiting for the slices enqueued, so that
        the tick a path arrives in depends on the request and the budget and not on timing — and applies what has ended: a
        request that takes s slices activates its robot at the start of tick s after the one it spawned in (True: tick 1).
        A mission of more than two taskpoints runs leg by leg (Mission::next_route, robot.rs:966-993): the robot keeps every
        taskpoint, the device mission gets the first route and the number of legs behind it, and a robot the tick reports as
        having ended a leg goes Idle, has its route closed and the next one opened, and asks for taskpoints[k] -> taskpoints[k+1]
        in that tick (between its halves) — applied under the same rules as a spawn's request.
        A robot despawned while it waits has its request cancelled; a request that FAILS is submitted again with the stream
        state its result carries (the reference's "try again"), and every attempt is in the export.  While requests are pending
        run() goes tick by tick."""
        self.dev = hasattr(world, "mission_tick_begin") if device_missions is None else bool(device_missions)
        self._dev_coll = (self.dev and hasattr(world, "collisions_enable")) if device_collisions is None else bool(device_collisions)
        if self._dev_coll and not self.dev:
            raise ValueError("device_collisions needs device_missions (the pass reads the device's Transforms)")
        self._coll_cursor = 0      # events of the device's log already taken into `collisions`
        self._dev_trk = (self.dev and hasattr(world, "tracks_enable")) if device_trackers is None else bool(device_trackers)
        if self._dev_trk and not self.dev:
            raise ValueError("device_trackers needs device_missions (the pass reads the device's Transforms)")
        self._dev_metrics, self._sample_log = bool(device_metrics), bool(sample_log)
        if self._dev_metrics and not self._dev_trk:
            raise ValueError("device_metrics needs device_trackers (the tracker pass carries them)")
        if not self._sample_log and not self._dev_metrics:
            raise ValueError("sample_log=False needs device_metrics (nothing else would be left of the samples)")
        if isinstance(goal_areas, str):
            if goal_areas != "junction":
                raise ValueError('goal_areas: a list of boxes ((x0, z0), (x1, z1)) or "junction"')
            goal_areas = JUNCTION_GOAL_AREAS
        self._goal_areas = None if goal_areas is None else [tuple(tuple(float(v) for v in c) for c in box) for box in goal_areas]
        if self._goal_areas is not None and not 0 < len(self._goal_areas) <= hostlib.GOAL_AREAS_MAX:
            raise ValueError(f"goal_areas: between 1 and {hostlib.GOAL_AREAS_MAX} boxes")
        self._dev_goals = self._goal_areas is not None and ((self.dev and hasattr(world, "goal_areas_enable")) if device_goal_areas is None
                                                            else bool(device_goal_areas))
        if self._dev_goals and not self.dev:
            raise ValueError("device_goal_areas needs device_missions (the pass reads the device's Transforms)")
        self._goal_clock_set = False  # the device's goal-area clock has been set to tick_no (when the first robots tick)
        self._goal_first = [{} for _ in self._goal_areas or []]  # host pass: per area, robot id -> tick of the first contact
        self._trk_clock_set = False  # the device's clock has been set to tick_no (when the first robots tick)
        self._trk_bound = 0          # samples the device's log holds at the most since it was last taken
        if environment_collisions not in (False, True, "host"):
            raise ValueError('environment_collisions: False, True or "host"')
        self._env_coll = bool(environment_collisions)
        self._dev_env_coll = environment_collisions is True and self.dev and hasattr(world, "env_collisions_enable")
        self._env_coll_cursor = 0
        self._env_collisions = {}  # (robot, collider) -> {"colliding": bool, "times": int, "aabbs": [...]}
        if global_planner not in (None, True, "host", "sliced"):
            raise ValueError('global_planner: None, True, "host" or "sliced"')
        if isinstance(plan_budget, bool) or int(plan_budget) != plan_budget or plan_budget <= 0:
            raise ValueError("plan_budget: a positive count of iterations")
        self._planner = global_planner
        self._sliced = global_planner == "sliced"
        self._plan_budget = int(plan_budget)
        self._plan_tickets = {}    # sliced: ticket -> (robot id, start, end) of the requests that ride the ticks
        self._plan_requests = []   # (robot id, start, end, stream state) of the robots spawned in this tick
        self._plans_ready = []     # (robot id, result) planned in the tick before: applied when the next one starts
        self._plan_log = []        # per request: {"robot", "status", "n_nodes", "iterations", "n_points"}
        self._has_legs = False     # some robot's mission has more than one leg: the ticks ask the world who ended one
        self._pending_track = None
        self._trk_log = []  # what _track noted since _tracks last ran
        self.name = scenario.get("name", "")
        self.cfg, self.env, self.formations = scenario["config"], scenario["environment"], scenario["formation"]["formations"]
        self.w = world
        sim, gbp = self.cfg["simulation"], self.cfg["gbp"]
        self.hz = sim["hz"]
        self.dt_ns = int(round(1e9 / self.hz))                   # Time::<Fixed>::from_hz
        self.dt32 = F(self.dt_ns * 1e-9)                         # Time<Fixed>::delta_seconds
        self.rng = WyRand(sim["prng-seed"])                      # simulation_loader.rs:651-652
        self.world_dims = _environment.world_size(self.env)      # spawner.rs:437-442
        sch = gbp["iteration-schedule"]
        self.steps = hostlib.schedule(_config.SCHEDULE_KINDS[sch["schedule"]], sch["internal"], sch["external"])
        self.comms_radius = self.cfg["robot"]["communication"]["radius"]
        self.failure_rate = float(F(self.cfg["robot"]["communication"]["failure-rate"]))
        self.max_speed = self.cfg["robot"]["target-speed"]
        self.despawn = sim["despawn-robot-when-final-waypoint-reached"]
        self.method = neighbours_method
        world.set_environment(self.env)                          # simulation_loader.rs:154-162
        self.spawners = [spawner.FormationSpawner(i, f) for i, f in enumerate(self.formations)]
        if hasattr(world, "reserve"):  # (the engine: robots that spawn while the world runs are appended on the device)
            world.reserve(self._robots_expected())
        self.robots = []           # per robot: dict (see _add_robot)
        self._translation = np.zeros((0, 3), dtype=F)
        self.tick_no, self.next_number, self.K = 0, 1, None
        self.events = []           # (tick, connections created, pairs deleted)
        self._collisions = {}      # (robot a, robot b), a < b -> {"colliding": bool, "times": int, "aabbs": [...]}
        if self._dev_coll:
            world.collisions_enable(True, method=neighbours_method)
        if self._dev_env_coll:
            world.env_collisions_enable(self.env)
        elif self._env_coll:
            self._colliders, self._collider_vertices = hostlib.env_colliders(self.env)
        if self._dev_goals:
            world.goal_areas_enable(self._goal_areas, next_tick=0)
        if self._dev_trk:
            world.tracks_enable(True, period_ns=self.TRACK_PERIOD_NS, tick_ns=self.dt_ns, next_tick=0, sample_capacity=self.TRACK_LOG_SAMPLES)
        if self._dev_metrics:
            world.track_metrics_enable(True, max_route_points=self.METRIC_ROUTE_POINTS)
            if not self._sample_log:
                world.tracks_set_logging(False)
        if self._planner is not None:
            from . import global_planner as _gp
            self._plan_params = _gp.params_from_config(self.cfg, **(planner_overrides or {}))
            _gp.check_params(self._plan_params)
            if (self._planner is True or self._sliced) and self.dev and hasattr(world, "planner_enable"):
                world.planner_enable(self.env, self._plan_params)
            if self._sliced:
                if not (self.dev and hasattr(world, "plan_submit")):
                    raise NotImplementedError('global_planner "sliced" needs an engine world with device missions')
                world.planner_set_tick_budget(self._plan_budget)
        self.entities = spawner.EntityAllocator()  # the robots' Entity bits = their graphs' order (id.rs:19-54)

    TRACK_PERIOD_NS = 100_000_000  # the trackers' timers (spawner.rs:627-628)
    TRACK_LOG_SAMPLES = 1 << 18    # room of the device's sample log: drained before it can fill
    METRIC_ROUTE_POINTS = 256      # room per robot for the route its deviation is measured against
    RESERVE_LIMIT = 256  # robots reserved at most for formations that repeat forever (beyond it the engine doubles its head-room)

    def _robots_expected(self):
        """robots the formations will ever spawn (removed ones included) where that is finite; formations that repeat forever:
        what they spawn within the scenario's max-time, RESERVE_LIMIT at the most"""
        horizon_ns = float(self.cfg["simulation"]["max-time"]) * 1e9
        total = 0
        for f in self.formations:
            rep = f["repeat"]
            if rep is None:
                spawns = 1
            elif rep["times"] is not None:
                spawns = 1 + rep["times"]
            elif rep["every"] > 0 and np.isfinite(horizon_ns):
                spawns = 1 + int(max(horizon_ns - f["delay"], 0) // rep["every"])
            else:
                return self.RESERVE_LIMIT
            total += f["robots"] * spawns
        return int(min(total, self.RESERVE_LIMIT))

    # -- spawn_formation (spawner.rs:415-649) + RobotBundle::new (robot.rs:1134-1356) -------------------
    def _add_robot(self, desc, formation_index):
        planned = desc["planning-strategy"] != "only-local"
        if planned:
            if self._planner is None:
                raise NotImplementedError("planning-strategy rrt-star: the global planner is outside the hot path")
            if not (self.dev and hasattr(self.w, "apply_global_paths") and (self._planner == "host" or hasattr(self.w, "planner_enable"))):
                raise NotImplementedError("planning-strategy rrt-star: the global planner needs an engine world with device missions")
        rb = self.cfg["robot"]
        taskpoints = desc["waypoints"]
        # Mission::global keeps every taskpoint and opens with the route [taskpoint 0, taskpoint 1] (robot.rs:862-908); the later
        # legs are planned when the earlier ones end (_legs_ended)
        states = taskpoints[:2] if planned else taskpoints
        legs_after = len(taskpoints) - 2 if planned else 0
        mean0, prior, dt = robot_initial_state(states[0], states[1], desc["timesteps"], desc["radius"], rb["target-speed"], rb["planning-horizon"])
        if planned:
            mean0[:] = np.asarray(states[0], dtype=F).astype(np.float64)  # horizon state = start (robot.rs:1195)
        if self.K is None:
            self.K = len(desc["timesteps"])
        path = np.array([s[:2] for s in states], dtype=np.float32)  # the route's positions (robot.rs:1310-1315)
        key = self.entities.alloc()
        rid = self.w.add_robot(mean0, prior, dt, float(desc["radius"]), path=path, order_key=key)
        assert rid == len(self.robots)
        t0 = F(desc["radius"]) / F(2.0) / F(rb["target-speed"])
        self.robots.append({"id": rid, "formation": formation_index, "radius": F(desc["radius"]), "waypoints": [s.copy() for s in states],
                            "target": 1, "alive": True, "completed": False, "started_at": self.elapsed(), "finished_at": None,
                            "time_scale": float(self.dt32 / t0), "colour": desc["colour"], "rng": desc["rng"],
                            "strategy": desc["planning-strategy"], "reach": desc["waypoint-reached-when-intersects"],
                            "finish": desc["finished-when-intersects"], "positions": [], "velocities": [], "travelled": 0.0,
                            "trk_elapsed": 0, "trk_prev": None, "entity": key, "idle": planned,
                            # the legs of a global-planner mission: every taskpoint, the leg under way, the legs that ended (as
                            # export() gives them, with the tick they ended in) and when the one under way was opened; the tick of
                            # every entry of `positions` (metrics() measures a sample against the route of the leg it was taken in)
                            "taskpoints": [s.copy() for s in taskpoints] if planned else None, "leg": 0, "routes": [],
                            "route_started_at": self.elapsed(), "position_ticks": []})
        self._translation = np.vstack([self._translation, np.array([[states[0][0], -1.5, states[0][1]]], dtype=F)])  # spawner.rs:548
        if self.dev:
            me = self.robots[-1]

            def rule(when):
                kind, n = when["intersects-with"]
                var = 0 if kind == "current" else (self.K - 1 if kind == "horizon" or n >= self.K else n)
                dkind, meter = when["distance"]
                lim = me["radius"] * me["radius"] if dkind == "robot-radius" else F(meter) * F(meter)
                return var, float(lim)
            (rv, rd), (fv, fd) = rule(me["reach"]), rule(me["finish"])
            self.w.mission_set(rid, np.array([s_[:2] for s_ in states[1:]], dtype=np.float64), rv, fv, rd, fd,
                               self._translation[-1], me["time_scale"], **({"legs_after": legs_after} if legs_after else {}))
            self._has_legs = self._has_legs or legs_after > 0
            if self._dev_metrics:
                self.w.track_metrics_set_route(rid, self._route(me))
            if planned:  # Mission::global (robot.rs:1294): Idle until a path has been found
                self.w.set_idle(rid, True)
                self._plan_requests.append((rid, tuple(float(v) for v in states[0][:2]), tuple(float(v) for v in states[1][:2]),
                                            desc["rng"].state))

    @staticmethod
    def _points(states):
        return [[float(s[0]), float(s[1])] for s in states]

    @staticmethod
    def _route(r):
        """a robot's route as export() gives it: the waypoints of the last of mission.routes, the leg under way"""
        return Simulation._points(r["waypoints"])

    @property
    def translation(self):
        """Transform::translation of every robot [n, 3] f32 (fetched from the device when the missions live there)"""
        if self.dev and self.robots:
            tr = self.w.mission_read()[0]
            self._translation[:len(tr)] = tr[:len(self._translation)]
        return self._translation

    # -- progress_missions (robot.rs:578-633) + the path-finding completion handler (robot.rs:643-799) ----------------------
    def _legs_ended(self, ids):
        """the device reported these robots at the last waypoint of a route with legs left (Mission::next_route, robot.rs:966-993):
        the leg's route is closed, the next one [taskpoint k, taskpoint k+1] opened, the robot Idle (the engine has made it so), and
        the path-finding request of progress_missions queued (robot.rs:578-633): between the TASKPOINTS' own positions (:601-602),
        from the robot's forked stream as it stands (:622 clones the component; nothing in this runner draws from it)"""
        for rid in ids:
            r = self.robots[int(rid)]
            now = self.elapsed()
            r["routes"].append({"waypoints": self._route(r), "started_at": r["route_started_at"], "finished_at": now, "end_tick": self.tick_no})
            r["leg"] += 1
            a, b = r["taskpoints"][r["leg"]], r["taskpoints"][r["leg"] + 1]
            r["waypoints"], r["target"], r["idle"], r["route_started_at"] = [a.copy(), b.copy()], 1, True, now
            self._plan_requests.append((r["id"], tuple(float(v) for v in a[:2]), tuple(float(v) for v in b[:2]), r["rng"].state))

    def _plan(self):
        """the requests of the robots that spawned in this tick (before its FixedUpdate) or ended a leg in it (between the tick's
        halves, ahead of its planner slice), in one call each; what comes back waits for the next tick"""
        reqs, self._plan_requests = self._plan_requests, []
        if not reqs:
            return
        if self._sliced:
            for q, t in zip(reqs, self.w.plan_submit([q[1:] for q in reqs])):
                self._plan_tickets[t] = q[:3]
            return
        if self._planner == "host":
            from . import global_planner as _gp
            res = _gp.plan_paths(self.env, [q[1:] for q in reqs], self._plan_params)
        else:
            res = self.w.plan_paths([q[1:] for q in reqs])
        self._plans_ready += [(q[0], r) for q, r in zip(reqs, res)]

    def _apply_plans(self):
        """the paths planned in the tick before: tracking path, variables, tracking factors, route and MissionState::Active of
        every robot whose request succeeded, in one call"""
        if self._plan_tickets:
            self._collect_plans()
        ids, paths, means = self._gather_plans()
        if ids:
            self.w.apply_global_paths(ids, paths, np.stack(means), reset_tracking=True, route=True, activate=True)
            self._plans_applied(ids)

    def _gather_plans(self):
        """what is ready goes into the request log, and the plans that succeeded for robots still alive come back as (robot ids,
        paths, means): the arguments of ONE apply_global_paths — this run's own (_apply_plans), or an Ensemble's for all its members"""
        ready, self._plans_ready = self._plans_ready, []
        if not ready:
            return [], [], []
        from .driver import global_path_plan
        rb = self.cfg["robot"]
        ids, paths, means = [], [], []
        for rid, r in ready:
            self._plan_log.append({"robot": rid, "status": int(r["status"]), "n_nodes": int(r["n_nodes"]), "iterations": int(r["iterations"]),
                                   "n_points": int(len(r["path"]))})
            me = self.robots[rid]
            if r["status"] != 0 or not me["alive"]:
                continue
            wps, m = global_path_plan(r["path"], rb["target-speed"], rb["planning-horizon"], self.K)
            ids.append(rid)
            paths.append(np.ascontiguousarray(wps[:, :2]))
            means.append(m)
            me["waypoints"], me["target"], me["idle"] = [w.copy() for w in wps], 1, False
        return ids, paths, means

    def _plans_applied(self, ids):
        """behind the apply_global_paths that took these robots' plans"""
        if self._dev_metrics:  # (the robots were Idle so far — since they spawned, or since their last leg ended: no sample was
            #                      measured against the route this one replaces; from here on samples belong to this leg's path)
            for rid in ids:
                self.w.track_metrics_set_route(rid, self._route(self.robots[rid]))

    def _collect_plans(self):
        """sliced: the requests that have ended by the slices enqueued so far -> _plans_ready; a robot that is gone has its
        request cancelled, a request that failed goes in again with the stream where the attempt left it"""
        self._cancel_dead_plans()
        while self._plan_tickets:
            done = self.w.plan_collect(wait=True, capacity=len(self._plan_tickets))
            if not done:
                break
            self._take_plans(done)

    def _cancel_dead_plans(self):
        for t in [t for t, q in self._plan_tickets.items() if not self.robots[q[0]]["alive"]]:
            self.w.plan_cancel(t)
            del self._plan_tickets[t]

    def _take_plans(self, done):
        """requests of this run that have ended, in the order the world handed them out"""
        for r in done:
            rid, start, end = self._plan_tickets.pop(r["ticket"])
            self._plans_ready.append((rid, r))
            if r["status"] != 0:  # (submitted again by this tick's _plan, with the robots that spawn in it)
                self._plan_requests.append((rid, start, end, r["wyrand_state"]))

    def _spawn(self):
        for sp in self.spawners:
            sp.tick(self.dt_ns)
            if sp.ready_to_spawn():
                sp.spawn()
                descs = spawner.spawn_formation(self.formations[sp.index], self.cfg, self.world_dims, self.rng)
                for d in descs or []:  # None: "failed to spawn formation", the reference logs and skips
                    self._add_robot(d, sp.index)

    def elapsed(self):
        return self.tick_no * self.dt_ns * 1e-9

    # -- reached_waypoint (robot.rs:2080-2176) --------------------------------------------------------------
    def _reached_waypoint(self):
        todo = [r for r in self.robots if r["alive"] and not r["completed"]]
        if not todo:
            return
        means = {}

        def mean_of(var):
            if var not in means:
                means[var] = self.w.read_variable_means(var)
            return means[var]
        for r in todo:
            last = r["target"] == len(r["waypoints"]) - 1
            when = r["finish"] if last else r["reach"]
            kind, n = when["intersects-with"]
            var = 0 if kind == "current" else (self.K - 1 if kind == "horizon" or n >= self.K else n)
            est = mean_of(var)[r["id"], :2].astype(F)
            dkind, meter = when["distance"]
            limit = r["radius"] * r["radius"] if dkind == "robot-radius" else F(meter) * F(meter)
            d = est - r["waypoints"][r["target"]][:2]
            if F(d[0] * d[0] + d[1] * d[1]) < limit:
                r["target"] += 1                                   # Route::advance
                if r["target"] >= len(r["waypoints"]):             # Mission::next_route: the only route is done
                    r["completed"], r["finished_at"] = True, self.elapsed()
                    if self.despawn:
                        self.w.remove_robot(r["id"])
                        self.entities.free(r["entity"])
                        r["alive"] = False

    # PositionTracker / VelocityTracker (planner/tracking.rs:104-122,189-218; 100 ms timers, spawner.rs:620-621):
    # FixedUpdate systems over Changed<Transform>, i.e. the robots that moved this tick; sampled after the move
    def _track(self, moving, translation, now):
        """track_robots (export.rs / tracking: a sample of every moving robot's Transform every 100 ms of simulated time).  The tick
        only NOTES what the samples are taken from — the moving robots' ids and their rows of the Transforms; the per-robot lists
        the export holds (positions, velocities with their measuring spans) are made from the notes when somebody reads them
        (_tracks): a dictionary per robot per tick was a fifth of a scenario's wall time."""
        if moving:
            ids = np.fromiter((r["id"] for r in moving), dtype=np.int64, count=len(moving))
            self._trk_log.append((ids, np.asarray(translation)[ids].copy(), now))

    def _tracks(self):
        """bring every robot's positions / velocities up to the last tick noted by _track (device trackers: up to the last tick
        enqueued — the samples of the device's log, whose velocities are the device's own; `travelled` comes along)"""
        if self._dev_trk:
            self._tracks_device()
            return
        log, self._trk_log = self._trk_log, []
        for ids, rows, now in log:
            tick = int(round(now / (self.dt_ns * 1e-9))) - 1
            for k, rid in enumerate(ids):
                r = self.robots[int(rid)]
                r["trk_elapsed"] += self.dt_ns
                if r["trk_elapsed"] < 100_000_000:
                    continue
                r["trk_elapsed"] %= 100_000_000
                pos = rows[k]
                r["positions"].append([float(pos[0]), float(pos[2])])
                r.setdefault("position_ticks", []).append(tick)  # (a bare tracker record, as the trackers' checkers keep, has no legs)
                if r["trk_prev"] is not None:
                    dt = now - r["trk_prev"][1]
                    v = (pos - r["trk_prev"][0]) / F(dt)
                    r["velocities"].append({"velocity": [float(v[0]), float(v[1]), float(v[2])], "timestamp": now,
                                            "measured_over": {"secs": int(dt), "nanos": int(round((dt - int(dt)) * 1e9))}})
                r["trk_prev"] = (pos, now)

    def _tracks_device(self):
        if not self._trk_clock_set:  # (no robot has ticked yet: nothing sampled, nothing travelled)
            return
        samples, _, dropped, dist = self.w.tracks_take()
        self._trk_bound = 0
        if dropped:
            raise hostlib.MgxError(f"the device's tracker log was full: {dropped} samples were not stored")
        for r, d in zip(self.robots, dist):
            r["travelled"] = float(d)
        for tick, rid, span, pos, vel in zip(samples["tick"].tolist(), samples["robot"].tolist(), samples["span_ticks"].tolist(),
                                             samples["position"].tolist(), samples["velocity"].tolist()):
            r = self.robots[rid]
            r["positions"].append([pos[0], pos[2]])
            r.setdefault("position_ticks", []).append(tick)  # (a bare tracker record, as the trackers' checkers keep, has no legs)
            if span:
                now = (tick + 1) * self.dt_ns * 1e-9
                dt = now - (tick - span + 1) * self.dt_ns * 1e-9
                r["velocities"].append({"velocity": [vel[0], vel[1], vel[2]], "timestamp": now,
                                        "measured_over": {"secs": int(dt), "nanos": int(round((dt - int(dt)) * 1e9))}})

    def _tracks_room(self, ticks, robots):
        """before `ticks` more ticks of `robots` live robots are enqueued: take the device's log in if they could fill it.  A
        robot gives at most one sample per tick and, its timer's remainder being below the period, at most
        ticks * dt_ns / period + 1 samples in `ticks` ticks."""
        if not self._dev_trk:
            return
        if not self._trk_clock_set:
            self.w.tracks_set_clock(self.tick_no)
            self._trk_clock_set = True
        if not self._sample_log:  # (nothing is appended: nothing to drain)
            return
        most = robots * min(ticks, ticks * self.dt_ns // self.TRACK_PERIOD_NS + 1)
        if self._trk_bound + most > self.TRACK_LOG_SAMPLES:
            self._tracks_device()
        self._trk_bound += most

    # update_robot_robot_collisions (planner/collisions.rs:72-140, FixedUpdate): every pair of live robots, bounding
    # spheres of their Ball(radius) at the Transform's (x, z) — parry2d 0.13 BoundingSphere::intersects, restated from its
    # published source (third party, absent from /root/reference): |c_b - c_a|^2 <= (r_a + r_b)^2 in f32 — through the
    # Free / Colliding state machine of CollisionHistory (:455-495): a Free -> Colliding edge is one collision, recorded with
    # the intersection of the two balls' AABBs (:113-119).  Robot - environment collisions: _collide_environment below.
    @property
    def collisions(self):
        """(robot a, robot b), a < b -> {"colliding", "times", "aabbs"}.  With the pass on the device the new events of its log are
        taken in first (the one read that waits for the device); "colliding" then only says that the pair has met — the
        Free / Colliding state itself stays on the device."""
        if getattr(self, "_dev_coll", False):
            self._coll_cursor = _take_in(self._collisions, self.w.collisions_read(self._coll_cursor), "robot_a", "robot_b", "collision")
        return self._collisions

    @collisions.setter
    def collisions(self, value):
        self._collisions = value

    def _collide(self, alive, translation):
        if len(alive) < 2:
            return
        ids = np.array([r["id"] for r in alive])
        rad = np.array([r["radius"] for r in alive], dtype=F)
        pos = np.ascontiguousarray(translation[ids][:, [0, 2]], dtype=F)
        d = pos[None, :, :] - pos[:, None, :]                        # d[i, j] = c_j - c_i (f32)
        rs = rad[:, None] + rad[None, :]
        hit = np.triu(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] <= rs * rs, k=1)
        now = {(int(ids[i]), int(ids[j])): (i, j) for i, j in zip(*np.nonzero(hit))}
        _edges(self.collisions, now, lambda key, ij: (np.maximum(pos[ij[0]] - rad[ij[0]], pos[ij[1]] - rad[ij[1]]),
                                                      np.minimum(pos[ij[0]] + rad[ij[0]], pos[ij[1]] + rad[ij[1]])))

    # update_robot_environment_collisions (planner/collisions.rs:368-438, FixedUpdate): every live robot's Ball against every
    # collider of the map (hostlib.env_colliders), the contact of include/mgx.h, the same Free / Colliding state machine; a
    # Free -> Colliding edge is one collision, recorded with robot_aabb intersected with the collider's AABB (:417-426)
    @property
    def environment_collisions(self):
        """(robot, collider) -> {"colliding", "times", "aabbs"}; empty while the option is off.  With the pass on the device the new
        events of its log are taken in first (the one read that waits for the device)."""
        if self._dev_env_coll:
            self._env_coll_cursor = _take_in(self._env_collisions, self.w.env_collisions_read(self._env_coll_cursor), "robot", "collider",
                                             "environment collision")
        return self._env_collisions

    def _collide_environment(self, alive, translation):
        if not self._env_coll or self._dev_env_coll:
            return
        seen = {}
        if alive and len(self._colliders):
            ids = np.array([r["id"] for r in alive])
            rad = np.array([r["radius"] for r in alive], dtype=F)
            pos = np.ascontiguousarray(np.asarray(translation)[ids][:, [0, 2]], dtype=F)
            hit = environment_contacts(self._colliders, self._collider_vertices, pos, rad) & np.isfinite(pos).all(axis=1)[:, None]
            seen = {(int(ids[i]), int(k)): i for i, k in zip(*np.nonzero(hit))}
        _edges(self._env_collisions, seen, lambda key, i: (np.maximum(pos[i] - rad[i], self._colliders[key[1]]["mins"]),
                                                           np.minimum(pos[i] + rad[i], self._colliders[key[1]]["maxs"])))

    # goal_area::detect_collisions (goal_area.rs:67-103, FixedUpdate): every live robot's Ball against every goal area's box, the
    # contact of include/mgx.h; the first tick in which the two touch is kept, later ones are not looked at
    def _goal_areas_host(self, alive, translation, tick):
        if self._goal_areas is None or self._dev_goals or not alive:
            return
        ids = np.array([r["id"] for r in alive])
        rad = np.array([r["radius"] for r in alive], dtype=F)
        pos = np.ascontiguousarray(np.asarray(translation)[ids][:, [0, 2]], dtype=F)
        for i, a in zip(*np.nonzero(goal_area_contacts(self._goal_areas, pos, rad))):
            self._goal_first[int(a)].setdefault(int(ids[i]), int(tick))

    def _goal_clock(self):
        """before the first mission tick: the device's goal-area clock names the tick that is coming"""
        if self._dev_goals and not self._goal_clock_set:
            self.w.goal_areas_set_clock(self.tick_no)
            self._goal_clock_set = True

    @property
    def goal_arrivals(self):
        """per goal area: robot id -> tick index of the first pass in which the two touched, in (tick, robot) order; [] while
        no areas are configured.  With the pass on the device this is the one read that waits for it."""
        if self._goal_areas is None:
            return []
        if self._dev_goals:
            first = [{} for _ in self._goal_areas]
            for e in self.w.goal_areas_read()[0]:
                first[int(e["area"])][int(e["robot"])] = int(e["tick"])
        else:
            if self.dev:
                self._flush_trackers(synchronise=True)
            first = self._goal_first
        return [dict(sorted(h.items(), key=lambda kv: (kv[1], kv[0]))) for h in first]

    def _goal_areas_export(self):
        """export.rs:235-247, 556-571: {area: {"aabb": {"mins", "maxs"}, "history": {robot: seconds}}} — the robots' keys are those
        of export()["robots"]; seconds: hostlib.goal_seconds (Time<Fixed>::elapsed_seconds() inside that FixedUpdate)"""
        if self._goal_areas is None:
            return {}
        lo, hi = goal_area_boxes(self._goal_areas)
        return {str(a): {"aabb": _box(lo[a], hi[a]), "history": {str(rid): hostlib.goal_seconds(k, self.dt_ns) for rid, k in h.items()}}
                for a, h in enumerate(self.goal_arrivals)}

    def _flush_trackers(self, synchronise=False):
        """device missions: the samples of the last tick, taken from the Transforms that tick sent to the host behind its
        launches (complete after the next synchronisation — the next tick's own, or an explicit one here)"""
        if self._pending_track is None:
            return
        if not self._host_needs_transforms():  # (trackers and collision passes all on the device: nobody waits, nothing comes back)
            self._pending_track = None
            return
        if synchronise:
            self.w.synchronize()
        moving, now, alive, tick = self._pending_track
        self._pending_track = None
        tr = self.w.mission_translations()
        if not self._dev_trk:
            self._track(moving, tr, now)
        if not self._dev_coll:
            self._collide(alive, tr)
        self._collide_environment(alive, tr)
        self._goal_areas_host(alive, tr, tick)

    def _host_needs_transforms(self):
        """a host tracker or a host collision pass still reads every tick's Transforms"""
        return (not self._dev_trk or not self._dev_coll or (self._env_coll and not self._dev_env_coll)
                or (self._goal_areas is not None and not self._dev_goals))

    # A device tick in three parts around the two world-wide calls (mission_tick_begin, mission_tick_end): _tick_device makes them
    # for this run alone; an Ensemble (ensemble.py) makes each of them ONCE for all its members and runs the parts per member
    def _tick_device_before(self):
        self._tracks_room(1, sum(1 for r in self.robots if r["alive"]))
        self._goal_clock()

    def _tick_device_between(self, next_number, created, deleted, fin, legs=()):
        """what mission_tick_begin gave (legs: the robots of this run that ended a leg in it, mission_legs_ended) -> the run's
        bookkeeping and this tick's comms draws; the antenna bytes for mission_tick_end (one per robot of this run; None: nothing
        fails)"""
        self.next_number = next_number
        self._flush_trackers()
        if created or deleted:
            self.events.append((self.tick_no, created, deleted))
        for rid in fin:                                            # reached_waypoint completed the mission (robot.rs:2150-2176)
            r = self.robots[int(rid)]
            r["target"] = len(r["waypoints"])
            r["completed"], r["finished_at"] = True, self.elapsed()
            if self.despawn:
                r["alive"] = False
                self.entities.free(r["entity"])
        self._legs_ended(legs)
        live = [r for r in self.robots if r["alive"]]
        ant = None
        if live:
            active = np.array([not self.rng.gen_bool(self.failure_rate) for _ in live], dtype=np.uint8)  # robot.rs:1599
            if self.failure_rate > 0.0:
                ant = np.ones(len(self.robots), dtype=np.uint8)
                ant[[r["id"] for r in live]] = active
        moving = [r for r in live if not r["completed"] and not r["idle"]]
        self._pending_track = (moving, (self.tick_no + 1) * self.dt_ns * 1e-9, live, self.tick_no)  # (read once mission_tick_end has run)
        return ant

    def _tick_device(self):
        w = self.w
        self._tick_device_before()
        ant = self._tick_device_between(*w.mission_tick_begin(self.comms_radius, self.next_number, despawn_finished=self.despawn, method=self.method),
                                        legs=w.mission_legs_ended() if self._has_legs else ())
        self._plan()  # (the next legs of the robots that have just ended one: ahead of this tick's planner slice)
        w.mission_tick_end(self.steps, float(self.max_speed), float(self.dt32), antennas=ant)

    def tick(self):
        w = self.w
        self._apply_plans()
        self._spawn()
        self._plan()
        if self.robots and self.dev:
            self._tick_device()
        elif self.robots:
            self._reached_waypoint()
            self.next_number, created, deleted = w.update_topology(self._translation, self.comms_radius, self.next_number, method=self.method)
            if created or deleted:
                self.events.append((self.tick_no, created, deleted))
            live = [r for r in self.robots if r["alive"]]
            if live:
                active = np.array([not self.rng.gen_bool(self.failure_rate) for _ in live], dtype=np.uint8)  # robot.rs:1599
                if self.failure_rate > 0.0:
                    w.set_antennas(np.array([r["id"] for r in live], dtype=np.int32), active)
            moving = [r for r in live if not r["completed"]]
            if moving:
                ids = np.array([r["id"] for r in moving], dtype=np.int32)
                m0, m1 = w.read_variable_means(0), w.read_variable_means(1)
                ts = np.array([r["time_scale"] for r in moving])
                change = ts[:, None] * (m1[ids] - m0[ids])                                   # robot.rs:2314
                self._translation[ids, 0] += change[:, 0].astype(F)                          # robot.rs:2328-2329
                self._translation[ids, 2] += change[:, 1].astype(F)
                for r, c in zip(moving, change):
                    r["travelled"] += float(np.hypot(c[0], c[1]))
                w.tick(robots=ids, waypoints_xy=np.array([r["waypoints"][r["target"]][:2] for r in moving], dtype=np.float64),
                       time_scale=ts, what=np.full(len(moving), 3, dtype=np.uint8), max_speed=float(self.max_speed),
                       delta_t=float(self.dt32), steps=self.steps)                          # prior updates + iterate_gbp_v2
            else:
                w.iterate(self.steps)
            self._track(moving, self._translation, (self.tick_no + 1) * self.dt_ns * 1e-9)
            self._collide(live, self._translation)
            self._collide_environment(live, self._translation)
            self._goal_areas_host(live, self._translation, self.tick_no)
        self.tick_no += 1

    def finished(self):
        """AllFormationsFinished: every spawner is exhausted and every spawned robot completed its mission."""
        return all(sp.exhausted() for sp in self.spawners) and all(r["completed"] for r in self.robots)

    # -- many ticks per call (device missions): what lies between two spawns is ONE mgx_mission_run ------------------
    def _quiet_ticks(self, cap):
        """how many ticks, the coming one included, pass before a spawner acts again (becomes ready, or runs out): the
        spawners' timers run ahead on copies"""
        sps = [sp.clone() for sp in self.spawners]
        n = 0
        while n < cap:
            was = [sp.exhausted() for sp in sps]
            for sp in sps:
                sp.tick(self.dt_ns)
            if any(sp.ready_to_spawn() for sp in sps) or [sp.exhausted() for sp in sps] != was:
                break
            n += 1
        return n

    def _run_chunk(self, cap):
        """One frame's Update (the spawners) and then every FixedUpdate up to the next frame in which a spawner acts, in one
        engine call: identical to tick() that many times — the per-tick bookkeeping (events, completions, trackers,
        collisions) is replayed from what the call returns per tick."""
        self._apply_plans()
        self._spawn()
        self._plan()
        if not self.robots:
            self.tick_no += 1
            return
        if self._has_legs and self._plan_tickets:
            # requests ride this tick's slice, and a robot that ends a leg in it must submit its next one AHEAD of that slice: the
            # tick in its two halves (as tick() makes it)
            self._tick_device()
            self.tick_no += 1
            return
        self._flush_trackers(synchronise=True)
        # (planned paths are applied one tick on; a pending plan is looked for at the start of every tick)
        m = 1 + (self._quiet_ticks(cap - 1) if cap > 1 and not self._plans_ready and not self._plan_tickets else 0)
        self._tracks_room(m, sum(1 for r in self.robots if r["alive"]))
        self._goal_clock()
        host_tr = self._host_needs_transforms()
        out = self.w.mission_run(m, self.comms_radius, self.next_number, self.steps, float(self.max_speed), float(self.dt32),
                                 despawn_finished=self.despawn, method=self.method, failure_rate=self.failure_rate,
                                 wyrand_state=self.rng.state, stop_when_all_finished=all(sp.exhausted() for sp in self.spawners),
                                 want_translations=host_tr)
        self.next_number, self.rng.state = out["next_number"], out["wyrand_state"]
        # the real spawners live through the same frames (nothing happens in them) — the frames the call made: it returns early
        # behind a tick in which a leg ended
        for _ in range(out["ticks"] - 1):
            for sp in self.spawners:
                sp.tick(self.dt_ns)
        for j in range(out["ticks"]):
            if out["created"][j] or out["deleted"][j]:
                self.events.append((self.tick_no, int(out["created"][j]), int(out["deleted"][j])))
            for rid in out["finished"][j]:
                r = self.robots[int(rid)]
                r["target"] = len(r["waypoints"])
                r["completed"], r["finished_at"] = True, self.elapsed()
                if self.despawn:
                    r["alive"] = False
                    self.entities.free(r["entity"])
            self._legs_ended(out["legs_ended"][j] if self._has_legs else ())
            if host_tr:
                live = [r for r in self.robots if r["alive"]]
                tr = out["translations"][j]
                if not self._dev_trk:
                    self._track([r for r in live if not r["completed"] and not r["idle"]], tr, (self.tick_no + 1) * self.dt_ns * 1e-9)
                if not self._dev_coll:
                    self._collide(live, tr)
                self._collide_environment(live, tr)
                self._goal_areas_host(live, tr, self.tick_no)
            self.tick_no += 1
        if self._plan_requests:  # legs ended in the call's last tick: their requests go out as in tick(), and a sliced one takes
            self._plan()         # that tick's slice, which the call enqueued when nothing was pending
            if self._sliced:
                self.w.plan_advance(self._plan_budget)

    def run(self, max_ticks=None, max_time=None, chunk=256):
        """chunk: device missions — up to that many ticks per engine call (mgx_mission_run) where no spawner acts; 1: tick by tick"""
        limit = self.cfg["simulation"]["max-time"] if max_time is None else max_time
        while not self.finished() and self.elapsed() < limit and (max_ticks is None or self.tick_no < max_ticks):
            if self.dev and chunk > 1 and hasattr(self.w, "mission_run"):
                cap = 0  # ticks the loop's own conditions allow from here
                while cap < chunk and (self.tick_no + cap) * self.dt_ns * 1e-9 < limit and (max_ticks is None or self.tick_no + cap < max_ticks):
                    cap += 1
                self._run_chunk(max(cap, 1))
            else:
                self.tick()
        if self.dev:
            self._flush_trackers(synchronise=True)
        if self._dev_trk:
            self._tracks()  # (`travelled` is up to date when run() returns)
        return self

    # -- export (export.rs:249-262, 283-620) ------------------------------------------------------------------
    def export(self):
        if self.dev:
            self._flush_trackers(synchronise=True)
        self._tracks()
        sch = self.cfg["gbp"]["iteration-schedule"]
        collisions = self.collisions
        env_coll = self.environment_collisions if self._env_coll else {}
        env_count = {}
        for (rid, _), h in env_coll.items():
            env_count[rid] = env_count.get(rid, 0) + h["times"]
        robots = {}
        for r in self.robots:
            sent_i, sent_e, recv_i, recv_e = self.w.message_counts(r["id"])
            wps = [[float(s[0]), float(s[1])] for s in r["waypoints"]]
            fin = r["finished_at"] if r["finished_at"] is not None else self.elapsed()
            robots[str(r["id"])] = {
                "radius": float(r["radius"]), "positions": r["positions"], "velocities": r["velocities"],
                "collisions": {"robots": sum(h["times"] for k, h in collisions.items() if r["id"] in k),
                               "environment": env_count.get(r["id"], 0)},
                "messages": {"sent": {"internal": sent_i, "external": sent_e}, "received": {"internal": recv_i, "external": recv_e}},
                # mission.waypoints: the taskpoints (export.rs:391); routes: one entry per leg started (export.rs:400-415), the
                # one under way with its planned path — or [taskpoint k, taskpoint k+1] while it waits for one
                "mission": {"waypoints": [wps[0], wps[-1]] if not r["taskpoints"] or len(r["taskpoints"]) == 2 else self._points(r["taskpoints"]),
                            "started_at": r["started_at"], "finished_at": fin,
                            "routes": [{k: leg[k] for k in ("waypoints", "started_at", "finished_at")} for leg in r["routes"]] +
                                      [{"waypoints": wps, "started_at": r["route_started_at"], "finished_at": fin}]},
                "planning_strategy": r["strategy"], "color": r["colour"]}
        extra = {}
        if self._planner is not None:  # what became of every path-finding request; a failed one left its robot Idle
            from .global_planner import STATUS_NAMES as _PLAN_STATUS
            extra["global_planner"] = {"requests": self._plan_log,
                                       "failed": [{"robot": q["robot"], "status": _PLAN_STATUS[q["status"]]} for q in self._plan_log if q["status"] != 0]}
        return {**extra, "scenario": self.name, "makespan": self.elapsed(), "delta_t": float(self.dt32),
                "gbp": {"iterations": {"internal": sch["internal"], "external": sch["external"]}}, "robots": robots,
                "prng_seed": self.cfg["simulation"]["prng-seed"], "config": self.cfg, "obstacles": {},
                "collisions": {"robots": [{"robot_a": a, "robot_b": b, "aabbs": h["aabbs"]} for (a, b), h in sorted(collisions.items())],
                               # only the pairs that have at least one AABB (collisions.rs:282-291); "obstacle": the collider's index
                               "environment": [{"robot": a, "obstacle": k, "aabbs": h["aabbs"]}
                                               for (a, k), h in sorted(env_coll.items()) if h["aabbs"]]},
                # goal_areas: the reference registers GoalAreaPlugin but its only system that SPAWNS goal areas
                # (setup_goal_areas_for_junction_scenario, goal_area.rs:105-119) is commented out of the plugin (:8-11):
                # the exported map is empty in the reference itself — and here unless the caller hands areas in (goal_areas=)
                "goal_areas": self._goal_areas_export()}

    # -- the run metrics (the reference's scripts/ldj.py and scripts/perpendicular-path-deviation.py over an export) -----------
    def metrics(self):
        """{"robots": {id: {ldj, path_deviation, mean_deviation, max_deviation, distance_travelled, duration, dimensionless_jerk,
        deviation_sum, n_positions, n_velocities, n_unrouted}}, "summary": {figure: track_metrics.summary}, "makespan",
        "collisions": {"robots", "environment"}}.  With device_metrics the records are the device's (one read that waits);
        otherwise the streaming restatement (track_metrics.Stream) over the robots' positions / velocities lists and the routes
        export() gives — the same figures bit for bit, and the checker of the device.
        A mission of several legs: a sample is measured against the route of the leg it was taken in, in both forms (the device's
        route is replaced at every hand-over; the host form switches at the same sample).  The reference's script measures every
        position against all legs' lines concatenated (scripts/perpendicular-path-deviation.py:81-99); the streaming form does NOT —
        a position is never measured against a leg the robot had not begun or had left."""
        if self.dev:
            self._flush_trackers(synchronise=True)
        self._tracks()
        if self._dev_metrics:
            recs = self.w.track_metrics_read() if self._trk_clock_set else []
            recs = [{k: rec[k].item() for k in rec.dtype.names} for rec in recs]
            recs += [_metrics.Stream().read() for _ in range(len(self.robots) - len(recs))]
        else:
            recs = [self._stream_metrics(r) for r in self.robots]
        robots = {}
        for r, rec in zip(self.robots, recs):
            fin = r["finished_at"] if r["finished_at"] is not None else self.elapsed()
            robots[str(r["id"])] = {**_metrics.robot_metrics(rec), "distance_travelled": float(r["travelled"]), "duration": fin - r["started_at"],
                                    "dimensionless_jerk": rec["dimensionless_jerk"], "deviation_sum": rec["deviation_sum"],
                                    "n_positions": rec["n_positions"], "n_velocities": rec["n_velocities"], "n_unrouted": rec["n_unrouted"]}
        figures = ("ldj", "path_deviation", "mean_deviation", "max_deviation", "distance_travelled", "duration")
        env_coll = self.environment_collisions if self._env_coll else {}
        return {"robots": robots, "summary": {f: _metrics.summary([m[f] for m in robots.values()]) for f in figures},
                "makespan": self.elapsed(),
                "collisions": {"robots": sum(h["times"] for h in self.collisions.values()), "environment": sum(h["times"] for h in env_coll.values())},
                **self._goal_metrics()}

    def _stream_metrics(self, r):
        """the host streaming form of one robot's record: every position against the route of the leg it was taken in"""
        vel = [(v["velocity"][0], v["velocity"][2]) for v in r["velocities"]]
        if not r["routes"]:
            return _metrics.stream(vel, r["positions"], self._route(r))
        s, k, legs = _metrics.Stream(), 0, r["routes"]
        for u, w in vel:
            s.velocity(u, w)
        for (x, y), tick in zip(r["positions"], r["position_ticks"]):
            while k < len(legs) and tick >= legs[k]["end_tick"]:  # (a leg's last sample lies before the tick it ended in)
                k += 1
            s.position(x, y, legs[k]["waypoints"] if k < len(legs) else self._route(r))
        return s.read()

    def _goal_metrics(self, window=50.0):
        """{"goal_areas": {"arrivals": per area, "reached": robots in any history, "time_to_goal": {robot: first arrival minus
        started_at}, "flow": goal_flow over `window` seconds, "window"}} — the key exists only when areas are configured"""
        if self._goal_areas is None:
            return {}
        arrivals = self.goal_arrivals
        first = {}
        for h in arrivals:
            for rid, k in h.items():
                first[rid] = min(first.get(rid, k), k)
        started = {r["id"]: r["started_at"] for r in self.robots}
        n = sum(1 for rid in first if not started[rid] >= window)
        return {"goal_areas": {"arrivals": [len(h) for h in arrivals], "reached": len(first),
                               "time_to_goal": {str(rid): hostlib.goal_seconds(k, self.dt_ns) - started[rid] for rid, k in sorted(first.items())},
                               "flow": 1 / (window / n) if n else 0.0, "window": window}}

    def goal_flow(self, window=50.0):
        """metrics()["goal_areas"]["flow"] for another window (scripts/analyse-junction-scenario.py:81-109)"""
        return self._goal_metrics(window)["goal_areas"]["flow"]

    def export_json(self, path):
        with open(path, "w", encoding="utf-8") as f:
            json.dump(self.export(), f)


def run_scenario(directory, world_factory, max_ticks=None, max_time=None):
    """Load a scenario directory and run it to the end (or the given bound)."""
    sc = _config.load_scenario(directory)
    sim = Simulation(sc, world_factory(_config.world_params(sc["config"])))
    return sim.run(max_ticks=max_ticks, max_time=max_time)
