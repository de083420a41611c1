"""Many independent scenario runs in ONE world: robot groups (include/mgx.h, ROBOT GROUPS) under the scenario front-end.

The reference's experiments loop over seeds and one or two parameters and start the binary once per combination; each of those
runs has a few dozen robots and fills a few dozen of the device's workgroup slots.  An `Ensemble` runs M such scenarios — its
MEMBERS — as the groups 0 .. M-1 of one world: one launch per schedule and one synchronisation per tick for all of them, and every
member stays bit-identical to the same scenario run by a `Simulation` on a world of its own (tests/test_gpu_ensemble.py).

Nothing of `Simulation` is restated here.  Every member IS a `Simulation`, on a view of the shared world (`_MemberWorld`) that
speaks the member's own robot numbering and puts its robots into its group; the ensemble makes the two world-wide calls of a tick
once (mission_tick_begin_groups, mission_tick_end) and runs the parts of `Simulation._tick_device` around them per member; the
device's collision logs and tracker sample log are drained once and their records routed to the members by robot id.

Per member (per group of the world): the seed, the comms failure rate, the formations, max-time — and the comms radius, which the
grouped search holds per group (mission_tick_begin_groups with one radius per member), the GBP iteration schedule
(mission_tick_end with one schedule per member: mgx_mission_tick_end_groups), the enabled factor kinds but the inter-robot one
(set_group_enabled before the member's first robot: mgx_set_group_enabled) and the four factor sigmas (set_group_sigmas, likewise:
mgx_set_group_sigmas).  The per-robot observers — environment
collisions, goal areas, the run metrics — do not look at the group: the first member switches them on for the world, and every
member reads its own robots' part.

The global planner (global_planner="sliced"): the world has ONE pool of requests, and a launch runs every request of it.  Each
member's `rrt.*` is a parameter set of its group (planner_set_group_params: mgx_planner_set_group_params — member 0's is the
world's, a member that agrees with it sets nothing); a member submits its requests under its group, and per tick the ensemble
drains the pool ONCE (one plan_collect that waits), routes what has ended to the members by group and ticket, and applies every
member's new paths in ONE apply_global_paths over the union of their robots; the mission tick's one slice advances them all.
global_planner="host" plans every member's requests with the host restatement under the member's own parameters and shares only
that one apply."""
import copy

import numpy as np

from . import config as _config
from . import hostlib
from .sim import Simulation
from .world import group_steps

UNSUPPORTED = ("global_planner",)   # the options whose value True (the synchronous form) an Ensemble refuses
# what a member's Simulation may ask of the world's planner; the view offers each only where the world does
PLANNER_CALLS = ("planner_enable", "planner_set_tick_budget", "plan_submit", "plan_collect", "plan_cancel", "plan_pending", "set_idle",
                 "apply_global_paths")
# rrt.* of a member's config: a parameter set of its group where the world takes one per group
RRT_KEYS = ("step-size", "neighbourhood-radius", "collision-radius", "max-iterations", "smoothing.enabled", "smoothing.max-iterations")
# the observers an Ensemble runs on the device, and what the world has to offer for each
OBSERVERS = (("environment_collisions", "env_collisions_enable"), ("goal_areas", "goal_areas_enable"), ("device_metrics", "track_metrics_enable"))
ENV_EVENTS_PER_MEMBER = 262144   # the room a run of its own has for environment-collision events (mgx_env_collisions_enable's default)
ENV_EVENTS_MOST = 1 << 24        # ... and where an ensemble's log stops growing with its members (24 bytes a record)


SIGMAS = ("dynamics", "interrobot", "obstacle", "tracking")   # gbp.sigma-factor-*: params.sigma_* of the world, mgx_group_sigmas of a group


def _member_sigmas(sc):
    """a member's four factor sigmas as its world's params hold them"""
    p = _config.world_params(sc["config"])
    return {k: p["sigma_" + k] for k in SIGMAS}


def _rrt_settings(cfg):
    """rrt.* as (key, value), in the order of RRT_KEYS"""
    out = []
    for key in RRT_KEYS:
        v = cfg["rrt"]
        for part in key.split("."):
            v = v[part]
        out.append(("rrt." + key, v))
    return out


def _shared_settings(sc, per_group_kinds=False, per_group_sigmas=False, rrt_once=False):
    """everything the world holds once, as (key, value) in the order it is compared.  per_group_kinds: the world takes
    gbp.factors-enabled per group (mgx_set_group_enabled) — all of it but the inter-robot kind, which stays the world's.
    per_group_sigmas: it takes the four gbp.sigma-factor-* per group as well (mgx_set_group_sigmas).  rrt_once: the engine's
    planner runs the members' requests and takes no parameter set per group, so rrt.* is held once as well"""
    cfg = sc["config"]
    out = [("params." + k, v) for k, v in _config.world_params(cfg).items()
           if not (per_group_kinds and k == "enable_mask") and not (per_group_sigmas and k in tuple("sigma_" + n for n in SIGMAS))]
    if per_group_kinds:
        out.append(("gbp.factors-enabled.interrobot", cfg["gbp"]["factors-enabled"]["interrobot"]))
    out += [("gbp.lookahead-multiple", cfg["gbp"]["lookahead-multiple"]),
            ("robot.target-speed", cfg["robot"]["target-speed"]),
            ("robot.planning-horizon", cfg["robot"]["planning-horizon"]), ("simulation.hz", cfg["simulation"]["hz"]),
            ("simulation.despawn-robot-when-final-waypoint-reached", cfg["simulation"]["despawn-robot-when-final-waypoint-reached"]),
            ("environment", sc["environment"])]
    if rrt_once:
        out += _rrt_settings(cfg)
    return out


class _MemberWorld:
    """What one member's Simulation sees of the shared world: its own robots under its own ids (0, 1, .. in the order it adds them),
    in its group.  What the world holds once (environment, observers) is set up by the first member; the two halves of the
    mission tick belong to the ensemble."""

    def __init__(self, ensemble, group):
        self._e, self._group = ensemble, group
        self.ids = []            # member id -> world id
        self.coll_events = []    # this member's collision events so far, member ids, in (pass, a, b) order
        self.env_events = []     # ... and its environment-collision events, in (pass, robot, collider) order
        self.samples = []        # this member's tracker samples not taken yet
        self.plans_done = []     # this member's requests that have ended and are not taken yet, in the world's order
        self.reserved = 0

    def __getattr__(self, name):
        # the planner's side of the world, offered only where the world offers it (Simulation asks with hasattr)
        if name in PLANNER_CALLS and hasattr(self._e.world, name):
            return getattr(self, "_" + name)
        raise AttributeError(name)

    # -- set up once for the world -------------------------------------------------------------------------------------------
    def set_environment(self, env):
        if self._group == 0:
            self._e.world.set_environment(env)

    def reserve(self, n):
        self.reserved = int(n)   # (the ensemble reserves the sum once every member has said what it expects)

    def collisions_enable(self, enabled=True, method=hostlib.NEIGHBOURS_AUTO, event_capacity=0):
        if self._group == 0:
            self._e.world.collisions_enable(enabled, method=method, event_capacity=event_capacity)

    def tracks_enable(self, *args, **kwargs):
        if self._group == 0:
            self._e.world.tracks_enable(*args, **kwargs)
            self._e._log_room = int(kwargs.get("sample_capacity", 0))

    def tracks_set_clock(self, next_tick):
        pass                     # (the members tick in step: the ensemble keeps the world's one clock)

    def tracks_set_logging(self, on=True):
        if self._group == 0:
            self._e.world.tracks_set_logging(on)
            self._e._logging = bool(on)

    def env_collisions_enable(self, env, event_capacity=0):
        """the world's log holds the events of ALL members: the room a run of its own has (ENV_EVENTS_PER_MEMBER, the engine's
        default) per member, so that no member loses an event its own run would have kept — up to ENV_EVENTS_MOST records; a log that
        was full raises when it is read, here as there"""
        if self._group == 0:
            room = int(event_capacity) or ENV_EVENTS_PER_MEMBER
            self._e.world.env_collisions_enable(env, event_capacity=min(room * len(self._e.members_worlds), max(room, ENV_EVENTS_MOST)))

    def goal_areas_enable(self, areas, next_tick=0):
        if self._group == 0:
            self._e.world.goal_areas_enable(areas, next_tick=next_tick)
            self._e._goals = True

    def goal_areas_set_clock(self, next_tick):
        pass                     # (the ensemble's, like the trackers' clock)

    def track_metrics_enable(self, *args, **kwargs):
        if self._group == 0:
            self._e.world.track_metrics_enable(*args, **kwargs)

    # -- robots -----------------------------------------------------------------------------------------------------------------
    def add_robot(self, mean0, prior_diag, dt, radius, path=None, order_key=None, ghost=False):
        # the order key unique across the members, the order within a member as it was
        key = int(order_key) * len(self._e.members_worlds) + self._group
        if key >= 2 ** 64:
            raise ValueError("order key too large for an ensemble of this size")
        wid = self._e.world.add_robot(mean0, prior_diag, dt, radius, path=path, order_key=key, ghost=ghost, group=self._group)
        self._e._owner[wid] = (self._group, len(self.ids))
        self.ids.append(wid)
        return len(self.ids) - 1

    def mission_set(self, robot, *args, **kwargs):
        self._e.world.mission_set(self.ids[robot], *args, **kwargs)

    def track_metrics_set_route(self, robot, xy):
        self._e.world.track_metrics_set_route(self.ids[robot], xy)

    def message_counts(self, robot):
        return self._e.world.message_counts(self.ids[robot])

    def mission_read(self):
        tr, tg, fin = self._e.world.mission_read()
        return tr[self.ids], tg[self.ids], fin[self.ids]

    def synchronize(self):
        self._e.world.synchronize()

    # -- the device's logs, routed -----------------------------------------------------------------------------------------------
    def collisions_read(self, first=0):
        dropped = self._e._drain_collisions()
        ev = self.coll_events[int(first):]
        out = np.zeros(len(ev), hostlib.collision_event_dtype())
        for k, e in enumerate(ev):
            out[k] = e
        return out, len(self.coll_events), dropped, None

    def env_collisions_read(self, first=0):
        self._e._drain_env_collisions()
        ev = self.env_events[int(first):]
        out = np.zeros(len(ev), hostlib.env_collision_event_dtype())
        for k, e in enumerate(ev):
            out[k] = e
        return out, len(self.env_events), 0, None

    def goal_areas_read(self):
        """the world's first arrivals of this member's robots, in member ids (the order of the world's: tick, robot, area)"""
        ev, _ = self._e.world.goal_areas_read()
        mine = [(int(e["tick"]), int(e["area"]), self._e._owner[int(e["robot"])]) for e in ev]
        mine = [(t, a, r) for t, a, (g, r) in mine if g == self._group]
        out = np.zeros(len(mine), hostlib.goal_arrival_dtype())
        for k, (t, a, r) in enumerate(mine):
            out[k]["tick"], out[k]["area"], out[k]["robot"] = t, a, r
        return out, None

    def track_metrics_read(self):
        """this member's records, in member-id order"""
        return self._e.world.track_metrics_read()[self.ids]

    def tracks_take(self, capacity=None, travelled=True):
        dropped, dist = self._e._drain_tracks()
        mine, self.samples = self.samples, []
        out = np.zeros(len(mine), hostlib.track_sample_dtype())
        for k, s in enumerate(mine):
            out[k] = s
        return out, len(mine), dropped, (dist[self.ids] if len(self.ids) else np.zeros(0))

    # -- the global planner: one pool and one apply for the world, in member ids and the member's group ---------------------------
    def _planner_enable(self, env, params=None):
        """member 0 enables the world's planner with its parameters; a member whose parameters differ from member 0's sets its
        group's set (members that agree leave the world as it was)"""
        e = self._e
        if self._group == 0:
            e.world.planner_enable(env, params)
            e._plan_params = None if env is None else dict(params)
        elif env is not None and dict(params) != e._plan_params:
            if not hasattr(e.world, "planner_set_group_params"):
                raise NotImplementedError("Ensemble: members that differ in their planner's parameters need an engine world that offers "
                                          "planner_set_group_params")
            e.world.planner_set_group_params(self._group, params)

    def _planner_set_tick_budget(self, iterations):
        if self._group == 0:
            self._e.world.planner_set_tick_budget(iterations)

    def _plan_submit(self, requests):
        tickets = self._e.world.plan_submit(requests, groups=[self._group] * len(requests))
        self._e._plan_owner.update((t, self._group) for t in tickets)
        return tickets

    def _plan_collect(self, wait=False, capacity=64, point_capacity=None):
        """this member's requests that have ended (the ensemble drains the world's pool and routes by group and ticket)"""
        self._e._drain_plans(wait)
        out, self.plans_done = self.plans_done[:int(capacity)], self.plans_done[int(capacity):]
        return out

    def _plan_cancel(self, ticket):
        if self._e._plan_owner.get(ticket) != self._group:
            raise hostlib.MgxError(f"ticket {ticket} is not pending in member {self._group}")
        held = [r for r in self.plans_done if r["ticket"] == ticket]
        if held:   # (drained already: the world has handed it out)
            self.plans_done.remove(held[0])
        else:
            self._e.world.plan_cancel(ticket)
        del self._e._plan_owner[ticket]

    def _plan_pending(self):
        return sum(1 for g in self._e._plan_owner.values() if g == self._group)

    def _set_idle(self, robot, idle):
        self._e.world.set_idle(self.ids[robot], idle)

    def _apply_global_paths(self, robots, paths, means, **kwargs):
        self._e.world.apply_global_paths([self.ids[int(r)] for r in robots], paths, means, **kwargs)

    # -- the ensemble's -----------------------------------------------------------------------------------------------------------
    def mission_tick_begin(self, *args, **kwargs):
        raise RuntimeError("a member of an Ensemble does not tick on its own: Ensemble.tick()")

    mission_tick_end = mission_tick_begin


class Member:
    """One run of an Ensemble: `sim` is its Simulation; export() and metrics() give what the same scenario gives alone — frozen
    when the member was retired (its mission over, or its time up)"""

    def __init__(self, sim, view):
        self.sim, self._view = sim, view
        self.retired = False
        self._export = self._metrics = None

    def export(self):
        return copy.deepcopy(self._export) if self.retired else self.sim.export()

    def metrics(self):
        return copy.deepcopy(self._metrics) if self.retired else self.sim.metrics()

    def elapsed(self):
        return self.sim.elapsed()

    @property
    def tick_no(self):
        return self.sim.tick_no


class Ensemble:
    def __init__(self, scenarios, world, masked_resident=False, **simulation_options):
        """scenarios: one scenario dict per member (config.load_scenario, tests/golden/scenarios.json); member m's robots are in
        group m of `world`, a fresh World made with config.world_params of any of them.  The members may differ in
        simulation.prng-seed, robot.communication.failure-rate, robot.communication.radius, gbp.iteration-schedule,
        gbp.factors-enabled.{dynamic, obstacle, tracking}, gbp.sigma-factor-{dynamics, interrobot, obstacle, tracking},
        rrt.* (and max-time) and in their formations; everything the world holds once must be equal (ValueError names the first key that differs; a world
        that takes no radius, no schedule, no enabled kinds, no sigmas or — under global_planner="sliced" — no planner parameters
        per group holds that once, too; gbp.factors-enabled.interrobot is the world's always).  simulation_options go to every member's Simulation, so the members share them —
        goal_areas among them.  An Ensemble runs device missions with device robot-robot collisions and device trackers, and on
        request the device's other observers: environment_collisions=True, goal_areas, device_metrics (with sample_log=False if
        asked).  global_planner="sliced" (with plan_budget and planner_overrides, shared like the rest) runs rrt-star formations on
        the engine's planner — one pool, one collect, one apply and one slice per tick for all members — and "host" on the
        restatement.  Still refused, with NotImplementedError: global_planner=True (a synchronous mgx_plan_paths per member would
        hold every member's ticks for the slowest plan), rrt-star formations without a planner, and every option that needs each
        tick's Transforms on the host:
        environment_collisions="host", device_goal_areas=False, device_missions / device_collisions / device_trackers = False.
        masked_resident is the Ensemble's own (no Simulation sees it): True lets a world whose members differ in
        gbp.factors-enabled or in their sigmas run the ticks they share a schedule in as resident launches (World.set_group_resident) — same
        results, bit for bit; it changes nothing where the members' kinds and sigmas agree."""
        scenarios = list(scenarios)
        if not scenarios:
            raise ValueError("an Ensemble needs at least one scenario")
        if len(scenarios) > hostlib.GROUPS_MAX:
            raise ValueError(f"an Ensemble has at most {hostlib.GROUPS_MAX} members")
        planner = simulation_options.get("global_planner")
        for opt in UNSUPPORTED:
            if simulation_options.get(opt) is True:
                raise NotImplementedError(f"Ensemble: {opt}=True is not supported (a synchronous mgx_plan_paths per member would hold every "
                                          f'member\'s ticks for the length of the slowest plan); {opt}="sliced" lets the plans ride the ticks')
        if planner == "sliced":
            for needs in ("planner_enable", "plan_submit", "plan_collect", "planner_set_tick_budget", "apply_global_paths"):
                if not hasattr(world, needs):
                    raise NotImplementedError(f'Ensemble: global_planner "sliced" needs an engine world that offers {needs} (the plans ride the '
                                              "device's ticks)")
        for opt in ("device_missions", "device_collisions", "device_trackers", "device_goal_areas"):
            if simulation_options.get(opt) is False:
                raise NotImplementedError(f"Ensemble: {opt}=False is not supported (the members share the device's passes; a host pass needs every "
                                          "tick's Transforms of every member on the host)")
        if simulation_options.get("environment_collisions") == "host":
            raise NotImplementedError('Ensemble: environment_collisions="host" is not supported (the host pass needs every tick\'s Transforms on the '
                                      "host); True runs the device's pass")
        for opt, needs in OBSERVERS:
            if simulation_options.get(opt) and not hasattr(world, needs):
                raise NotImplementedError(f"Ensemble: {opt} needs an engine world that offers {needs} (the pass runs on the device)")
        for m, sc in enumerate(scenarios):
            if planner is None and any(f["planning-strategy"] != "only-local" for f in sc["formation"]["formations"]):
                raise NotImplementedError(f'Ensemble: member {m} has an rrt-star formation and no global planner was asked for (global_planner='
                                          '"sliced" or "host")')
        per_group_radius = hasattr(world, "neighbours_groups")   # (the engine's grouped search: one comms radius per group)
        per_group_steps = hasattr(world, "group_schedule_stats")  # (mgx_mission_tick_end_groups: one iteration schedule per group)
        per_group_kinds = hasattr(world, "set_group_enabled")     # (mgx_set_group_enabled: dynamic, obstacle and tracking per group)
        per_group_sigmas = hasattr(world, "set_group_sigmas")     # (mgx_set_group_sigmas: the four factor sigmas per group)
        # (mgx_planner_set_group_params: rrt.* per group; the host restatement plans each member under its own anyway)
        rrt_once = planner == "sliced" and not hasattr(world, "planner_set_group_params")

        def shared(sc):
            return (_shared_settings(sc, per_group_kinds, per_group_sigmas, rrt_once) + ([] if per_group_steps else [("gbp.iteration-schedule", sc["config"]["gbp"]["iteration-schedule"])]) +
                    ([] if per_group_radius else [("robot.communication.radius", sc["config"]["robot"]["communication"]["radius"])]))
        first = shared(scenarios[0])
        for m, sc in enumerate(scenarios[1:], 1):
            for (key, a), (_, b) in zip(first, shared(sc)):
                if a != b:
                    raise ValueError(f"Ensemble: member {m} differs from member 0 in {key} ({b!r} against {a!r}): the world holds it once")
        if not hasattr(world, "mission_tick_begin_groups"):
            raise NotImplementedError("Ensemble needs an engine world (robot groups)")
        self.world = world
        self._owner = {}          # world id -> (member, member id)
        self._coll_cursor = 0     # events of the world's collision log already routed
        self._coll_dropped = 0
        self._env_cursor = 0      # ... and of its environment-collision log
        self._logging = True      # the device appends the trackers' samples to its log (sample_log)
        self._goals = False       # goal areas are on: their clock is the ensemble's
        self._per_group_radius = per_group_radius
        self._per_group_steps = per_group_steps
        self._steps_for = self._steps = None   # the tick's schedule(s) as handed to the world, and the retired flags they were packed for
        self._log_room = 0        # room of the device's sample log (what the first member enabled the trackers with)
        self._log_bound = 0       # samples the log holds at the most since it was last drained
        self._dist = np.zeros(0)
        self._clock = None        # the tick the device's tracker clock names
        self._plan_params = None  # the planner's parameters as member 0 enabled it with: the world's
        self._plan_owner = {}     # ticket -> member, of the requests submitted and neither taken by their member nor cancelled
        self.tick_no = 0
        # every member's enabled kinds, before its first robot is added (a mask equal to the world's is none: an ensemble whose
        # members agree stays the unmasked world it was)
        if masked_resident:   # (the world's switch, before the first robot)
            if not hasattr(world, "set_group_resident"):
                raise NotImplementedError("Ensemble: masked_resident needs an engine world that offers set_group_resident")
            world.set_group_resident(True)
        masks = [_config.enable_mask(sc["config"]) for sc in scenarios]
        if per_group_kinds and any(k != masks[0] for k in masks):
            for m, k in enumerate(masks):
                world.set_group_enabled(m, k)
        # ... and its sigmas, under the same rule (equal to the world's is none: members that agree leave the world as it was)
        sigmas = [_member_sigmas(sc) for sc in scenarios]
        if per_group_sigmas and any(s != sigmas[0] for s in sigmas):
            for m, s in enumerate(sigmas):
                world.set_group_sigmas(m, **s)
        self.members_worlds = [_MemberWorld(self, m) for m in range(len(scenarios))]
        self.members = [Member(Simulation(sc, view, **simulation_options), view) for sc, view in zip(scenarios, self.members_worlds)]
        s0 = self.members[0].sim
        if not (s0.dev and s0._dev_coll and s0._dev_trk):
            raise NotImplementedError("Ensemble needs device missions, device collisions and device trackers")
        world.reserve(sum(v.reserved for v in self.members_worlds))

    # -- the device's logs: drained once, routed by robot id ------------------------------------------------------------------------
    def _drain_collisions(self):
        ev, total, dropped = self.world.collisions_read(self._coll_cursor)[:3]
        self._coll_cursor = total
        for e in ev:
            (m, a), (m2, b) = self._owner[int(e["robot_a"])], self._owner[int(e["robot_b"])]
            assert m == m2, "robots of two members collided"
            self.members_worlds[m].coll_events.append((e["pass"], a, b, e["mins"], e["maxs"]))
        return dropped

    def _drain_env_collisions(self):
        ev, total, dropped = self.world.env_collisions_read(self._env_cursor)[:3]
        if dropped:
            raise hostlib.MgxError(f"the device's environment collision log was full: {dropped} events were not stored")
        self._env_cursor = total
        for e in ev:
            m, r = self._owner[int(e["robot"])]
            self.members_worlds[m].env_events.append((e["pass"], r, e["collider"], e["mins"], e["maxs"]))

    def _drain_tracks(self):
        if self._clock is None:   # (no robot has ticked yet)
            return 0, np.zeros(len(self._owner))
        samples, _, dropped, dist = self.world.tracks_take()
        self._log_bound = 0
        for s in samples:
            m, r = self._owner[int(s["robot"])]
            self.members_worlds[m].samples.append((s["tick"], r, s["span_ticks"], s["position"], s["velocity"]))
        return dropped, dist

    def _drain_plans(self, wait):
        """every request of the world's pool that has ended, to its member's list, in the world's order (slice number, ticket): at
        most one collect that waits, whatever the pool holds"""
        while self._plan_owner:
            done = self.world.plan_collect(wait=wait, capacity=len(self._plan_owner))
            wait = False          # (what the first look left behind for want of room has ended already)
            for r in done:
                g = self._plan_owner[r["ticket"]]
                assert g == r["group"], "a request came back under another group than it was submitted under"
                self.members_worlds[g].plans_done.append(r)
            if not done:
                break

    def _apply_members_plans(self, active):
        """the first pass of a tick: what the planner has finished for every member, and ONE apply_global_paths over the union of
        the members' robots (the call synchronises the stream and repacks every path on the host: once, not once per member)"""
        sliced = [m for m in active if m.sim._plan_tickets]
        for m in sliced:
            m.sim._cancel_dead_plans()
        if any(m.sim._plan_tickets for m in sliced):
            self._drain_plans(wait=True)
        for m in sliced:
            done, m._view.plans_done = m._view.plans_done, []
            for r in done:
                del self._plan_owner[r["ticket"]]
            m.sim._take_plans(done)
        ids, paths, means, per = [], [], [], []
        for m in active:
            mine, p, mu = m.sim._gather_plans()
            if mine:
                ids += [m._view.ids[r] for r in mine]
                paths += p
                means += mu
                per.append((m, mine))
        if ids:
            self.world.apply_global_paths(ids, paths, np.stack(means), reset_tracking=True, route=True, activate=True)
            for m, mine in per:
                m.sim._plans_applied(mine)

    # -- a tick: the existing tick with the world-wide calls made once ---------------------------------------------------------------
    def tick(self):
        active = [m for m in self.members if not m.retired]
        self._apply_members_plans(active)
        for m in active:          # every member applies its spawns, in member order, and asks for its new robots' plans
            m.sim._spawn()
            m.sim._plan()
        ticking = [m for m in active if m.sim.robots]
        if ticking:
            w, s0 = self.world, ticking[0].sim
            alive = sum(1 for m in ticking for r in m.sim.robots if r["alive"])
            if self._logging and self._log_room and self._log_bound + alive > self._log_room:   # (a robot gives at most one sample per tick)
                dropped, _ = self._drain_tracks()
                if dropped:
                    raise hostlib.MgxError(f"the device's tracker log was full: {dropped} samples were not stored")
            self._log_bound += alive
            if self._clock != self.tick_no:   # (before the first tick that has robots, and behind ticks that had none)
                w.tracks_set_clock(self.tick_no)
                if self._goals:
                    w.goal_areas_set_clock(self.tick_no)
            for m in ticking:
                m.sim._tick_device_before()
            numbers = np.array([m.sim.next_number for m in self.members], dtype=np.uint64)
            # one comms radius per member (a retired member's is its own still: it changes nothing, so nothing is uploaded again)
            radius = np.array([m.sim.comms_radius for m in self.members], dtype=np.float32) if self._per_group_radius else s0.comms_radius
            numbers, stats, fin = w.mission_tick_begin_groups(radius, numbers, despawn_finished=s0.despawn, method=s0.method)
            finished, legs = [[] for _ in self.members], [[] for _ in self.members]
            for wid in fin:
                g, r = self._owner[int(wid)]
                finished[g].append(r)
            # the robots that ended a leg of a global-planner mission in this tick: read once, routed like the completions
            if any(m.sim._has_legs for m in ticking):
                for wid in w.mission_legs_ended():
                    g, r = self._owner[int(wid)]
                    legs[g].append(r)
            antennas = None
            for m in ticking:     # every member makes its own draws from its own stream, in its own robot order
                g = m._view._group
                ant = m.sim._tick_device_between(int(numbers[g]), int(stats[g, 0]), int(stats[g, 1]), finished[g], legs=legs[g])
                if ant is not None:
                    if antennas is None:
                        antennas = np.ones(len(self._owner), dtype=np.uint8)
                    antennas[m._view.ids] = ant
            for m in ticking:     # the next legs' requests, under their members' groups: ahead of this tick's planner slice
                m.sim._plan()
            w.mission_tick_end(self._tick_steps(s0), float(s0.max_speed), float(s0.dt32), antennas=antennas)
            self._clock = self.tick_no + 1
        for m in active:
            m.sim.tick_no += 1
        self.tick_no += 1

    def _tick_steps(self, s0):
        """the tick's schedule: one per member where the world takes that and the members differ in it — a retired member's group
        holds no robot any more and gets an empty range — packed once for as long as nobody retires; else the one schedule"""
        if not self._per_group_steps:
            return s0.steps
        retired = tuple(m.retired for m in self.members)
        if retired != self._steps_for:
            per = [[] if m.retired else list(m.sim.steps) for m in self.members]
            live = [s for s in per if s]
            self._steps = live[0] if all(s == live[0] for s in live) else group_steps(per)
            self._steps_for = retired
        return self._steps

    def _retire(self, m):
        """the member's run is over: trackers flushed, export and metrics frozen, its remaining robots out of the world"""
        m.sim._flush_trackers(synchronise=True)
        m.sim._tracks()
        m._export, m._metrics = m.sim.export(), m.sim.metrics()
        m.retired = True
        for t in list(m.sim._plan_tickets):   # (its requests are never handed out: ended or not, their slots are free again)
            m._view.plan_cancel(t)
        m.sim._plan_tickets.clear()
        for r in m.sim.robots:
            if r["alive"]:
                self.world.remove_robot(m._view.ids[r["id"]])

    def run(self, max_ticks=None, max_time=None):
        """until every member is retired: its mission finished (Simulation.finished), its max-time (the scenario's own, or
        max_time) reached, or max_ticks ticks made — the bounds of Simulation.run, per member"""
        def over(m):
            limit = m.sim.cfg["simulation"]["max-time"] if max_time is None else max_time
            return m.sim.finished() or not m.sim.elapsed() < limit or (max_ticks is not None and m.sim.tick_no >= max_ticks)
        while True:
            for m in self.members:
                if not m.retired and over(m):
                    self._retire(m)
            if all(m.retired for m in self.members):
                return self
            self.tick()
