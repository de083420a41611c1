"""Host-side mirror of the reference's FactorGraph API over the C ABI (include/mgx.h).

``World`` owns every robot's factor graph on the device; the method names follow
crates/magics/src/factorgraph/factorgraph.rs and crates/magics/src/planner/robot.rs
(``internal_factor_iteration``, ``change_prior`` ...).  ``FactorGraph`` is the per-robot
handle a reference user would hold (a Bevy component there, ``(world, robot_id)`` here).
"""
import collections
import ctypes as C

import numpy as np

from . import hostlib
from .hostlib import Params, RobotDesc, c_double_p
from .hostlib import check as _check


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def group_radii(radius, n_groups):
    """the comms radius of a per-group call as the engine takes it: None for ONE radius (a scalar: the scalar call), else one f32 per
    group, by group id — ValueError unless there are exactly n_groups of them"""
    if np.ndim(radius) == 0:
        return None
    radii = np.ascontiguousarray(radius, dtype=np.float32)
    if radii.ndim != 1 or len(radii) != n_groups:
        raise ValueError(f"one comms radius per group: got shape {radii.shape} for {n_groups} groups")
    return radii


GroupSteps = collections.namedtuple("GroupSteps", "steps first")   # one schedule per group, packed (group_steps)
_SEQUENCES = (list, tuple, bytes, bytearray, np.ndarray)


def _per_group(steps):
    """the cheap look World.iterate / mission_tick_end take at every call's schedule — it is issued every tick: one schedule per
    group when its first entry is itself a schedule (group_steps then checks all of it), or when it has been packed already"""
    if type(steps) is GroupSteps:
        return steps
    if isinstance(steps, (bytes, bytearray)) or len(steps) == 0 or not isinstance(steps[0], _SEQUENCES):
        return None
    return group_steps(steps)


def group_steps(steps):
    """the schedule of an iterate / mission_tick_end call as the engine takes it: None for ONE schedule (bytes, or a sequence of
    MGX_STEP_* values: the plain call), else one schedule per group, by group id, packed as GroupSteps(steps bytes, first
    [n_groups + 1] u32) for mgx_iterate_groups — group g runs steps[first[g]:first[g + 1]], an empty one sits the call out.
    ValueError for a sequence that mixes the two, or that nests deeper.  A caller that issues the same schedules tick after tick
    packs them once and hands the GroupSteps in."""
    if type(steps) is GroupSteps:
        return steps
    if isinstance(steps, (bytes, bytearray)):
        return None
    items = list(steps)
    def depth(x):   # 0: a step value; 1: a schedule (bytes, or a flat sequence of step values); -1: anything else
        if isinstance(x, (bytes, bytearray)):
            return 1
        if isinstance(x, (list, tuple)):
            return 1 if all(not isinstance(v, (bytes, bytearray, list, tuple)) and np.ndim(v) == 0 for v in x) else -1
        return {0: 0, 1: 1}.get(np.ndim(x), -1)
    depths = [depth(x) for x in items]
    if -1 in depths:
        raise ValueError("one schedule per group: every schedule is a flat sequence of step values")
    if 1 not in depths:
        return None
    if 0 in depths:
        raise ValueError("one schedule per group: got step values and schedules in one sequence")
    packed = [bytes(x) if isinstance(x, (bytes, bytearray)) else bytes(bytearray(int(v) for v in x)) for x in items]
    first = np.zeros(len(packed) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(b) for b in packed], dtype=np.uint64)
    return GroupSteps(b"".join(packed), first)


def make_params(p):
    return Params(
        float(p["sigma_dynamics"]), float(p["sigma_interrobot"]), float(p["sigma_obstacle"]),
        float(p["sigma_tracking"]), float(p["safety_multiplier"]),
        float(p.get("tracking_switch_padding", 1.0)), float(p.get("tracking_attraction_distance", 2.0)),
        int(p.get("enable_mask", 7)), 0)


class World:
    def _chk(self, rc):
        return _check(rc, self._L)

    def __init__(self, params, stream=None, fma=None):
        self._L = hostlib.lib(fma)
        self._p = make_params(params)
        h = C.c_void_p()
        self._chk(self._L.mgx_world_create(C.byref(self._p), C.byref(h)))
        self._w = h
        self._next_key = 0
        self._n_ids = 0  # robot ids handed out so far (ghosts and removed robots included)
        self._args = {}  # array arguments seen before: id -> (the array, its address), see _arg
        self.stream_handle = 0  # raw HIP stream every launch of this world goes to (0: the default stream)
        if stream is not None:
            self.set_stream(stream)

    # -- lifecycle -----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_w", None):
            self._L.mgx_world_destroy(self._w)
            self._w = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """``stream``: raw hipStream_t value (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        self._chk(self._L.mgx_set_stream(self._w, C.c_void_p(int(stream))))
        self.stream_handle = int(stream)

    def synchronize(self):
        self._chk(self._L.mgx_synchronize(self._w))

    def flush(self):
        """everything issued so far is enqueued: a batch is submitted, a lingering launch told to end — no wait (mgx_flush)"""
        self._chk(self._L.mgx_flush(self._w))

    def set_linger(self, microseconds):
        """how long a resident launch waits for the next schedule before it ends (0: never; None: the default) — mgx_set_linger"""
        self._chk(self._L.mgx_set_linger(self._w, -1 if microseconds is None else int(microseconds)))

    def linger_stats(self):
        """(launches that lingered, schedules posted into them, posts taken back and re-run, launches that ended by themselves)"""
        v = [C.c_uint64() for _ in range(4)]
        self._chk(self._L.mgx_linger_stats(self._w, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def set_post_merge(self, mode):
        """back-to-back schedules merged into one post: 0 off, 1 while the launch is behind (default), 2 whenever they fit
        (None: the default) — mgx_set_post_merge"""
        self._chk(self._L.mgx_set_post_merge(self._w, -1 if mode is None else int(mode)))

    def post_merge_stats(self):
        """(plans posted into lingering launches, schedules in them, schedules in the largest) — mgx_post_merge_stats"""
        v = [C.c_uint64() for _ in range(3)]
        self._chk(self._L.mgx_post_merge_stats(self._w, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # -- topology --------------------------------------------------------------------------
    def set_sdf(self, rgb, world_w, world_h):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must be HxWx3 u8")
        h, w, _ = rgb.shape
        self._chk(self._L.mgx_world_set_sdf(self._w, rgb.ctypes.data, w, h, float(world_w), float(world_h)))

    def set_environment(self, env):
        """simulation_loader.rs:154-162 + robot.rs:1259-1264: rasterise + blur the environment on the
        device with its own sdf settings and use the result as the obstacle image."""
        from .environment import _Desc
        d = _Desc(env)
        self._chk(self._L.mgx_world_set_environment(self._w, C.byref(d.desc)))

    def add_robot(self, mean0, prior_diag, dt, radius, path=None, order_key=None, ghost=False, group=0):
        """group: the independent run the robot belongs to (include/mgx.h, ROBOT GROUPS); 0: an ungrouped world's one run."""
        mean0 = _f64(mean0)
        K = mean0.shape[0]
        prior_diag = _f64(prior_diag, (K,))
        dt = _f64(dt, (K - 1,))
        d = RobotDesc()
        d.K = K
        d.mean0, d.prior_diag, d.dt = _dp(mean0), _dp(prior_diag), _dp(dt)
        d.radius = float(radius)
        if path is not None:
            path = np.ascontiguousarray(path, dtype=np.float32)
            d.n_path = path.shape[0]
            d.path_xy = path.ctypes.data_as(C.POINTER(C.c_float))
        if order_key is None:
            order_key = self._next_key
        self._next_key = max(self._next_key, int(order_key) + 1)
        d.order_key = int(order_key)
        d.ghost = 1 if ghost else 0
        if not 0 <= int(group) < 2 ** 32:
            raise ValueError("group must be a non-negative 32-bit number")
        d.group = int(group)
        rid = C.c_int32(-1)
        self._chk(self._L.mgx_robot_add(self._w, C.byref(d), C.byref(rid)))
        self._n_ids = max(self._n_ids, rid.value + 1)
        return rid.value

    def ir_connect(self, owner, other, first_robot_number):
        self._chk(self._L.mgx_ir_connect(self._w, owner, other, int(first_robot_number)))

    def remove_robot(self, robot):
        """Entity despawn (robot.rs:2172): the robot leaves every query for good."""
        self._chk(self._L.mgx_robot_remove(self._w, robot))

    def ir_disconnect(self, a, b):
        self._chk(self._L.mgx_ir_disconnect(self._w, a, b))

    def set_enabled(self, mask):
        """change_factor_enabled for every graph (factorgraph.rs:1529-1539): MGX_FACTOR_* bits."""
        self._chk(self._L.mgx_set_enabled(self._w, int(mask)))

    def set_safety_multiplier(self, multiplier):
        """update_inter_robot_safety_distance_multiplier for every graph and for factors created from now on
        (factorgraph.rs:892-910, ui/settings.rs:586-590): applied on the device, in place."""
        self._chk(self._L.mgx_set_safety_multiplier(self._w, float(multiplier)))

    def set_antenna(self, robot, active):
        self._chk(self._L.mgx_set_antenna(self._w, robot, int(bool(active))))

    def set_idle(self, robot, idle):
        self._chk(self._L.mgx_set_idle(self._w, robot, int(bool(idle))))

    def idle_flags(self):
        """the idle flag of every robot [n] bool, as the world holds them (mgx_get_idle)"""
        n, _ = self.num_robots()
        out, v = np.zeros(n, dtype=bool), C.c_int32()
        for r in range(n):
            self._chk(self._L.mgx_get_idle(self._w, r, C.byref(v)))
            out[r] = bool(v.value)
        return out

    def set_antennas(self, robots, active):
        """update_failed_comms (robot.rs:1593-1601): one write per antenna per tick."""
        robots = np.ascontiguousarray(robots, dtype=np.int32)
        active = np.ascontiguousarray(active, dtype=np.uint8)
        assert robots.shape == active.shape
        self._chk(self._L.mgx_set_antennas(self._w, robots.size, robots.ctypes.data, active.ctypes.data))

    # -- dynamic inter-robot topology (robot.rs:1362-1586) --------------------------------------
    def neighbours(self, positions, radius, method=hostlib.NEIGHBOURS_AUTO, capacity=None):
        """update_robot_neighbours: CSR (row_ptr, neighbours) of robots_within_comms_range.  capacity: ONE search into a buffer
        of that many entries (an error if the rows need more) instead of a sizing search and a second one."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        ptr = np.zeros(pos.shape[0] + 1, dtype=np.int32)
        need = C.c_uint64()
        if capacity is not None:
            idx = np.zeros(max(int(capacity), 1), dtype=np.int32)
            self._chk(self._L.mgx_neighbours(self._w, pos.ctypes.data, float(radius), method, ptr.ctypes.data, idx.ctypes.data,
                                             int(capacity), C.byref(need)))
            return ptr, idx[:need.value]
        self._chk(self._L.mgx_neighbours(self._w, pos.ctypes.data, float(radius), method, ptr.ctypes.data, None, 0, C.byref(need)))
        idx = np.zeros(max(need.value, 1), dtype=np.int32)
        self._chk(self._L.mgx_neighbours(self._w, pos.ctypes.data, float(radius), method, ptr.ctypes.data, idx.ctypes.data,
                                         need.value, C.byref(need)))
        return ptr, idx[:need.value]

    def neighbours_groups(self, positions, radii, method=hostlib.NEIGHBOURS_AUTO, capacity=None):
        """neighbours with one comms radius per group (mgx_neighbours_groups): radii [n_groups], by group id."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        rad = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        ptr = np.zeros(pos.shape[0] + 1, dtype=np.int32)
        need = C.c_uint64()
        if capacity is None:
            self._chk(self._L.mgx_neighbours_groups(self._w, pos.ctypes.data, rad.ctypes.data, len(rad), method, ptr.ctypes.data, None, 0, C.byref(need)))
            capacity = need.value
        idx = np.zeros(max(int(capacity), 1), dtype=np.int32)
        self._chk(self._L.mgx_neighbours_groups(self._w, pos.ctypes.data, rad.ctypes.data, len(rad), method, ptr.ctypes.data, idx.ctypes.data,
                                                int(capacity), C.byref(need)))
        return ptr, idx[:need.value]

    def update_topology(self, positions, radius, next_number, method=hostlib.NEIGHBOURS_AUTO):
        """update_robot_neighbours + delete_/create_interrobot_factors; returns (next robot number,
        connections created, pairs deleted)."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nxt = C.c_uint64(int(next_number))
        stats = (C.c_uint32 * 2)()
        self._chk(self._L.mgx_update_topology(self._w, pos.ctypes.data, float(radius), method, C.byref(nxt), stats))
        return nxt.value, stats[0], stats[1]

    def update_topology_groups(self, positions, radius, next_numbers, method=hostlib.NEIGHBOURS_AUTO):
        """update_topology with one RobotNumberGenerator per group (mgx_update_topology_groups): next_numbers [n_groups].
        radius: one for all groups, or one per group [n_groups] (mgx_update_topology_groups_radii).
        Returns (next robot numbers [n_groups] u64, stats [n_groups, 2] u32: connections created, pairs deleted)."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nxt = None if next_numbers is None else np.array(next_numbers, dtype=np.uint64).reshape(-1)
        n_groups = 0 if nxt is None else len(nxt)
        stats = np.zeros((max(n_groups, 1), 2), dtype=np.uint32)
        radii = group_radii(radius, n_groups)
        if radii is None:
            self._chk(self._L.mgx_update_topology_groups(self._w, pos.ctypes.data, float(radius), int(method), n_groups,
                                                         None if nxt is None else nxt.ctypes.data, stats.ctypes.data))
        else:
            self._chk(self._L.mgx_update_topology_groups_radii(self._w, pos.ctypes.data, radii.ctypes.data, int(method), n_groups,
                                                               None if nxt is None else nxt.ctypes.data, stats.ctypes.data))
        return nxt, stats[:n_groups]

    def connections(self, robot):
        n = C.c_uint32()
        self._chk(self._L.mgx_connections(self._w, robot, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        self._chk(self._L.mgx_connections(self._w, robot, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value].tolist()

    # -- hot path ----------------------------------------------------------------------------
    def iterate(self, steps):
        """steps: one schedule, or one schedule per robot group (group_steps above: mgx_iterate_groups)"""
        per_group = _per_group(steps)
        if per_group is not None:
            b, first = per_group
            self._chk(self._L.mgx_iterate_groups(self._w, len(first) - 1, b, first.ctypes.data))
            return
        # (a tick's schedule is issued over and over: its byte string is made once — building it costs more host time than the call)
        key = steps if isinstance(steps, (bytes, tuple)) else tuple(steps)
        b = _STEP_BYTES.get(key)
        if b is None:
            if len(_STEP_BYTES) > 256:
                _STEP_BYTES.clear()
            b = _STEP_BYTES[key] = bytes(bytearray(int(s) for s in steps))
        self._chk(self._L.mgx_iterate(self._w, b, len(b)))

    def batch_begin(self):
        self._chk(self._L.mgx_batch_begin(self._w))

    def batch_end(self):
        """-> (schedules recorded since batch_begin, sweep-kernel launches they were submitted as)"""
        ns, nl = C.c_uint32(), C.c_uint32()
        self._chk(self._L.mgx_batch_end(self._w, C.byref(ns), C.byref(nl)))
        return ns.value, nl.value

    def batch(self):
        """`with world.batch(): for ...: world.iterate(steps)` — the schedules are submitted together, merged into as few
        resident launches as their segments fit (include/mgx.h: mgx_batch_begin); same results, bit for bit"""
        return _Batch(self)

    def sweep(self, external_phases, internal_phases, n_internal=1, robot=-1, hints=0):
        self._chk(self._L.mgx_sweep(self._w, robot, external_phases, internal_phases, n_internal, hints))

    def internal_factor_iteration(self, robot=-1):
        self._chk(self._L.mgx_internal_factor_iteration(self._w, robot))

    def internal_variable_iteration(self, robot=-1):
        self._chk(self._L.mgx_internal_variable_iteration(self._w, robot))

    def external_factor_iteration(self, robot=-1):
        self._chk(self._L.mgx_external_factor_iteration(self._w, robot))

    def external_variable_iteration(self, robot=-1):
        self._chk(self._L.mgx_external_variable_iteration(self._w, robot))

    def change_prior(self, robot, var_ix, mean):
        mean = _f64(mean, (4,))
        self._chk(self._L.mgx_change_prior(self._w, robot, var_ix, _dp(mean)))

    def reset_variables(self, robot, means, first_last_sigma=1e30, inbetween_sigma=float("inf")):
        """FactorGraph::reset_variables (factorgraph.rs:1541-1564); the defaults are the reference's call (robot.rs:768)."""
        m = _f64(means).reshape(-1, 4)
        self._chk(self._L.mgx_reset_variables(self._w, robot, _dp(m), len(m), float(first_last_sigma), float(inbetween_sigma)))

    def reset_tracking_factors(self, robot):
        """FactorGraph::reset_tracking_factors (factorgraph.rs:1566-1590)."""
        self._chk(self._L.mgx_reset_tracking_factors(self._w, robot))

    def set_tracking_path(self, robot, path):
        """modify_tracking_factors(|t| t.set_tracking_path(path)) (factorgraph.rs:1467, tracking.rs:134-136, robot.rs:674-682):
        the robot's tracking factors follow `path` ([n >= 2][2]) and keep their records and timeouts."""
        path = np.ascontiguousarray(path, dtype=np.float32).reshape(-1, 2)
        self._chk(self._L.mgx_set_tracking_path(self._w, robot, path.ctypes.data, path.shape[0]))

    def apply_global_paths(self, robots, paths, means, first_last_sigma=1e30, inbetween_sigma=float("inf"), reset_tracking=True,
                           route=False, activate=False):
        """The path-finding completion handler (robot.rs:643-799) for a batch of robots in one call (mgx_apply_global_paths):
        set_tracking_path, reset_variables, reset_tracking_factors and — on request — the device mission's new route (`route`:
        paths[i][1:]) and mission.state = Active (`activate`: idle off).  paths: one [n_i >= 2][2] polyline per robot; means:
        [len(robots)][K][4].  Applied in place on the device when the world is laid out, unsharded and has never switched a
        factor kind at run time; otherwise the per-robot calls run internally."""
        robots = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        if len(paths) != robots.size:
            raise ValueError(f"{robots.size} robots, {len(paths)} paths")
        paths = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2) for p in paths]
        ptr = np.zeros(robots.size + 1, dtype=np.uint32)
        ptr[1:] = np.cumsum([p.shape[0] for p in paths])
        xy = np.ascontiguousarray(np.concatenate(paths, axis=0)) if paths else np.zeros((1, 2), dtype=np.float32)
        m = _f64(means).reshape(robots.size, -1, 4) if robots.size else np.zeros((1, 1, 4))
        flags = ((hostlib.GLOBAL_PATH_RESET_TRACKING if reset_tracking else 0) | (hostlib.GLOBAL_PATH_ROUTE if route else 0)
                 | (hostlib.GLOBAL_PATH_ACTIVATE if activate else 0))
        self._chk(self._L.mgx_apply_global_paths(self._w, robots.size, robots.ctypes.data, ptr.ctypes.data, xy.ctypes.data, m.ctypes.data,
                                                 float(first_last_sigma), float(inbetween_sigma), flags))

    def layout_stats(self):
        """-> (full rebuilds of the device arrays from the host mirror, downloads of the device state into it) — mgx_layout_stats"""
        nl, npl = C.c_uint64(), C.c_uint64()
        self._chk(self._L.mgx_layout_stats(self._w, C.byref(nl), C.byref(npl)))
        return int(nl.value), int(npl.value)

    def reserve(self, robots):
        """The world expects to hold up to `robots` robots (removed ones included): robots added to the laid-out world are then
        appended on the device — nothing pulled, nothing laid out again — for as long as they fit (mgx_world_reserve)."""
        self._chk(self._L.mgx_world_reserve(self._w, int(robots)))

    def append_stats(self):
        """-> (commits that appended in place, robots they brought onto the device, commits of the reserved world that had new
        robots and ran the full layout all the same) — mgx_append_stats"""
        a, r, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._L.mgx_append_stats(self._w, C.byref(a), C.byref(r), C.byref(f)))
        return int(a.value), int(r.value), int(f.value)

    def change_priors(self, robots, var_ix, means):
        robots = np.ascontiguousarray(robots, dtype=np.int32)
        var_ix = np.ascontiguousarray(var_ix, dtype=np.uint32)
        means = _f64(means, (len(robots), 4))
        self._chk(self._L.mgx_change_priors(self._w, len(robots), robots.ctypes.data_as(C.POINTER(C.c_int32)),
                                        var_ix.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(means)))

    def update_priors(self, robots, waypoints_xy, time_scale, what, max_speed, delta_t):
        """update_prior_of_horizon_state (what & 1) / update_prior_of_current_state_v3 (what & 2) for the
        listed robots (robot.rs:2182-2338)."""
        robots = np.ascontiguousarray(robots, dtype=np.int32)
        n = len(robots)
        wp = _f64(waypoints_xy, (n, 2))
        ts = _f64(time_scale, (n,))
        what = np.ascontiguousarray(what, dtype=np.uint8)
        if what.shape != (n,):
            raise ValueError(f"expected shape {(n,)}, got {what.shape}")
        self._chk(self._L.mgx_update_priors(self._w, n, robots.ctypes.data_as(C.POINTER(C.c_int32)), _dp(wp), _dp(ts),
                                            what.ctypes.data_as(C.POINTER(C.c_uint8)), float(max_speed), float(delta_t)))

    def _arg(self, a, dtype, shape=None):
        """(keep-alive, address) of an array argument.  A driver hands the same arrays tick after tick: an array that is already
        what the C side reads (dtype, C-contiguous) is remembered with its address — preparing four pointers costs more host
        time than the call they go into (15 us of a 130 us tick).  The shape is checked on every call, remembered or not: the
        same array may come with a different number of robots (or have been reshaped in place)."""
        e = self._args.get(id(a))
        if e is None or e[0] is not a:
            b = np.ascontiguousarray(a, dtype=dtype)
            e = (b, b.ctypes.data)
            if b is a:  # (held here: its id cannot be handed to another object, its buffer cannot be resized)
                if len(self._args) >= 16:
                    self._args.pop(next(iter(self._args)))
                self._args[id(a)] = e
        if shape is not None and e[0].shape != shape:
            raise ValueError(f"expected shape {shape}, got {e[0].shape}")
        return e

    def tick(self, robots, waypoints_xy, time_scale, what, max_speed, delta_t, steps):
        """One FixedUpdate tick of the planner chain (robot.rs:86-103): the prior updates of `update_priors`
        for the listed robots, then `iterate(steps)` — one C call (mgx_tick)."""
        r = self._arg(robots, np.int32)
        n = len(r[0])
        wp = self._arg(waypoints_xy, np.float64, (n, 2))
        ts = self._arg(time_scale, np.float64, (n,))
        wh = self._arg(what, np.uint8, (n,))
        key = steps if isinstance(steps, (bytes, tuple)) else tuple(steps)
        b = _STEP_BYTES.get(key)
        if b is None:
            if len(_STEP_BYTES) > 256:
                _STEP_BYTES.clear()
            b = _STEP_BYTES[key] = bytes(bytearray(int(s) for s in steps))
        self._chk(self._L.mgx_tick(self._w, n, r[1], wp[1], ts[1], wh[1], float(max_speed), float(delta_t), b, len(b)))

    # -- read-back -----------------------------------------------------------------------------
    def get_belief(self, robot, var_ix):
        eta, lam, mean, cov = np.zeros(4), np.zeros((4, 4)), np.zeros(4), np.zeros((4, 4))
        valid = C.c_int32()
        self._chk(self._L.mgx_get_belief(self._w, robot, var_ix, _dp(eta), _dp(lam), _dp(mean), _dp(cov), C.byref(valid)))
        return {"eta": eta, "lam": lam, "mean": mean, "cov": cov, "valid": bool(valid.value)}

    def num_robots(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self._L.mgx_num_robots(self._w, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- whole driver ticks on the device (include/mgx.h, mgx_mission_*) ---------------------------------------------
    def mission_set(self, robot, waypoints_xy, reach_var, finish_var, reach_dist2, finish_dist2, translation, time_scale, legs_after=0):
        """legs_after: further legs that follow this route (include/mgx.h, MISSIONS OF SEVERAL LEGS); 0: the route is the mission"""
        wp = _f64(waypoints_xy).reshape(-1, 2)
        if int(legs_after) < 0:
            raise ValueError("legs_after: a count of legs")
        d = hostlib.MissionDesc(len(wp), int(legs_after), _dp(wp), int(reach_var), int(finish_var), float(reach_dist2), float(finish_dist2),
                                (C.c_float * 3)(*[float(x) for x in translation]), 0.0, float(time_scale))
        self._chk(self._L.mgx_mission_set(self._w, int(robot), C.byref(d)))

    def mission_tick(self, comms_radius, next_number, steps, max_speed, delta_t, despawn_finished=True, antennas=None,
                     method=hostlib.NEIGHBOURS_AUTO):
        """One FixedUpdate of the planner chain with the mission state on the device.  Returns
        (next robot number, connections created, pairs deleted, missions completed this tick)."""
        nn, st = C.c_uint64(int(next_number)), (C.c_uint32 * 3)()
        ant = None
        if antennas is not None:
            ant = np.ascontiguousarray(antennas, dtype=np.uint8)
        self._chk(self._L.mgx_mission_tick(self._w, float(comms_radius), int(method), C.byref(nn), 1 if despawn_finished else 0,
                                           None if ant is None else ant.ctypes.data, float(max_speed), float(delta_t),
                                           bytes(bytearray(steps)), len(steps), st))
        return nn.value, st[0], st[1], st[2]

    def mission_tick_begin(self, comms_radius, next_number, despawn_finished=True, method=hostlib.NEIGHBOURS_AUTO):
        """reached_waypoint + the topology pass (the tick's one synchronisation).  Returns (next robot number, connections
        created, pairs deleted, ids of the robots whose mission completed in this tick)."""
        nn, st = C.c_uint64(int(next_number)), (C.c_uint32 * 3)()
        self._chk(self._L.mgx_mission_tick_begin(self._w, float(comms_radius), int(method), C.byref(nn), 1 if despawn_finished else 0, st))
        fin = np.zeros(st[2], dtype=np.int32)
        if st[2]:
            k = C.c_uint32()
            self._chk(self._L.mgx_mission_finished(self._w, fin.ctypes.data, st[2], C.byref(k)))
        return nn.value, st[0], st[1], fin

    def mission_tick_begin_groups(self, comms_radius, next_numbers, despawn_finished=True, method=hostlib.NEIGHBOURS_AUTO):
        """mission_tick_begin with one RobotNumberGenerator per group (mgx_mission_tick_begin_groups): next_numbers [n_groups].
        comms_radius: one for all groups, or one per group [n_groups] (mgx_mission_tick_begin_groups_radii).
        Returns (next robot numbers [n_groups] u64, stats [n_groups, 3] u32: connections created, pairs deleted, missions
        completed, ids of the robots of all groups whose mission completed in this tick, ascending)."""
        nxt = None if next_numbers is None else np.array(next_numbers, dtype=np.uint64).reshape(-1)
        n_groups = 0 if nxt is None else len(nxt)
        stats = np.zeros((max(n_groups, 1), 3), dtype=np.uint32)
        radii = group_radii(comms_radius, n_groups)
        if radii is None:
            self._chk(self._L.mgx_mission_tick_begin_groups(self._w, float(comms_radius), int(method), n_groups,
                                                            None if nxt is None else nxt.ctypes.data, 1 if despawn_finished else 0, stats.ctypes.data))
        else:
            self._chk(self._L.mgx_mission_tick_begin_groups_radii(self._w, radii.ctypes.data, int(method), n_groups,
                                                                  None if nxt is None else nxt.ctypes.data, 1 if despawn_finished else 0,
                                                                  stats.ctypes.data))
        n_fin = int(stats[:n_groups, 2].sum())
        fin = np.zeros(n_fin, dtype=np.int32)
        if n_fin:
            k = C.c_uint32()
            self._chk(self._L.mgx_mission_finished(self._w, fin.ctypes.data, n_fin, C.byref(k)))
        return nxt, stats[:n_groups], fin

    def mission_finished(self):
        """ids of the robots whose mission completed in the last mission_tick_begin (any form), ascending (mgx_mission_finished)"""
        k = C.c_uint32()
        self._chk(self._L.mgx_mission_finished(self._w, None, 0, C.byref(k)))
        out = np.zeros(k.value, dtype=np.int32)
        if k.value:
            self._chk(self._L.mgx_mission_finished(self._w, out.ctypes.data, k.value, C.byref(k)))
        return out

    def mission_legs_ended(self):
        """ids of the robots that ended a leg with legs left in the last mission_tick_begin (any form), ascending: idle since, waiting
        for apply_global_paths(route=True, activate=True) (mgx_mission_legs_ended)"""
        k = C.c_uint32()
        self._chk(self._L.mgx_mission_legs_ended(self._w, None, 0, C.byref(k)))
        out = np.zeros(k.value, dtype=np.int32)
        if k.value:
            self._chk(self._L.mgx_mission_legs_ended(self._w, out.ctypes.data, k.value, C.byref(k)))
        return out

    def mission_legs_read(self):
        """legs left per robot as the device has counted them down [n] int32 (mgx_mission_legs_read; synchronises)"""
        n, _ = self.num_robots()
        out = np.zeros(n, np.int32)
        self._chk(self._L.mgx_mission_legs_read(self._w, out.ctypes.data))
        return out

    def mission_tick_end(self, steps, max_speed, delta_t, antennas=None):
        """steps: one schedule, or one schedule per robot group (group_steps above: mgx_mission_tick_end_groups)"""
        ant = None if antennas is None else np.ascontiguousarray(antennas, dtype=np.uint8)
        per_group = _per_group(steps)
        if per_group is not None:
            b, first = per_group
            self._chk(self._L.mgx_mission_tick_end_groups(self._w, None if ant is None else ant.ctypes.data, float(max_speed), float(delta_t),
                                                          len(first) - 1, b, first.ctypes.data))
            return
        self._chk(self._L.mgx_mission_tick_end(self._w, None if ant is None else ant.ctypes.data, float(max_speed), float(delta_t),
                                               bytes(bytearray(steps)), len(steps)))

    def mission_run(self, n_ticks, comms_radius, next_number, steps, max_speed, delta_t, despawn_finished=True, method=hostlib.NEIGHBOURS_AUTO,
                    failure_rate=0.0, wyrand_state=None, stop_when_all_finished=False, want_translations=True, want_antennas=False):
        """Up to n_ticks whole driver ticks in ONE call (mgx_mission_run): per tick what mission_tick_begin / _end would have
        given.  Returns dict(ticks, next_number, wyrand_state, created [t], deleted [t], finished (list of id arrays per tick),
        legs_ended (likewise: the call returns behind the first tick in which a robot ended a leg, so only the last may hold any),
        translations [t, n, 3] f32, antennas [t, n] u8)."""
        n, _ = self.num_robots()
        T = int(n_ticks)
        d = hostlib.MissionRunDesc()
        created, deleted, nfin = (np.zeros(T, np.uint32) for _ in range(3))
        fin = np.zeros(max(n, 1), np.int32)
        tr = np.zeros((T, n, 3), np.float32) if want_translations else None
        ant = np.zeros((T, n), np.uint8) if want_antennas else None
        nn, ws = C.c_uint64(int(next_number)), C.c_uint64(0 if wyrand_state is None else int(wyrand_state))
        sb = bytes(bytearray(int(x) for x in steps))
        d.n_ticks, d.comms_radius, d.method, d.despawn_finished = T, float(comms_radius), int(method), 1 if despawn_finished else 0
        d.stop_when_all_finished, d.n_steps, d.steps = (1 if stop_when_all_finished else 0), len(sb), sb
        d.max_speed, d.delta_t, d.failure_rate = float(max_speed), float(delta_t), float(failure_rate)
        d.wyrand_state = None if wyrand_state is None else C.pointer(ws)
        d.robot_number_next = C.pointer(nn)
        u32p = C.POINTER(C.c_uint32)
        d.created, d.deleted, d.n_finished = created.ctypes.data_as(u32p), deleted.ctypes.data_as(u32p), nfin.ctypes.data_as(u32p)
        d.finished, d.finished_capacity = fin.ctypes.data_as(C.POINTER(C.c_int32)), len(fin)
        d.translations = None if tr is None else tr.ctypes.data_as(C.POINTER(C.c_float))
        d.antennas = None if ant is None else ant.ctypes.data_as(C.POINTER(C.c_uint8))
        self._chk(self._L.mgx_mission_run(self._w, C.addressof(d)))
        t = int(d.ticks_done)
        cuts = np.concatenate([[0], np.cumsum(nfin[:t])]).astype(int)
        return dict(ticks=t, next_number=int(nn.value), wyrand_state=None if wyrand_state is None else int(ws.value), created=created[:t],
                    deleted=deleted[:t], finished=[fin[cuts[i]:cuts[i + 1]].copy() for i in range(t)],
                    # (an older build named by MGX_LIB knows no legs: nobody ever ends one there)
                    legs_ended=[np.zeros(0, np.int32) for _ in range(t - 1)] +
                               ([self.mission_legs_ended() if hasattr(self._L, "mgx_mission_legs_ended") else np.zeros(0, np.int32)] if t else []),
                    translations=None if tr is None else tr[:t], antennas=None if ant is None else ant[:t])

    def mission_translations(self):
        """Transforms [n, 3] as of the end of the last tick; valid once the stream has been synchronised since (no sync here)."""
        n, _ = self.num_robots()
        out, k = np.zeros((n, 3), np.float32), C.c_uint32()
        self._chk(self._L.mgx_mission_translations(self._w, out.ctypes.data, n, C.byref(k)))
        return out[:min(n, k.value)]

    def mission_read(self):
        """(Transform translations [n, 3] f32, next waypoint index per robot, completion tick per robot)"""
        n, _ = self.num_robots()
        tr, tg, fin = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        self._chk(self._L.mgx_mission_read(self._w, tr.ctypes.data, tg.ctypes.data, fin.ctypes.data))
        return tr, tg, fin

    # -- collision bookkeeping on the device (include/mgx.h): robot-robot (mgx_collisions_*), robot-environment (mgx_env_collisions_*)
    def _contacts_update(self, update, positions):
        pos = None if positions is None else np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        if pos is not None and len(pos) != self.num_robots()[0]:
            raise ValueError("one position per robot of the world")
        self._chk(update(self._w, None if pos is None else pos.ctypes.data))

    def _contacts_read(self, read, dtype, first, strict=True):
        """two calls: how many events there are, then the events from `first` on.  A status may come with every output filled."""
        n, first = self.num_robots()[0], int(first)
        tot, drop = C.c_uint64(), C.c_uint64()
        per = np.zeros(n, np.uint32)
        ev = np.zeros(0, dtype)
        rc = read(self._w, first, None, 0, C.byref(tot), C.byref(drop), per.ctypes.data)
        if tot.value > first:
            ev = np.zeros(tot.value - first, dtype)
            rc = read(self._w, first, ev.ctypes.data, len(ev), C.byref(tot), C.byref(drop), per.ctypes.data)
            ev = ev[:max(0, min(len(ev), tot.value - first))]
        if strict:
            self._chk(rc)
            return ev, int(tot.value), int(drop.value), per
        return ev, int(tot.value), int(drop.value), per, rc

    def collisions_enable(self, enabled=True, method=hostlib.NEIGHBOURS_AUTO, event_capacity=0):
        """while on, every mission tick ends with one pass of update_robot_robot_collisions on the device (no synchronisation)"""
        self._chk(self._L.mgx_collisions_enable(self._w, 1 if enabled else 0, int(method), int(event_capacity)))

    def collisions_update(self, positions=None):
        """one pass over the caller's Transforms [n, 3] f32 (None: the device's mission Transforms); enqueued, not waited for"""
        self._contacts_update(self._L.mgx_collisions_update, positions)

    def collisions_read(self, first=0):
        """(events from `first` on in (pass, robot_a, robot_b) order — a structured array with fields pass, robot_a, robot_b,
        mins [2], maxs [2] —, events in the log, events dropped because it was full, contacts per robot).  Synchronises."""
        return self._contacts_read(self._L.mgx_collisions_read, hostlib.collision_event_dtype(), first)

    def collisions_clear(self):
        self._chk(self._L.mgx_collisions_clear(self._w))

    def env_collisions_enable(self, env, event_capacity=0):
        """env: an environment dict — its colliders (hostlib.env_colliders) go to the device once and every mission tick ends with
        one pass of update_robot_environment_collisions (no synchronisation); None: off, the state is dropped"""
        if env is None:
            self._chk(self._L.mgx_env_collisions_enable(self._w, None, 0))
            return
        from .environment import _Desc
        d = _Desc(env)
        self._chk(self._L.mgx_env_collisions_enable(self._w, C.byref(d.desc), int(event_capacity)))

    def env_collisions_update(self, positions=None):
        """one pass over the caller's Transforms [n, 3] f32 (None: the device's mission Transforms); enqueued, not waited for"""
        self._contacts_update(self._L.mgx_env_collisions_update, positions)

    def env_collisions_read(self, first=0, strict=True):
        """(events from `first` on in (pass, robot, collider) order — a structured array with fields pass, robot, collider,
        mins [2], maxs [2] —, events in the log, events dropped because it was full, contacts per robot).  Synchronises.
        strict=False: a status that comes with filled outputs (MGX_ERR_STATE: a robot touched more colliders at once than the
        device remembers) is returned as a fifth element instead of being raised."""
        return self._contacts_read(self._L.mgx_env_collisions_read, hostlib.env_collision_event_dtype(), first, strict)

    def env_collisions_clear(self):
        self._chk(self._L.mgx_env_collisions_clear(self._w))

    # -- goal areas on the device (include/mgx.h, mgx_goal_areas_*): the first arrival of every robot in every area
    def goal_areas_enable(self, areas, next_tick=0):
        """areas: boxes ((x0, z0), (x1, z1)) in world (x, z), corners in either order, at most hostlib.GOAL_AREAS_MAX — while on,
        every mission tick ends with one pass of goal_area::detect_collisions on the device (no synchronisation); None or
        empty: off, the state is dropped"""
        boxes = np.zeros(0 if areas is None else len(areas), hostlib.goal_area_dtype())
        for i in range(len(boxes)):
            boxes[i]["mins"], boxes[i]["maxs"] = areas[i][0], areas[i][1]
        self._chk(self._L.mgx_goal_areas_enable(self._w, boxes.ctypes.data if len(boxes) else None, len(boxes), int(next_tick)))
        self._goal_areas_n = len(boxes)

    _goal_areas_n = 0

    def goal_areas_set_clock(self, next_tick):
        """the simulated tick index of the coming mission tick"""
        self._chk(self._L.mgx_goal_areas_set_clock(self._w, int(next_tick)))

    def goal_areas_update(self, tick, positions=None):
        """one pass at `tick` over the caller's Transforms [n, 3] f32 (None: the device's mission Transforms); does not move the
        clock; enqueued, not waited for"""
        pos = None if positions is None else np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        if pos is not None and len(pos) != self.num_robots()[0]:
            raise ValueError("one position per robot of the world")
        self._chk(self._L.mgx_goal_areas_update(self._w, None if pos is None else pos.ctypes.data, int(tick)))

    def goal_areas_read(self):
        """(arrivals in (tick, robot, area) order — a structured array with fields tick, area, robot —, arrivals per area).
        Synchronises."""
        tot = C.c_uint64()
        per = np.zeros(self._goal_areas_n, np.uint32)
        self._chk(self._L.mgx_goal_areas_read(self._w, None, 0, C.byref(tot), per.ctypes.data if len(per) else None))
        out = np.zeros(tot.value, hostlib.goal_arrival_dtype())
        if tot.value:
            self._chk(self._L.mgx_goal_areas_read(self._w, out.ctypes.data, len(out), C.byref(tot), per.ctypes.data))
        return out[:tot.value], per

    def goal_areas_clear(self):
        """every (area, robot) back to "never"; the areas and the clock stay"""
        self._chk(self._L.mgx_goal_areas_clear(self._w))

    # -- trackers on the device (include/mgx.h, mgx_tracks_*): position / velocity samples and distance travelled
    def tracks_enable(self, enabled=True, period_ns=100_000_000, tick_ns=0, next_tick=0, sample_capacity=0):
        """while on, every mission tick ends with one tracker pass on the device (no synchronisation): a sample of every moving
        robot's Transform every period_ns of simulated time, and the length of its Transform increment added to its distance"""
        self._chk(self._L.mgx_tracks_enable(self._w, 1 if enabled else 0, int(period_ns), int(tick_ns), int(next_tick), int(sample_capacity)))

    def tracks_set_clock(self, next_tick):
        """the simulated tick index of the coming mission tick"""
        self._chk(self._L.mgx_tracks_set_clock(self._w, int(next_tick)))

    def tracks_update(self, tick, positions=None, moved=None):
        """one sampling pass at `tick` over the caller's Transforms [n, 3] f32 (None: the device's mission Transforms) for the robots
        with a non-zero `moved` byte (None: every live robot); adds no distance; enqueued, not waited for"""
        n = self.num_robots()[0]
        pos = None if positions is None else np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        mv = None if moved is None else np.ascontiguousarray(moved, dtype=np.uint8).reshape(-1)
        if (pos is not None and len(pos) != n) or (mv is not None and len(mv) != n):
            raise ValueError("one position and one moved byte per robot of the world")
        self._chk(self._L.mgx_tracks_update(self._w, None if pos is None else pos.ctypes.data, None if mv is None else mv.ctypes.data, int(tick)))

    def tracks_take(self, capacity=None, travelled=True):
        """(samples in (tick, robot) order — a structured array with fields tick, robot, span_ticks, position [3], velocity [3] —,
        samples that were in the log, samples dropped because it was full, distance travelled per robot or None).  Synchronises.
        The log is emptied when it is handed out.  capacity (default: whatever the log holds): with less room than the log needs
        nothing is taken and the samples come back empty."""
        n = self.num_robots()[0]
        dist = np.zeros(n, np.float64) if travelled else None
        took, in_log, drop = C.c_uint64(), C.c_uint64(), C.c_uint64()
        dp = None if dist is None else dist.ctypes.data
        buf = np.zeros(int(capacity) if capacity is not None else self._tracks_room, hostlib.track_sample_dtype())
        self._chk(self._L.mgx_tracks_take(self._w, buf.ctypes.data if len(buf) else None, len(buf), C.byref(took), C.byref(in_log), C.byref(drop), dp))
        if capacity is None and in_log.value > len(buf):  # (nothing was taken: once more with the room the log needs)
            self._tracks_room = int(in_log.value) + int(in_log.value) // 4
            buf = np.zeros(int(in_log.value), hostlib.track_sample_dtype())
            self._chk(self._L.mgx_tracks_take(self._w, buf.ctypes.data, len(buf), C.byref(took), C.byref(in_log), C.byref(drop), dp))
        return buf[:took.value], int(in_log.value), int(drop.value), dist

    _tracks_room = 1024

    def tracks_clear(self):
        self._chk(self._L.mgx_tracks_clear(self._w))

    def tracks_set_logging(self, on=True):
        """off: a sample still moves the timer, the previous sample, the distance and the run metrics, but is not appended to the log"""
        self._chk(self._L.mgx_tracks_set_logging(self._w, 1 if on else 0))

    # -- run metrics on the device (include/mgx.h, mgx_track_metrics_*): dimensionless jerk and path deviation per robot
    def track_metrics_enable(self, enabled=True, max_route_points=0):
        """while on (the trackers must be), every sample a tracker pass takes also feeds the robot's jerk and deviation state"""
        self._chk(self._L.mgx_track_metrics_enable(self._w, 1 if enabled else 0, int(max_route_points)))

    def track_metrics_set_route(self, robot, xy):
        """the polyline [n, 2] f64 the robot's deviation is measured against from the next pass on (None or empty: no route)"""
        pts = np.zeros((0, 2), np.float64) if xy is None else np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._chk(self._L.mgx_track_metrics_set_route(self._w, int(robot), pts.ctypes.data if len(pts) else None, len(pts)))

    def track_metrics_read(self):
        """one record per robot (hostlib.track_metrics_dtype: n_positions, n_velocities, n_unrouted, flags, dimensionless_jerk,
        vmax2, deviation_sum, deviation_max), finalised on a copy of the device's state.  Synchronises."""
        n = self.num_robots()[0]
        out = np.zeros(n, hostlib.track_metrics_dtype())
        self._chk(self._L.mgx_track_metrics_read(self._w, out.ctypes.data if n else None, n))
        return out

    # -- the global planner (include/mgx.h): batched RRT* over the map's colliders
    def planner_enable(self, env, params=None):
        """env: an environment dict — its colliders go to the device; params: a dict as global_planner.params makes it (the fields
        of mgx_plan_params).  env None: off, every allocation is dropped."""
        if env is None:
            self._chk(self._L.mgx_planner_enable(self._w, None, None))
            return
        from .environment import _Desc
        d = _Desc(env)
        p = self._plan_params(params)
        self._chk(self._L.mgx_planner_enable(self._w, C.byref(d.desc), C.byref(p)))

    @staticmethod
    def _plan_params(params):
        """a dict as global_planner.params makes it -> mgx_plan_params"""
        return hostlib.PlanParams(float(params["step_size"]), float(params["neighbourhood_radius"]), float(params["collision_radius"]),
                                  int(params["max_iterations"]), 1 if params.get("smoothing_enabled") else 0,
                                  int(params.get("smoothing_max_iterations", 0)), float(params.get("smoothing_step", 0.0)),
                                  float(params.get("sample_half_extent", 0.0)), int(params.get("max_nodes", 0)),
                                  int(params.get("iterations_per_launch", 0)))

    def planner_set_group_params(self, group, params):
        """from the next submit on, requests of `group` run under `params` (a dict as planner_enable takes it; max_nodes and
        iterations_per_launch absent, 0 or the world's); None: the world's parameters again.  Raises while requests are pending
        (mgx_planner_set_group_params)"""
        p = None if params is None else self._plan_params(params)
        self._chk(self._L.mgx_planner_set_group_params(self._w, int(group), None if p is None else C.addressof(p)))

    def planner_group_params(self, group):
        """what a request of `group` would run under — its own set, or the world's with the defaults filled in — as a dict of the
        fields of mgx_plan_params (mgx_planner_group_params)"""
        p = hostlib.PlanParams()
        self._chk(self._L.mgx_planner_group_params(self._w, int(group), C.addressof(p)))
        out = {name: getattr(p, name) for name, _ in hostlib.PlanParams._fields_}
        out["smoothing_enabled"] = bool(out["smoothing_enabled"])
        return out

    @staticmethod
    def _plan_groups(groups, n):
        """one group per request as the engine reads it; None stays None (group 0 for every request)"""
        if groups is None:
            return None
        g = np.ascontiguousarray(groups, dtype=np.int64)
        if g.shape != (n,):
            raise ValueError("groups: one group per request")
        if n and (g.min() < 0 or g.max() > 0xffffffff):
            raise ValueError("groups: a group index is not a 32-bit count")
        return g.astype(np.uint32)

    def plan_paths_raw(self, requests, point_capacity, groups=None):
        """mgx_plan_paths_groups as it is: requests a structured array (hostlib.plan_request_dtype), groups None or one per request
        -> (status code, results, points [point_capacity, 2] f32, all points); nothing is raised"""
        req = np.ascontiguousarray(requests, dtype=hostlib.plan_request_dtype())
        g = self._plan_groups(groups, len(req))
        res = np.zeros(len(req), hostlib.plan_result_dtype())
        xy = np.full((max(int(point_capacity), 1), 2), np.nan, np.float32)
        total = C.c_uint32(0)
        rc = self._L.mgx_plan_paths_groups(self._w, len(req), req.ctypes.data, None if g is None else g.ctypes.data, res.ctypes.data,
                                           xy.ctypes.data, int(point_capacity), C.byref(total))
        return rc, res, xy[:int(point_capacity)], int(total.value)

    def plan_paths(self, requests, groups=None):
        """requests: [(start (x, y), end (x, y), wyrand_state)] -> one dict per request (status, n_nodes, iterations, cost,
        wyrand_state, path [n, 2] f32 — empty unless the status is hostlib.PLAN_OK), as global_planner.plan_paths gives them.
        groups: one group per request — the parameter set it runs under (planner_set_group_params); None: group 0 for all.
        One call, synchronous (mgx_plan_paths_groups)."""
        req = np.zeros(len(requests), hostlib.plan_request_dtype())
        for i, (s, e, state) in enumerate(requests):
            req["start"][i], req["end"][i], req["wyrand_state"][i] = s, e, int(state)
        room = 256 * max(len(req), 1)
        rc, res, xy, total = self.plan_paths_raw(req, room, groups)
        if rc < 0 and total > room:  # (the counts came back: once more with room for them)
            rc, res, xy, total = self.plan_paths_raw(req, total, groups)
        self._chk(rc)
        return [{"status": int(r["status"]), "n_nodes": int(r["n_nodes"]), "iterations": int(r["iterations"]),
                 "smoothing_iterations": int(r["smoothing_iterations"]), "cost": float(r["cost"]),
                 "wyrand_state": int(r["wyrand_state"]), "path": xy[int(r["first_point"]):int(r["first_point"]) + int(r["n_points"])].copy()}
                for r in res]

    # plans that ride the stream (include/mgx.h): submit returns at once, advance enqueues one slice, collect hands out what ended
    def plan_submit(self, requests, groups=None):
        """requests: [(start (x, y), end (x, y), wyrand_state)] -> their tickets; groups: one group per request, None: group 0 for
        all (mgx_plan_submit_groups: nothing is launched or waited for)"""
        req = np.zeros(len(requests), hostlib.plan_request_dtype())
        for i, (s, e, state) in enumerate(requests):
            req["start"][i], req["end"][i], req["wyrand_state"][i] = s, e, int(state)
        g = self._plan_groups(groups, len(req))
        tickets = np.zeros(len(req), np.uint64)
        self._chk(self._L.mgx_plan_submit_groups(self._w, len(req), req.ctypes.data, None if g is None else g.ctypes.data, tickets.ctypes.data))
        return [int(t) for t in tickets]

    def plan_advance(self, iterations):
        """one slice of at most `iterations` iterations for every pending request, enqueued on the world's stream (mgx_plan_advance)"""
        self._chk(self._L.mgx_plan_advance(self._w, int(iterations)))

    def planner_set_tick_budget(self, iterations):
        """0: off; otherwise every mission tick ends by enqueuing one such slice when requests are pending"""
        self._chk(self._L.mgx_planner_set_tick_budget(self._w, int(iterations)))

    def plan_collect(self, wait=False, capacity=64, point_capacity=None):
        """The requests that have ended, in the order of (slice number, ticket), each once: one dict per request as plan_paths gives
        them, with `ticket`, `slices`, `group` (the one it was submitted under) and `smoothing_iterations` beside.  wait: first wait for the slices enqueued so far
        (MGX_PLAN_WAIT); otherwise the call never blocks.  What does not fit into capacity / point_capacity stays for the next call."""
        capacity = int(capacity)
        room = 256 * max(capacity, 1) if point_capacity is None else int(point_capacity)
        done = np.zeros(max(capacity, 1), hostlib.plan_done_dtype())
        xy = np.full((max(room, 1), 2), np.nan, np.float32)
        nd, npts = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.mgx_plan_collect(self._w, hostlib.PLAN_WAIT if wait else 0, capacity, done.ctypes.data, xy.ctypes.data, room,
                                           C.byref(nd), C.byref(npts)))
        out = []
        for d in done[:nd.value]:
            r = d["result"]
            out.append({"ticket": int(d["ticket"]), "slices": int(d["slices"]), "group": int(d["group"]), "status": int(r["status"]), "n_nodes": int(r["n_nodes"]),
                        "iterations": int(r["iterations"]), "smoothing_iterations": int(r["smoothing_iterations"]), "cost": float(r["cost"]),
                        "wyrand_state": int(r["wyrand_state"]),
                        "path": xy[int(r["first_point"]):int(r["first_point"]) + int(r["n_points"])].copy()})
        return out

    def plan_cancel(self, ticket):
        """the request is never handed out (mgx_plan_cancel); an unknown, collected or cancelled ticket raises"""
        self._chk(self._L.mgx_plan_cancel(self._w, int(ticket)))

    def plan_pending(self):
        """requests submitted and neither collected nor cancelled"""
        n = C.c_uint32(0)
        self._chk(self._L.mgx_plan_pending(self._w, C.byref(n)))
        return int(n.value)

    def plan_tree(self, request):
        """(positions [n, 2] f64, parents [n], stored costs [n]) of a request of the last plan_paths (mgx_plan_tree)"""
        n = C.c_uint32()
        self._chk(self._L.mgx_plan_tree(self._w, int(request), 0, None, None, None, C.byref(n)))
        xy, par, cost = np.zeros((n.value, 2)), np.zeros(n.value, np.int32), np.zeros(n.value)
        if n.value:
            self._chk(self._L.mgx_plan_tree(self._w, int(request), n.value, xy.ctypes.data, par.ctypes.data, cost.ctypes.data, C.byref(n)))
        return xy, par, cost

    def set_resident_launches(self, enabled):
        """per-world switch: False keeps every schedule on the launch-per-segment path (mgx_set_resident_launches)"""
        self._chk(self._L.mgx_set_resident_launches(self._w, 2 if enabled == "decline" else 1 if enabled else 0))

    def resident_outcome(self):
        """what became of the resident launch of the last iterate (hostlib.RESIDENT_NONE / _RAN / _DECLINED: issue it again)"""
        o = C.c_int32()
        self._chk(self._L.mgx_resident_outcome(self._w, C.byref(o)))
        return o.value

    def resident_ready(self, steps):
        """whether iterate(steps) would go out as a resident launch now (mgx_resident_ready)"""
        b, r = bytes(int(x) for x in steps), C.c_int32()
        self._chk(self._L.mgx_resident_ready(self._w, b, len(b), C.byref(r)))
        return bool(r.value)

    def resident_stats(self):
        """(resident launches so far, declined ones, what is left of the back-off after the last declined one)"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._chk(self._L.mgx_resident_stats(self._w, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def group_schedule_stats(self):
        """(iterate / mission_tick_end calls that ran MIXED — groups with different schedules —, the sweep-kernel launches of those
        calls, workgroups that sat such a launch out): mgx_group_schedule_stats"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._L.mgx_group_schedule_stats(self._w, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_group_enabled(self, group, kind_mask):
        """gbp.factors-enabled of ONE robot group (mgx_set_group_enabled): kind_mask of the MGX_FACTOR_* bits, before the group's
        first robot is added.  Dynamic, obstacle and tracking may differ from the world's; the inter-robot bit may not."""
        self._chk(self._L.mgx_set_group_enabled(self._w, int(group), int(kind_mask)))

    def group_enabled(self, group):
        """the kinds a robot added to `group` runs under (mgx_get_group_enabled)"""
        m = C.c_uint32()
        self._chk(self._L.mgx_get_group_enabled(self._w, int(group), C.byref(m)))
        return m.value

    def group_enabled_stats(self):
        """(schedules and world-wide sweeps that ran as group plans only because the world is masked, the sweep-kernel launches of
        those): mgx_group_enabled_stats"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self._L.mgx_group_enabled_stats(self._w, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_group_sigmas(self, group, dynamics=None, interrobot=None, obstacle=None, tracking=None):
        """gbp.sigma-factor-{dynamics, interrobot, obstacle, tracking} of ONE robot group (mgx_set_group_sigmas), before the group's
        first robot is added: every value finite and positive; one left out keeps what the group has (the world's unless set
        before).  A set equal to the world's is none; a world whose groups differ in their sigmas runs as a masked world does."""
        s = hostlib.GroupSigmas()
        self._chk(self._L.mgx_get_group_sigmas(self._w, int(group), C.byref(s)))
        for name, v in (("dynamics", dynamics), ("interrobot", interrobot), ("obstacle", obstacle), ("tracking", tracking)):
            if v is not None:
                setattr(s, name, float(v))
        self._chk(self._L.mgx_set_group_sigmas(self._w, int(group), C.byref(s)))

    def group_sigmas(self, group):
        """the sigmas a robot added to `group` runs under, {dynamics, interrobot, obstacle, tracking}: the group's own, else the
        world's (mgx_get_group_sigmas)"""
        s = hostlib.GroupSigmas()
        self._chk(self._L.mgx_get_group_sigmas(self._w, int(group), C.byref(s)))
        return {"dynamics": s.dynamics, "interrobot": s.interrobot, "obstacle": s.obstacle, "tracking": s.tracking}

    def set_group_resident(self, enabled):
        """True: a masked world's equal schedules (iterate, tick, mission ticks, batches) run as resident launches of the masked
        form of the kernel, lingering and posts included (mgx_set_group_resident); False, the default: as group plans.  Same
        results bit for bit; nothing changes on an unmasked world."""
        self._chk(self._L.mgx_set_group_resident(self._w, 1 if enabled else 0))

    def group_resident_stats(self):
        """(resident launches of the masked form, schedules posted into one, schedules of the switched-on masked world that ran
        as group plans all the same): mgx_group_resident_stats"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._L.mgx_group_resident_stats(self._w, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def is_thawing(self):
        """factors switched back on are still resuming from their frozen inboxes (mgx_is_thawing)"""
        t = C.c_int32()
        self._chk(self._L.mgx_is_thawing(self._w, C.byref(t)))
        return bool(t.value)

    def last_launch_count(self):
        """sweep-kernel launches of the last iterate / tick call (1: the whole schedule ran as one resident launch)"""
        n = C.c_uint32()
        self._chk(self._L.mgx_last_launch_count(self._w, C.byref(n)))
        return n.value

    def last_sweep(self):
        """how the last iterate / tick call ran its sweeps (mgx_last_sweep): (variant, ir_mode, form, resident_capacity) —
        the sweep kernel's horizon variant (K, or 0 / -1 for the run-time-K kernels), inter-robot mode (0 none, 1 unstaged,
        2 staged), form (0 launch per segment, 1 resident launch, 2 posted into a lingering launch, 3 sharded resident launch;
        -1: no sweep ran) and the workgroups of this world's resident instantiation the device holds at once (0: none)"""
        v = [C.c_int32() for _ in range(4)]
        self._chk(self._L.mgx_last_sweep(self._w, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def last_sweep_features(self):
        """the form of the sweep kernel last_sweep reports (mgx_last_sweep_features): bit 0 tracking factors, bit 1 mgx_tick's
        prior updates, bit 2 the kinds per robot group; 0: the lean resident form (or no sweep ran), 3: the full form (every
        launch-per-segment kernel), 7: the masked form (set_group_resident)"""
        f = C.c_uint32()
        self._chk(self._L.mgx_last_sweep_features(self._w, C.byref(f)))
        return int(f.value)

    def set_specialize(self, enabled):
        """False: every resident launch in the full form of the kernel; True: the smallest form that covers it; None: the
        default (MGX_SPECIALIZE) — mgx_set_specialize"""
        self._chk(self._L.mgx_set_specialize(self._w, -1 if enabled is None else int(bool(enabled))))

    def last_search(self):
        """how the last neighbour search ran (mgx_last_search): (kernel, row_cap, n_launches, n_changed, changed) — the kernel it
        launched last (hostlib.SEARCH_*), with which row capacity (0: the two-pass forms), in how many launches, how many robots'
        changed-row flags reached the topology pass behind it (-1: none did) and those flags, one uint8 per robot (None with -1)"""
        v = [C.c_int32() for _ in range(4)]
        n = self._n_ids
        chg = np.full(max(n, 1), 255, dtype=np.uint8)  # (left as it is where no flags are copied)
        self._chk(self._L.mgx_last_search(self._w, *[C.byref(x) for x in v], chg.ctypes.data, n))
        k, cap, launches, n_changed = (int(x.value) for x in v)
        return k, cap, launches, n_changed, (chg[:n] if n_changed >= 0 and (n == 0 or chg[0] != 255) else None)

    def note_change_priors(self, robots, var_ix):
        """counters only: prior changes another rank applied to robots that are ghosts here (mgx_note_change_priors)"""
        r, v = np.ascontiguousarray(robots, dtype=np.int32), np.ascontiguousarray(var_ix, dtype=np.uint32)
        if len(r):
            self._chk(self._L.mgx_note_change_priors(self._w, len(r), r.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     v.ctypes.data_as(C.POINTER(C.c_uint32))))

    def message_counts(self, robot):
        """(sent internal, sent external, received internal, received external) of one graph."""
        out = (C.c_uint64 * 4)()
        self._chk(self._L.mgx_message_counts(self._w, robot, out))
        return tuple(int(x) for x in out)

    def read_variable_means(self, var_ix):
        """Belief mean of one variable of every robot, [n_robots, 4]."""
        nr, _ = self.num_robots()
        out = np.zeros((nr, 4))
        self._chk(self._L.mgx_read_variable_means(self._w, var_ix, _dp(out)))
        return out

    def read_means(self):
        _, nv = self.num_robots()
        means = np.zeros((nv, 4))
        self._chk(self._L.mgx_read_means(self._w, _dp(means)))
        return means

    def read_beliefs(self):
        _, nv = self.num_robots()
        eta, lam, means = np.zeros((nv, 4)), np.zeros((nv, 4, 4)), np.zeros((nv, 4))
        self._chk(self._L.mgx_read_beliefs(self._w, _dp(eta), _dp(lam), _dp(means)))
        return eta, lam, means

    # -- halo ------------------------------------------------------------------------------------
    @staticmethod
    def halo_words(K):
        return hostlib.lib().mgx_halo_words(K)

    # halo exchange through RCCL inside the library (see include/mgx.h)
    def halo_rccl_connect(self, unique_id, n_ranks, rank, peer_rank, send_first, recv_first):
        a = np.ascontiguousarray(peer_rank, dtype=np.uint32)
        b = np.ascontiguousarray(send_first, dtype=np.uint32)
        c = np.ascontiguousarray(recv_first, dtype=np.uint32)
        assert b.size == c.size == (a.size + 1 if a.size else 0) or (a.size == 0)
        self._chk(self._L.mgx_halo_rccl_connect(self._w, unique_id, n_ranks, rank, a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data))

    def halo_rccl_disconnect(self):
        self._chk(self._L.mgx_halo_rccl_disconnect(self._w))

    # direct halo exchange (peer-mapped stores; see include/mgx.h)
    def halo_direct_setup_slots(self, n_sources, slot_capacity):
        """a receive area with one record slot per ghost robot (a wiring that outlives the exchange lists)"""
        recv, flags = C.c_void_p(), C.c_void_p()
        self._chk(self._L.mgx_halo_direct_setup_slots(self._w, n_sources, slot_capacity, C.byref(recv), C.byref(flags)))
        return recv.value, flags.value

    def halo_ghost_slots(self, robots):
        r = np.ascontiguousarray(robots, dtype=np.int32)
        out = np.zeros(r.size, dtype=np.int32)
        self._chk(self._L.mgx_halo_ghost_slots(self._w, r.size, r.ctypes.data, out.ctypes.data))
        return out

    def robot_export(self, robot):
        """the record of a robot this rank owns, for the rank that is to own it (mgx_robot_export)"""
        n = C.c_uint64()
        self._chk(self._L.mgx_robot_export(self._w, int(robot), None, 0, C.byref(n)))
        buf = np.zeros(n.value, dtype=np.uint8)
        self._chk(self._L.mgx_robot_export(self._w, int(robot), buf.ctypes.data, n.value, C.byref(n)))
        return buf.tobytes()

    def robot_import(self, robot, record):
        buf = np.frombuffer(record, dtype=np.uint8)
        self._chk(self._L.mgx_robot_import(self._w, int(robot), buf.ctypes.data, buf.size))

    def robot_release(self, robot):
        self._chk(self._L.mgx_robot_release(self._w, int(robot)))

    def halo_send_list(self):
        """robot ids of the send list as it stands (by consumer rank)"""
        ns, nr = C.c_uint32(), C.c_uint32()
        self._chk(self._L.mgx_halo_get_lists(self._w, None, 0, None, 0, C.byref(ns), C.byref(nr)))
        out = np.zeros(max(ns.value, 1), dtype=np.int32)
        self._chk(self._L.mgx_halo_get_lists(self._w, out.ctypes.data, ns.value, None, 0, C.byref(ns), C.byref(nr)))
        return [int(x) for x in out[:ns.value]]

    def halo_direct_connect_slots(self, send_first, peer_recv_base, peer_slot_capacity, entry_slot, peer_flag_slot):
        n = len(peer_recv_base)
        a = np.ascontiguousarray(send_first, dtype=np.uint32)
        b = np.ascontiguousarray(peer_recv_base, dtype=np.uint64)
        c = np.ascontiguousarray(peer_slot_capacity, dtype=np.uint64)
        d = np.ascontiguousarray(entry_slot, dtype=np.uint32)
        e = np.ascontiguousarray(peer_flag_slot, dtype=np.uint64)
        assert a.size == n + 1 and b.size == c.size == e.size == n and d.size == int(a[-1])
        self._chk(self._L.mgx_halo_direct_connect_slots(self._w, n, a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, e.ctypes.data))

    def halo_direct_exchange(self, what=hostlib.HALO_PUSH | hostlib.HALO_WAIT):
        self._chk(self._L.mgx_halo_direct_exchange(self._w, what))

    def halo_direct_status(self):
        """Number of exchanges so far; raises if one of them timed out waiting for a peer."""
        n, bad = C.c_uint64(), C.c_uint64()
        self._chk(self._L.mgx_halo_direct_status(self._w, C.byref(n), C.byref(bad)))
        return n.value

    def halo_direct_disconnect(self):
        self._chk(self._L.mgx_halo_direct_disconnect(self._w))

    # resident schedule launches on sharded worlds (ghost records travel inside the launches; see include/mgx.h)
    def halo_resident_setup(self, n_recv):
        """Allocates this rank's ghost area.  Returns (area address, ghost slots, parity, segment count, slot of every entry of
        the receive list, eligible)."""
        area, ng, par, seg, ok = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_int32()
        slots = np.zeros(max(int(n_recv), 1), dtype=np.int32)
        self._chk(self._L.mgx_halo_resident_setup(self._w, C.byref(area), C.byref(ng), C.byref(par), C.byref(seg), slots.ctypes.data, C.byref(ok)))
        # (eligible: 1 yes; 2 everything but inter-robot factors — a world that follows its topology may get them later; 0 no)
        return area.value, ng.value, par.value, seg.value, slots[:n_recv].tolist(), int(ok.value)

    def halo_n_recv(self):
        ns, nr = C.c_uint32(), C.c_uint32()
        self._chk(self._L.mgx_halo_get_lists(self._w, None, 0, None, 0, C.byref(ns), C.byref(nr)))
        return nr.value

    def halo_resident_connect_peers(self, peer_area, peer_ghost_slots, peer_parity, peer_segment_count, coordinator_area=None, n_ranks=0):
        """coordinator_area: rank 0's ghost area as this rank maps it — where the ranks agree on every schedule's launches"""
        n = len(peer_area)
        b = np.ascontiguousarray(peer_area, dtype=np.uint64)
        c = np.ascontiguousarray(peer_ghost_slots, dtype=np.uint32)
        e = np.ascontiguousarray(peer_parity, dtype=np.uint32)
        f = np.ascontiguousarray(peer_segment_count, dtype=np.uint64)
        assert b.size == c.size == e.size == f.size == n
        self._chk(self._L.mgx_halo_resident_connect_peers(self._w, n, b.ctypes.data, c.ctypes.data, e.ctypes.data, f.ctypes.data,
                                                          coordinator_area, int(n_ranks)))

    def halo_resident_aim(self, robots, peer_index, peer_slot):
        a = np.ascontiguousarray(robots, dtype=np.int32)
        b = np.ascontiguousarray(peer_index, dtype=np.uint32)
        c = np.ascontiguousarray(peer_slot, dtype=np.uint32)
        assert a.size == b.size == c.size
        self._chk(self._L.mgx_halo_resident_aim(self._w, a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data))

    def halo_resident_disconnect(self):
        self._chk(self._L.mgx_halo_resident_disconnect(self._w))

    def halo_plan(self, send_robots, recv_ghosts):
        a = np.ascontiguousarray(send_robots, dtype=np.int32)
        b = np.ascontiguousarray(recv_ghosts, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._chk(self._L.mgx_halo_plan(self._w, len(a), a.ctypes.data_as(ip), len(b), b.ctypes.data_as(ip)))

    def halo_plan_from_connections(self, rank_of, my_rank, n_ranks):
        """Exchange lists derived from the connections held (mgx_halo_plan_from_connections):
        returns (send_counts, recv_counts) in records per peer rank."""
        rank_of = np.ascontiguousarray(rank_of, dtype=np.int32)
        sc, rc = (C.c_uint32 * n_ranks)(), (C.c_uint32 * n_ranks)()
        self._chk(self._L.mgx_halo_plan_from_connections(self._w, rank_of.ctypes.data_as(C.POINTER(C.c_int32)), rank_of.size,
                                                         int(my_rank), int(n_ranks), sc, rc))
        return list(sc), list(rc)

    def halo_pack(self, dev_ptr):
        self._chk(self._L.mgx_halo_pack(self._w, C.c_void_p(dev_ptr)))

    def halo_unpack(self, dev_ptr):
        self._chk(self._L.mgx_halo_unpack(self._w, C.c_void_p(dev_ptr)))

    def factorgraph(self, robot):
        return FactorGraph(self, robot)


class FactorGraph:
    """Per-robot handle with the method names of the reference ``FactorGraph``
    (factorgraph.rs:688-826,494-528)."""

    def __init__(self, world, robot_id):
        self.world, self.id = world, robot_id

    def internal_factor_iteration(self):
        self.world.internal_factor_iteration(self.id)

    def internal_variable_iteration(self):
        self.world.internal_variable_iteration(self.id)

    def change_prior_of_variable(self, variable_index, new_mean):
        self.world.change_prior(self.id, variable_index, new_mean)
        return []  # routing to external factors happens on the device

    def variable(self, variable_index):
        return self.world.get_belief(self.id, variable_index)

    def set_tracking_path(self, path):
        """modify_tracking_factors(|t| t.set_tracking_path(path)) (robot.rs:674-682)"""
        self.world.set_tracking_path(self.id, path)

    def update_inter_robot_safety_distance_multiplier(self, multiplier):
        """world-wide, like the reference's only caller (ui/settings.rs:586-590: every graph and the config entry)"""
        self.world.set_safety_multiplier(multiplier)


_STEP_BYTES = {}


class _Batch:
    def __init__(self, world):
        self.world, self.schedules, self.launches = world, 0, 0

    def __enter__(self):
        self.world.batch_begin()
        return self

    def __exit__(self, exc_type, exc, tb):
        self.schedules, self.launches = self.world.batch_end()
        return False
