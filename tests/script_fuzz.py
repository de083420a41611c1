"""Seeded scripts over the whole mutator surface of a world (helper of tests/test_script_fuzz_recipes.py, which runs them on
the extended CPU oracle alone, and tests/test_gpu_script_fuzz.py, which runs them on the engine and the oracle side by side).

make_script(seed) is plain numpy and never touches a GPU.  A script is a small grid world (inter-robot factors, tracking
factors on every other seed, a ragged initial topology, the last three robots held back), some twenty operations each followed
by a random schedule, the steps after which the two sides are compared, and a DRESS: calls that change how the engine submits
its work (batches, resident launches, lingering, post merging, flushes) and must not show in any result — on the oracle a dress
operation does nothing.

Operations name robots by their index in the scenario and look them up when they are applied, in what their side has been told
so far (`Script.ctx`): the same script with the calls of one kind left out (Script.without) stays a valid script — robots join
under other ids, nobody is removed — which is what lets the recipe tests ask whether every kind of call matters.

run(script, eng, ref) applies the operations segment by segment — the engine's calls of a segment back to back, then the
oracle's, as a caller that runs ahead would issue them — and compares beliefs (bit for bit), connection sets, message counts,
robot counts and the topology passes' return values at every compare point.  The engine side keeps a TRACE of how the work ran
(sweep form, inter-robot mode, layouts, appends, posts, merged schedules, thawing), read only where the read costs nothing:
mgx_layout_stats and mgx_append_stats are plain reads; mgx_last_sweep, mgx_linger_stats and mgx_post_merge_stats submit what a
batch has recorded (a launch that lingers stays) and are read only in front of a call that submits it anyway; mgx_is_thawing
ends a lingering launch like every mutator and is read only right behind one.  So the trace has one record per STRETCH — a call
and the schedules behind it — not one per schedule: the sweep form and inter-robot mode are those of the stretch's last schedule,
and "thawing" is what the world said right behind the call, in front of the stretch's first schedule."""
import numpy as np

from magics_amd import hostlib, scenarios as S

F32 = np.float32
KS = (10, 12, 16, 21, 13)          # four constant-K kernels and one run-time-K horizon
RUNTIME_K_HORIZON = {13: 30}       # (look-ahead horizon whose variable timesteps number 13: not in the scenarios' table)
HELD_BACK = 3
MULTIPLIERS = (1.0, 2.2, 4.0)
RADII = (3.0, 4.5, 6.0)
METHODS = (hostlib.NEIGHBOURS_AUTO, hostlib.NEIGHBOURS_PAIRS, hostlib.NEIGHBOURS_GRID)
SCHEDULES = ("tick", "iterate")    # kinds that are a schedule and nothing else: they do not end a launch that lingers
KINDS = ("switch", "multiplier", "tracking_path", "handler", "change_prior", "change_priors", "set_antenna", "set_idle",
         "set_antennas", "connect", "disconnect", "topology", "remove", "late_add", "update_priors", "tick", "iterate")
TRACKING_ONLY = ("tracking_path", "handler")
_WEIGHTS = dict(switch=3.0, multiplier=1.5, tracking_path=1.0, handler=1.5, change_prior=0.7, change_priors=0.7, set_antenna=0.7,
                set_idle=0.6, set_antennas=0.7, connect=1.2, disconnect=0.7, topology=1.5, remove=0.6, late_add=1.6,
                update_priors=0.8, tick=1.0, iterate=1.0)


class Op:
    """one operation: `call(world, ctx, side)` (None: nothing but the schedule), then iterate(steps) (None: no schedule — a tick
    carries its own, a dress operation has none)"""

    def __init__(self, script, kind, text, call, steps=None, tags=(), dress=False):
        self.script, self.kind, self.text, self.call, self.steps, self.tags, self.dress = script, kind, text, call, steps, frozenset(tags), dress
        self.mask = None        # the kinds switched on while the operation's schedule runs (the generator's picture; None: dress)
        self.tick_steps = None  # a tick's own schedule

    def describe(self):
        return self.text + (f"; iterate({self.steps})" if self.steps is not None else "")

    def apply(self, world, side):
        assert side in ("engine", "oracle"), side
        if self.dress and side == "oracle":
            return
        ctx = self.script.ctx[side]
        probe = ctx.get("probe")
        if probe is not None and self.kind not in SCHEDULES:
            probe.settle()  # (in front of a call that submits and ends whatever is there)
        if self.call is not None:
            self.call(world, ctx, side)
        if probe is not None:
            probe.note(self, world)
        if self.steps is not None:
            world.iterate(self.steps)


class Script:
    def __init__(self, seed):
        self.seed, self.ops, self.compare_after, self.ctx = seed, [], set(), {}
        self.scenario = self.first = None
        self.reserve = None        # engine only: mgx_world_reserve before the first robot (None: never)
        self.first_number = 1      # the robot number generator's next number when the script starts
        self.dress = {}

    def describe(self, upto=None):
        ops = self.ops if upto is None else self.ops[:upto + 1]
        return "\n".join(f"  {i:2d}: {op.describe()}" for i, op in enumerate(ops))

    def kinds(self):
        return [op.kind for op in self.ops if not op.dress]

    def reset(self, side):
        n0 = len(self.first["robots"])
        self.ctx[side] = dict(id_of={i: i for i in range(n0)}, index_of=list(range(n0)), removed=set(), next_number=self.first_number,
                              returns=[])
        return self.ctx[side]

    def _copy(self, keep):
        s = Script(self.seed)
        s.scenario, s.first, s.reserve, s.dress, s.first_number = self.scenario, self.first, self.reserve, self.dress, self.first_number
        s.compare_after = set(self.compare_after)
        for op in self.ops:
            s.ops.append(Op(s, op.kind, op.text, op.call if keep(op) else None, op.steps, op.tags, op.dress))
            s.ops[-1].mask, s.ops[-1].tick_steps = op.mask, op.tick_steps
        return s

    def without(self, kind):
        """the same script without the calls of one kind: their schedules stay (a tick keeps its schedule and loses its prior updates)"""
        s = self._copy(lambda op: op.kind != kind)
        if kind == "tick":
            for op, mine in zip(s.ops, self.ops):
                if op.kind == "tick":
                    op.steps, op.text = mine.tick_steps, "(tick left out)"
        if kind == "iterate":
            for op in s.ops:
                if op.kind == "iterate":
                    op.steps = None
        return s

    def undressed(self):
        s = self._copy(lambda op: not op.dress)
        s.ops = [op for op in s.ops if not op.dress]
        # (compare points are op indices: one that stands behind a dress operation moves to the operation in front of it)
        behind = np.cumsum([0 if op.dress else 1 for op in self.ops]) - 1
        s.compare_after = {int(behind[i]) for i in self.compare_after if behind[i] >= 0}
        return s


# ---- what the calls need of their side's state ---------------------------------------------------------------------------------
def _live(ctx, indices):
    """(ids, scenario indices) of the listed robots that have joined and not been removed, on this side"""
    pairs = [(ctx["id_of"][i], i) for i in indices if i in ctx["id_of"] and i not in ctx["removed"]]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _grid(K, n, seed, tracking):
    # (the scenarios' table of horizons has no entry for 13 variables: one for the time being, as the other tests do)
    added = K not in S.HORIZON_FOR_K
    if added:
        S.HORIZON_FOR_K[K] = RUNTIME_K_HORIZON[K]
    try:
        return S.grid_scenario(n, K, interrobot=True, tracking=tracking, seed=seed, pitch=2.5, comm_radius=4.5)
    finally:
        if added:
            del S.HORIZON_FOR_K[K]


def make_script(seed, n_ops=20, K=None, tracking=None):
    """K, tracking: None for the seed's own; given, they replace it and nothing else — the draws are the same (tests/group_fuzz.py:
    the scripts that share a world share the horizon and the kinds of factors)"""
    rng = np.random.default_rng(seed)
    sp = Script(seed)
    own_K = int(KS[int(rng.integers(0, len(KS)))])
    K = own_K if K is None else int(K)
    n = int(rng.integers(6, 13))
    tracking = seed % 2 == 0 if tracking is None else bool(tracking)
    sc = _grid(K, n, seed, tracking)
    n0 = n - HELD_BACK
    # the held-back robots' order keys run against their ids: whatever sorts by key must not get away with sorting by id
    sc["robots"][n0:] = [dict(rb, order_key=n - 1 - j) for j, rb in enumerate(sc["robots"][n0:])]
    full = sc["params"]["enable_mask"]
    # ragged: a quarter of the directed connections dropped; those and the held-back robots' are there for ir_connect
    kept = [c for c in sc["ir"] if c[0] < n0 and c[1] < n0 and rng.random() > 0.25]
    if len(kept) == sum(1 for c in sc["ir"] if c[0] < n0 and c[1] < n0):
        kept = kept[1:]  # (never the full topology)
    if seed % 4 == 3:
        kept = []        # (every fourth world starts unconnected: its sweeps stage no inter-robot messages until somebody connects)
    spare = [c for c in sc["ir"] if c not in kept]
    rng.shuffle(spare)
    sp.scenario = sc
    sp.first = dict(sc, robots=sc["robots"][:n0], ir=kept)
    sp.first_number = 1 + (K - 1) * len(sc["ir"])
    if rng.random() < 0.5:
        sp.reserve = int(rng.choice([n, n0 + 1]))  # room for all three, or for one: the second outgrows it
    tick = S.tick_inputs(sc)
    pos = np.array([[rb["pos"][0], 0.5, rb["pos"][1]] for rb in sc["robots"]], dtype=F32)

    # -- the generator's own picture of the world (exact when nothing is left out: what describe() says is what happens)
    present, removed, joined = list(range(n0)), set(), 0
    mask, switched, room = full, False, sp.reserve
    maybe_connected = {frozenset(c[:2]) for c in kept}

    def live():
        return [i for i in present if i not in removed]

    def steps():
        return [int(x) for x in rng.integers(1, 4, size=int(rng.integers(1, 6)))]

    def add(kind, text, call, tags=(), own_schedule=False):
        sp.ops.append(Op(sp, kind, text, call, None if own_schedule else steps(), tags))
        return sp.ops[-1]

    burst_at = int(rng.integers(3, n_ops - 4))  # three schedules back to back somewhere: what a launch that lingers is posted
    kinds = [k for k in KINDS if tracking or k not in TRACKING_ONLY]
    weights = np.array([_WEIGHTS[k] for k in kinds])
    weights /= weights.sum()
    k_op = 0
    while k_op < n_ops:
        kind = str(rng.choice(kinds, p=weights)) if not burst_at <= k_op < burst_at + 3 else ("tick" if rng.random() < 0.4 else "iterate")
        lv = live()
        if kind == "switch":
            # mostly a random subset of the kinds the world was created with goes off; a world with something off often gets
            # everything back, and a world that is thawing is sometimes switched again at once
            if mask != full and rng.random() < 0.45:
                new = full
            else:
                new = full & ~int(rng.integers(0, 16)) if rng.random() < 0.8 else full
            tags = {"switch"}
            if new & ~mask:
                tags.add("switch_on")
            if mask & ~new:
                tags.add("switch_off")
            if (new ^ mask) & S.EN_TRK:
                tags.add("switch_tracking")
            if (new & ~mask) & S.EN_IR:
                tags.add("ir_on")
            if k_op == 0:
                tags.add("before_first_iteration")
            add(kind, f"set_enabled({new}) [was {mask}]", lambda w, ctx, side, m=new: w.set_enabled(m), tags)
            mask, switched = new, True
        elif kind == "multiplier":
            m = float(rng.choice(MULTIPLIERS))
            add(kind, f"set_safety_multiplier({m})", lambda w, ctx, side, m=m: w.set_safety_multiplier(m),
                {"multiplier_off"} if not mask & S.EN_IR else ())
        elif kind == "tracking_path":
            i = int(rng.choice(lv))
            path = sc["robots"][i]["path"].copy()
            path[1:] += rng.normal(0, 1.5, size=(2, 2)).astype(F32)

            def call(w, ctx, side, i=i, path=path):
                ids, _ = _live(ctx, [i])
                if ids:
                    w.set_tracking_path(ids[0], path)
            add(kind, f"set_tracking_path({i}, {path.tolist()})", call)
        elif kind == "handler":
            robots = sorted(int(i) for i in rng.choice(lv, size=min(len(lv), int(rng.integers(1, 4))), replace=False))
            means = np.array([sc["robots"][i]["mean0"] + rng.normal(0, 0.3, size=(K, 4)) for i in robots])
            paths = [np.ascontiguousarray(m[[0, K // 2, K - 1], :2], dtype=F32) for m in means]

            def call(w, ctx, side, robots=robots, means=means, paths=paths):
                ids, idx = _live(ctx, robots)
                if not ids:
                    return
                sel = [robots.index(i) for i in idx]
                if side == "engine":  # the completion handler in one call
                    w.apply_global_paths(ids, [paths[s] for s in sel], means[sel], reset_tracking=True)
                else:                 # robot.rs:674-769, robot by robot
                    for r, s in zip(ids, sel):
                        w.set_tracking_path(r, paths[s])
                        w.reset_variables(r, means[s])
                        w.reset_tracking_factors(r)
            add(kind, f"apply_global_paths({robots}) / handler sequence, means mean0 + N(0, 0.3)", call,
                {"handler_after_switch" if switched else "handler_no_switch_before"})
        elif kind == "change_prior":
            i, var = int(rng.choice(lv)), int(rng.choice([0, K - 1]))
            m = sc["robots"][i]["mean0"][var] + rng.normal(0, 1.0, size=4)

            def call(w, ctx, side, i=i, var=var, m=m):
                ids, _ = _live(ctx, [i])
                if ids:
                    w.change_prior(ids[0], var, m)
            add(kind, f"change_prior({i}, {var}, {m.tolist()})", call)
        elif kind == "change_priors":
            robots = sorted(int(i) for i in rng.choice(lv, size=min(len(lv), 3), replace=False))
            var = [int(v) for v in rng.choice([0, K - 1], size=len(robots))]
            m = np.array([sc["robots"][i]["mean0"][v] for i, v in zip(robots, var)]) + rng.normal(0, 1.0, size=(len(robots), 4))

            def call(w, ctx, side, robots=robots, var=var, m=m):
                ids, idx = _live(ctx, robots)
                sel = [robots.index(i) for i in idx]
                if ids:
                    w.change_priors(ids, [var[s] for s in sel], m[sel])
            add(kind, f"change_priors({robots}, {var})", call)
        elif kind in ("set_antenna", "set_idle"):
            i, v = int(rng.choice(lv)), bool(rng.integers(0, 2))

            def call(w, ctx, side, i=i, v=v, kind=kind):
                ids, _ = _live(ctx, [i])
                if ids:
                    getattr(w, kind)(ids[0], v)
            add(kind, f"{kind}({i}, {v})", call)
        elif kind == "set_antennas":
            on = rng.random(n) > 0.3

            def call(w, ctx, side, on=on):
                ids, idx = _live(ctx, range(n))
                w.set_antennas(np.array(ids, dtype=np.int32), on[idx])
            add(kind, f"set_antennas(live, {on.astype(int).tolist()})", call)
        elif kind == "connect":
            usable = [c for c in spare if c[0] in lv and c[1] in lv]
            if not usable:
                continue
            a, b, n0_ = usable[0]
            spare.remove(usable[0])
            maybe_connected.add(frozenset((a, b)))

            def call(w, ctx, side, a=a, b=b, n0_=n0_):
                ids, _ = _live(ctx, [a, b])
                if len(ids) == 2:
                    w.ir_connect(ids[0], ids[1], n0_ + 100000)
            add(kind, f"ir_connect({a}, {b})" + ("" if mask & S.EN_IR else " [inter-robot factors off: keyless]"), call,
                {"connect_off"} if not mask & S.EN_IR else ())
        elif kind == "disconnect":
            usable = sorted(tuple(sorted(p)) for p in maybe_connected if all(i in lv for i in p))
            if not usable:
                continue
            a, b = usable[int(rng.integers(0, len(usable)))]
            maybe_connected.discard(frozenset((a, b)))

            def call(w, ctx, side, a=a, b=b):
                ids, _ = _live(ctx, [a, b])
                if len(ids) == 2:
                    w.ir_disconnect(ids[0], ids[1])
            add(kind, f"ir_disconnect({a}, {b})", call)
        elif kind == "topology":
            pos = pos + rng.normal(0, 1.2, size=pos.shape).astype(F32) * np.array([1, 0, 1], dtype=F32)
            radius, method = float(rng.choice(RADII)), int(rng.choice(METHODS))
            for a in lv:
                for b in lv:
                    if a < b and np.linalg.norm(pos[a] - pos[b]) <= radius + 0.01:
                        maybe_connected.add(frozenset((a, b)))

            def call(w, ctx, side, p=pos.copy(), radius=radius, method=method):
                out = w.update_topology(p[ctx["index_of"]], radius, ctx["next_number"], method)
                ctx["next_number"] = out[0]
                ctx["returns"].append(tuple(int(x) for x in out))
            add(kind, f"update_topology(walked positions, {radius}, method {method})", call,
                {"topology_off"} if not mask & S.EN_IR else ())
        elif kind == "remove":
            if len(lv) <= 4:
                continue
            i = int(rng.choice(lv))
            removed.add(i)

            def call(w, ctx, side, i=i):
                ids, _ = _live(ctx, [i])
                if ids:
                    w.remove_robot(ids[0])
                    ctx["removed"].add(i)
            add(kind, f"remove_robot({i})", call)
        elif kind == "late_add":
            if joined == HELD_BACK:
                continue
            i = n0 + joined
            joined += 1
            present.append(i)
            tags = {"late_add"}
            if room is not None and len(present) > room:
                tags.add("outgrows")  # laid out in full, with twice the room
                room = 2 * len(present)
            rb = sc["robots"][i]

            def call(w, ctx, side, i=i, rb=rb):
                rid = w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=rb["order_key"])
                assert rid == len(ctx["index_of"]), (rid, ctx["index_of"])
                ctx["id_of"][i] = rid
                ctx["index_of"].append(i)
            add(kind, f"add_robot(scenario robot {i}, order_key {rb['order_key']})" + (" [outgrows the reservation]" if "outgrows" in tags else ""),
                call, tags)
        elif kind in ("update_priors", "tick"):
            st = steps()

            def call(w, ctx, side, st=st, one_call=(kind == "tick")):
                ids, idx = _live(ctx, range(n))
                args = dict(tick, robots=np.array(ids, dtype=np.int32), waypoints_xy=tick["waypoints_xy"][idx], time_scale=tick["time_scale"][idx],
                            what=tick["what"][idx])
                if one_call:
                    w.tick(steps=st, **args)
                else:
                    w.update_priors(**args)
            if kind == "tick":
                op = add(kind, f"tick(live robots, steps={st})", call, own_schedule=True)
                op.tick_steps = st
            else:
                add(kind, "update_priors(live robots)", call).steps = st
        else:
            add("iterate", "(another schedule)", None)
        sp.ops[-1].mask = mask  # (the kinds switched on while the operation's schedule runs)
        k_op += 1

    # -- compare points: after every `stride`-th operation, and always at the end
    stride = int(rng.choice([1, 3, 7, 0]))
    sp.compare_after = {i for i in range(len(sp.ops)) if stride and i % stride == stride - 1} | {len(sp.ops) - 1}
    _dress(sp, rng)
    return sp


def _dress(sp, rng):
    """engine-only calls around and between the operations; compare points move with the operations they follow"""
    d = dict(batch=bool(rng.random() < 0.35), resident=str(rng.choice(["on", "on", "off", "off_then_on", "on_then_off"])),
             linger=(0 if rng.random() < 0.3 else None), post_merge=int(rng.integers(0, 3)))
    sp.dress = d
    n = len(sp.ops)
    inserts = {}  # op index -> dress operations in front of it

    def dress(at, text, call):
        inserts.setdefault(at, []).append(Op(sp, "dress", text, call, None, (), dress=True))
    if d["linger"] is not None:
        dress(0, f"set_linger({d['linger']})", lambda w, ctx, side: w.set_linger(d["linger"]))
    dress(0, f"set_post_merge({d['post_merge']})", lambda w, ctx, side: w.set_post_merge(d["post_merge"]))
    if d["resident"] in ("off", "off_then_on"):
        dress(0, "set_resident_launches(False)", lambda w, ctx, side: w.set_resident_launches(False))
    if d["resident"] in ("off_then_on", "on_then_off"):
        on = d["resident"] == "off_then_on"
        dress(int(rng.integers(2, n - 1)), f"set_resident_launches({on})", lambda w, ctx, side: w.set_resident_launches(on))
    for _ in range(2):
        name = str(rng.choice(["flush", "synchronize"]))
        dress(int(rng.integers(1, n)), f"{name}()", lambda w, ctx, side, name=name: getattr(w, name)())
    if d["batch"]:
        dress(0, "batch_begin()", lambda w, ctx, side: w.batch_begin())

        def end(w, ctx, side):
            ctx["batch_end"] = w.batch_end()
        dress(n, "batch_end()", end)
    ops, compare = [], set()
    for i in range(n + 1):
        ops.extend(inserts.get(i, []))
        if i < n:
            ops.append(sp.ops[i])
            if i in sp.compare_after:
                compare.add(len(ops) - 1)
    compare.add(len(ops) - 1)  # (behind batch_end, where there is one)
    sp.ops, sp.compare_after = ops, compare


# ---- running a script ------------------------------------------------------------------------------------------------------------
def build_worlds(script, engine=True):
    """(engine or None, extended oracle) populated with the script's first robots, as oracle_ext.make_pair makes them"""
    from oracle_ext import ExtOracleWorld
    ref = ExtOracleWorld(script.scenario["params"])
    ids = S.populate(ref, script.first)
    eng = None
    if engine:
        from magics_amd import World
        eng = World(script.scenario["params"])
        if script.reserve:
            eng.reserve(script.reserve)
        assert S.populate(eng, script.first) == ids
    return eng, ref


class Probe:
    """how the engine ran the script: one record per stretch [call, schedule, schedule ...] between two calls that are no schedule"""

    def __init__(self, eng, script):
        self.eng, self.script, self.records, self.pending, self.thawing = eng, script, [], [], False
        self.pure, self.sched = self._pure(), self._sched()

    def _pure(self):
        return self.eng.layout_stats() + self.eng.append_stats()

    def _sched(self):
        return self.eng.linger_stats() + self.eng.post_merge_stats()

    def note(self, op, world):
        if op.dress:
            return
        if op.kind not in SCHEDULES:
            self.thawing = world.is_thawing()  # (right behind a call that has ended whatever launch was there)
        self.pending.append(op)

    def settle(self):
        if not self.pending:
            return
        sweep = self.eng.last_sweep()  # (first: it submits what a batch has recorded — the layouts that go with it happen here)
        sched, pure = self._sched(), self._pure()
        d_sched = tuple(a - b for a, b in zip(sched, self.sched))
        d_pure = tuple(a - b for a, b in zip(pure, self.pure))
        self.records.append(dict(kinds=[op.kind for op in self.pending], tags=set().union(*[op.tags for op in self.pending]),
                                 schedules=sum(1 for op in self.pending if op.steps is not None or op.kind == "tick"),
                                 variant=sweep[0], ir_mode=sweep[1], form=sweep[2], thawing=self.thawing, mask=self.pending[-1].mask,
                                 d_layout=d_pure[:2], d_append=d_pure[2:], d_linger=d_sched[:4], d_post=d_sched[4:]))
        self.sched, self.pure, self.pending, self.thawing = sched, pure, [], False


class Result:
    def __init__(self):
        self.finite, self.final, self.records, self.batch_end, self.n_compared = [], None, [], None, 0


def _same_beliefs(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _compare(script, step, eng, ref):
    from parity import assert_identical
    what = f"seed {script.seed} after step {step}"
    ce, cr = script.ctx["engine"], script.ctx["oracle"]
    assert ce["returns"] == cr["returns"], f"{what}: update_topology returned {ce['returns']} on the engine, {cr['returns']} on the oracle"
    assert eng.num_robots() == ref.num_robots(), f"{what}: num_robots {eng.num_robots()} != {ref.num_robots()}"
    assert_identical(eng, ref, what=what)
    live = [r for r, i in enumerate(cr["index_of"]) if i not in cr["removed"]]
    got, want = [eng.connections(r) for r in live], [ref.connections(r) for r in live]
    assert got == want, f"{what}: connections of robots {live}: {got} != {want}"
    got, want = [eng.message_counts(r) for r in live], [ref.message_counts(r) for r in live]
    assert got == want, f"{what}: message counts of robots {live}: {got} != {want}"


def run(script, eng, ref, upto=None, at_compare=None):
    """the script (its operations 0 .. upto) on both sides, compared at its compare points and at the end; eng None: the oracle
    alone.  Returns a Result: whether the oracle's beliefs were finite at every compare point, its final beliefs, the engine's
    trace.  A failed comparison carries the seed, the step and every operation up to it.  at_compare(step, ref): called at every
    compare point (tests/group_fuzz.py takes the oracle's state there)."""
    res = Result()
    last = len(script.ops) - 1 if upto is None else min(upto, len(script.ops) - 1)
    script.reset("oracle")
    if eng is not None:
        script.reset("engine")["probe"] = Probe(eng, script)
    first = 0
    for step in range(last + 1):
        if step not in script.compare_after and step != last:
            continue
        sides = ([("engine", eng)] if eng is not None else []) + [("oracle", ref)]
        try:
            for side, w in sides:  # (the engine's calls back to back, then the oracle's)
                for op in script.ops[first:step + 1]:
                    op.apply(w, side)
            if eng is not None:
                _compare(script, step, eng, ref)
                script.ctx["engine"]["probe"].settle()
                res.n_compared += 1
        except Exception as e:
            raise AssertionError(f"script fuzz seed {script.seed}, operations {first} .. {step} (dress {script.dress}, reserve "
                                 f"{script.reserve}, scenario {script.scenario['name']}): {type(e).__name__}: {e}\n"
                                 f"{script.describe(step)}") from e
        res.finite.append(all(np.isfinite(x).all() for x in ref.read_beliefs()))
        if at_compare is not None:
            at_compare(step, ref)
        first = step + 1
    res.final = ref.read_beliefs()
    if eng is not None:
        res.records = script.ctx["engine"]["probe"].records
        res.batch_end = script.ctx["engine"].get("batch_end")
    return res
