"""Seeded scripts over the mutator surface of a GROUPED world (helper of tests/test_group_fuzz_recipes.py, which runs them on the
oracles alone, and tests/test_gpu_group_fuzz.py, which runs them on the engine): M = 3 scripts of script_fuzz.make_script are the
three groups of ONE world.

make_scripts(seed, K) makes the three scripts — one horizon and one tracking flag, since they share a world, and the first
script's obstacle image for all — without their dress and without the kinds of call that cannot run per group (LEFT_OUT).  A
topology pass of a grouped world is one call over ALL groups (mgx_update_topology_groups_radii: one radius and one robot number
generator per group), so the passes are ALIGNED: at a step where any of the three scripts has a `topology` operation every script
gets one, over its own walked positions with its own radius.  Each script is still a script of its own: reference(script) runs it
on an oracle of its own through script_fuzz.run(script, None, ref) and keeps what the oracle holds at the script's compare points.

run_shared(scripts, world) is the adapter.  Every script sees a GroupView: a world-like object that maps the script's robot ids to
the shared world's, passes group=g on every add_robot, answers update_topology from the step's one update_topology_groups call,
and does not iterate — it notes the schedule.  The three schedules of a step (an operation's iterate(steps), a tick's own) go as
ONE per-group call; a tick's prior updates go through update_priors in front of it.  After a step, every group whose script has a
compare point there is compared with its oracle's state: beliefs bit for bit, connections through the id table, message counts,
the topology passes' return values."""
import numpy as np

import script_fuzz as SF
from test_gpu_groups_schedules import segments

M = 3
# kinds of call that cannot run per group, left out with Script.without (their schedules stay), and what makes them so
LEFT_OUT = (
    "switch",       # include/mgx.h:147-148: a mixed schedule is refused (MGX_ERR_STATE) on a world that has switched a factor kind
                    # (mgx_set_enabled: the thaw kernels are world-wide)
    "multiplier",   # include/mgx.h:150: "Everything else is per robot and does not look at the group" — the safety distance
                    # multiplier (mgx_set_safety_multiplier) is one number of the world's parameters
)
KEPT = tuple(k for k in SF.KINDS if k not in LEFT_OUT)
F32 = np.float32


def script_seeds(seed):
    return [1000 + M * seed + g for g in range(M)]


def make_scripts(seed, K, tracking=None):
    """the three scripts of world `seed`"""
    tracking = seed % 2 == 0 if tracking is None else tracking
    scripts = []
    for s in script_seeds(seed):
        sp = SF.make_script(s, K=K, tracking=tracking).undressed()
        for kind in LEFT_OUT:
            sp = sp.without(kind)
        scripts.append(sp)
    for sp in scripts[1:]:   # one world, one obstacle image
        sp.scenario["sdf"] = sp.first["sdf"] = scripts[0].scenario["sdf"]
    _align_topology(scripts, seed)
    return scripts


def _align_topology(scripts, seed):
    n_ops = len(scripts[0].ops)
    assert all(len(sp.ops) == n_ops for sp in scripts)
    for k in range(n_ops):
        if not any(sp.ops[k].kind == "topology" for sp in scripts):
            continue
        for g, sp in enumerate(scripts):
            op = sp.ops[k]
            if op.kind == "topology":
                continue
            rng = np.random.default_rng([seed, k, g])
            pos = np.array([[rb["pos"][0], 0.5, rb["pos"][1]] for rb in sp.scenario["robots"]], dtype=F32)
            pos = pos + rng.normal(0, 1.2, size=pos.shape).astype(F32) * np.array([1, 0, 1], dtype=F32)
            radius = float(rng.choice(SF.RADII))

            def call(w, ctx, side, p=pos, radius=radius, inner=op.call):
                out = w.update_topology(p[ctx["index_of"]], radius, ctx["next_number"], 0)
                ctx["next_number"] = out[0]
                ctx["returns"].append(tuple(int(x) for x in out))
                if inner is not None:
                    inner(w, ctx, side)
            # (an operation whose own call has been left out is a topology pass and nothing else)
            sp.ops[k] = SF.Op(sp, op.kind if op.call is not None or op.kind in SF.SCHEDULES else "topology", f"update_topology(walked start positions, {radius}); " + op.text, call, op.steps, op.tags | {"aligned_topology"})
            sp.ops[k].mask, sp.ops[k].tick_steps = op.mask, op.tick_steps


def schedule_of(op):
    """the schedule an operation ends with: its iterate(steps), or a tick's own"""
    if op.kind == "tick" and op.call is not None:
        return op.tick_steps
    return op.steps if op.steps is not None else []


def ragged_steps(scripts):
    """at how many steps the three schedules do not have the same number of segments"""
    return sum(len({len(segments(schedule_of(sp.ops[k]))) for sp in scripts}) > 1 for k in range(len(scripts[0].ops)))


# ---- the reference: every script on an oracle of its own ---------------------------------------------------------------------------
def reference(script):
    """(Result, {step: what the oracle held at that compare point}) of script_fuzz.run(script, None, ref)"""
    _, ref = SF.build_worlds(script, engine=False)
    held = {}

    def keep(step, ref):
        ctx = script.ctx["oracle"]
        live = [r for r, i in enumerate(ctx["index_of"]) if i not in ctx["removed"]]
        held[step] = dict(beliefs=[b.copy() for b in ref.read_beliefs()], n=len(ctx["index_of"]), live=live, returns=list(ctx["returns"]),
                          connections=[ref.connections(r) for r in live], counts=[ref.message_counts(r) for r in live])
    res = SF.run(script, None, ref, at_compare=keep)
    return res, held


# ---- the adapter -------------------------------------------------------------------------------------------------------------------
class GroupView:
    """group g of the shared world as script g sees it: a world of its own, robot ids from 0"""

    def __init__(self, world, g):
        self.w, self.g, self.ids, self.schedule, self.topology = world, g, [], None, None

    def _id(self, r):
        return self.ids[int(r)]

    def set_sdf(self, rgb, world_w, world_h):
        pass   # (the shared world has the one image already)

    def add_robot(self, mean0, prior_diag, dt, radius, path=None, order_key=None):
        # (order keys are unique in a world and only ever compared within a group: the script's own, spread over the groups)
        key = None if order_key is None else M * int(order_key) + self.g
        self.ids.append(self.w.add_robot(mean0, prior_diag, dt, radius, path=path, order_key=key, group=self.g))
        return len(self.ids) - 1

    def remove_robot(self, r):
        self.w.remove_robot(self._id(r))

    def ir_connect(self, a, b, first_robot_number):
        self.w.ir_connect(self._id(a), self._id(b), first_robot_number)

    def ir_disconnect(self, a, b):
        self.w.ir_disconnect(self._id(a), self._id(b))

    def set_antenna(self, r, on):
        self.w.set_antenna(self._id(r), on)

    def set_idle(self, r, idle):
        self.w.set_idle(self._id(r), idle)

    def set_antennas(self, robots, on):
        self.w.set_antennas(np.array([self._id(r) for r in robots], dtype=np.int32), on)

    def set_tracking_path(self, r, path):
        self.w.set_tracking_path(self._id(r), path)

    def apply_global_paths(self, robots, paths, means, **kw):
        self.w.apply_global_paths([self._id(r) for r in robots], paths, means, **kw)

    def change_prior(self, r, var, mean):
        self.w.change_prior(self._id(r), var, mean)

    def change_priors(self, robots, var, means):
        self.w.change_priors([self._id(r) for r in robots], var, means)

    def update_priors(self, robots, **kw):
        self.w.update_priors(robots=np.array([self._id(r) for r in robots], dtype=np.int32), **kw)

    def tick(self, robots, steps, **kw):
        self.update_priors(robots, **kw)
        self.iterate(steps)

    def iterate(self, steps):
        assert self.schedule is None, "one schedule per step"
        self.schedule = [int(s) for s in steps]

    def update_topology(self, positions, radius, next_number, method=0):
        """answered from the step's one update_topology_groups call, which run_shared has made with these arguments"""
        pos, rad, nxt, out = self.topology
        assert np.array_equal(pos, np.asarray(positions, dtype=F32)) and rad == radius and nxt == next_number, (self.g, "topology arguments")
        self.topology = None
        return out


def _topology_arguments(op):
    """(positions by scenario index, radius, method) of a topology operation: script_fuzz's own (the call's bound defaults), or the
    aligned one's"""
    d = op.call.__defaults__
    if "aligned_topology" in op.tags:
        return d[0], d[1], 0
    return d[0], d[1], d[2]


def build_shared(scripts):
    """the shared world with the scripts' first robots, ids interleaved across the groups, and the three views"""
    from magics_amd import World
    sc = scripts[0].scenario
    assert all(sp.scenario["params"] == sc["params"] and sp.scenario["K"] == sc["K"] for sp in scripts)
    world = World(sc["params"])
    world.set_sdf(sc["sdf"]["rgb"], sc["sdf"]["world_w"], sc["sdf"]["world_h"])
    n_first = sum(len(sp.first["robots"]) for sp in scripts)
    if any(sp.reserve for sp in scripts):
        world.reserve(n_first + 1)   # room for ONE late robot: the second one outgrows it
    views = [GroupView(world, g) for g in range(M)]
    for i in range(max(len(sp.first["robots"]) for sp in scripts)):
        for v, sp in zip(views, scripts):
            if i < len(sp.first["robots"]):
                rb = sp.first["robots"][i]
                assert v.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=rb["order_key"]) == i
    for v, sp in zip(views, scripts):
        for a, b, n0 in sp.first["ir"]:
            v.ir_connect(a, b, n0)
    return world, views


def _compare(seed, step, g, script, view, world, held):
    what = f"group fuzz seed {seed}, group {g} (script seed {script.seed}) after step {step}"
    want, ctx = held[step], script.ctx["engine"]
    assert ctx["returns"] == want["returns"], f"{what}: update_topology returned {ctx['returns']} in the shared world, {want['returns']} on the oracle"
    assert len(view.ids) == want["n"], f"{what}: {len(view.ids)} robots, the oracle has {want['n']}"
    K = script.scenario["K"]
    sel = np.array(view.ids)
    for name, a, b in zip(("eta", "lam", "mean"), world.read_beliefs(), want["beliefs"]):
        a = a.reshape((-1, K) + a.shape[1:])[sel]
        b = b.reshape((len(sel), K) + b.shape[1:])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: {name} differs from the oracle in {int((a != b).sum())} elements"
    got = [world.connections(view.ids[r]) for r in want["live"]]
    assert got == [[view.ids[j] for j in c] for c in want["connections"]], f"{what}: connections of robots {want['live']}: {got}"
    got = [world.message_counts(view.ids[r]) for r in want["live"]]
    assert got == want["counts"], f"{what}: message counts of robots {want['live']}: {got} != {want['counts']}"


def run_shared(seed, scripts, held):
    """the three scripts on ONE world; held[g]: reference(scripts[g])[1].  Returns (the world, comparisons made)"""
    world, views = build_shared(scripts)
    for sp in scripts:
        sp.reset("engine")
    compared = 0
    for k in range(len(scripts[0].ops)):
        ops = [sp.ops[k] for sp in scripts]
        try:
            if any(op.kind == "topology" or "aligned_topology" in op.tags for op in ops):
                # one pass over all groups: every script's positions, radius and number generator
                args = [_topology_arguments(op) for op in ops]
                pos = np.zeros((sum(len(v.ids) for v in views), 3), dtype=F32)
                nxt = np.zeros(M, dtype=np.uint64)
                for g, (v, sp) in enumerate(zip(views, scripts)):
                    pos[v.ids] = args[g][0][sp.ctx["engine"]["index_of"]]
                    nxt[g] = sp.ctx["engine"]["next_number"]
                methods = {a[2] for a in args if a[2]}
                out, stats = world.update_topology_groups(pos, np.array([a[1] for a in args], dtype=F32), nxt, methods.pop() if len(methods) == 1 else 0)
                for g, (v, sp) in enumerate(zip(views, scripts)):
                    v.topology = (args[g][0][sp.ctx["engine"]["index_of"]], args[g][1], int(nxt[g]), (int(out[g]), int(stats[g][0]), int(stats[g][1])))
            for v, op in zip(views, ops):
                op.apply(v, "engine")
                assert v.topology is None
            per_group = [v.schedule if v.schedule is not None else [] for v in views]
            for v in views:
                v.schedule = None
            if any(len(s) for s in per_group):
                world.iterate(per_group)
            for g, (v, sp) in enumerate(zip(views, scripts)):
                if k in held[g]:
                    _compare(seed, k, g, sp, v, world, held[g])
                    compared += 1
        except Exception as e:
            text = "\n".join(f"-- group {g}, script seed {sp.seed}\n{sp.describe(k)}" for g, sp in enumerate(scripts))
            raise AssertionError(f"group fuzz seed {seed}, step {k}: {type(e).__name__}: {e}\n{text}") from e
    return world, compared
