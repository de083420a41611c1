// mgx_world_goal_areas.inc — C ABI: goal areas on the device — the first arrival of every robot in every area (the pass
// mgx_mission_tick_end enqueues beside the collision passes).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a pass computes: mgx_goal_areas.hip; the specification: include/mgx.h.  The host's side here: the table follows the
// world's robots under the rule of mgx_world_observers.inc (its rows are strided for the head-room of that rule, and only robots
// beyond it make it grow, the arrivals so far copied row by row), a pass is enqueued on the world's stream without a
// synchronisation or a read-back, and mgx_goal_areas_read is the call that waits.

static const char *const GOALS_OFF = "the goal areas are off (mgx_goal_areas_enable)";
static const char *const GOALS_UNSHARDED = "the goal areas run on unsharded worlds";
static constexpr uint64_t GOALS_MAX_TICK = 0xfffffffeull;  // tick + 1 travels in 32 bits, 0 is "never"
static constexpr size_t GOALS_MAX_STRIDE = (size_t)1 << 24;

static void goal_areas_drop(mgx_world *w) {  // switched off: the state goes with it
    mgx_world::GoalAreas &g = w->goals;
    g.enabled = false;
    g.recs.release(); g.first.release();
    g.n_areas = 0; g.stride = 0; g.n_sized = 0; g.clock = 0;
}

// the table for the robots the world has NOW, the shared radii complete: the robots so far keep their arrivals, the others start
// at "never".  While the robots fit the rows nothing moves
static int goal_areas_size(mgx_world *w) {
    mgx_world::GoalAreas &g = w->goals;
    const size_t R = w->robots.size(), stride = observers_room(w, R);
    if (R <= g.n_sized) return MGX_OK;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", GOALS_UNSHARDED);
    if (R > g.stride && stride > GOALS_MAX_STRIDE) return fail(MGX_ERR_NOMEM, "goal areas: %zu robots are more than the table holds", R);
    Outgrown out{w->stream};
    const int rc = observers_radii(w, out);
    if (rc != MGX_OK) return rc;
    if (R > g.stride) {  // longer rows: every cell "never", then the arrivals so far, row by row
        HIP_TRY(out.grow(g.first, stride, g.n_sized, 0, g.n_areas, g.stride));
        g.stride = (uint32_t)stride;
    }
    HIP_TRY(out.retire());
    g.n_sized = R;
    return MGX_OK;
}

// one pass at `tick` over device-resident positions [R][3] and alive bytes [R], enqueued on `s`; no launch while nobody is alive
static int goal_areas_pass(mgx_world *w, const float *pos_d, const uint8_t *alive_d, uint64_t tick, hipStream_t s) {
    mgx_world::GoalAreas &g = w->goals;
    if (tick > GOALS_MAX_TICK) return fail(MGX_ERR_INVALID, "goal areas: tick %llu is beyond what the table stores", (unsigned long long)tick);
    const int rc = goal_areas_size(w);
    if (rc != MGX_OK) return rc;
    const size_t R = w->robots.size();
    bool any_alive = false;
    for (size_t r = 0; r < R && !any_alive; r++) any_alive = observed(w->robots[r]);
    if (!any_alive) return MGX_OK;
    GoalAreasDev d{};  // (goal_areas_size has succeeded: the rows and the radii hold R robots)
    d.pos = pos_d; d.alive = alive_d; d.radius = w->obs.radius.p; d.areas = g.recs.p; d.first = g.first.p;
    d.stride = g.stride; d.stamp = (uint32_t)(tick + 1);
    d.n = (int)R; d.n_areas = (int)g.n_areas;
    HIP_TRY(launch_goal_areas_pass(d, s));
    return MGX_OK;
}

extern "C" {

int mgx_goal_areas_enable(mgx_world *w, const mgx_goal_area *areas, uint32_t n_areas, uint64_t next_tick) {
    MGX_ENTER(w);
    // (the arguments first: what is wrong with them is said whatever the world's state, and without a device)
    if (n_areas && !areas) return fail(MGX_ERR_INVALID, "null areas");
    if (n_areas > MGX_GOAL_AREAS_MAX) return fail(MGX_ERR_INVALID, "%u goal areas, at most %u", n_areas, (unsigned)MGX_GOAL_AREAS_MAX);
    if (next_tick > GOALS_MAX_TICK) return fail(MGX_ERR_INVALID, "next_tick beyond 2^32 - 2");
    // corners sorted per axis; centre and half extents in f32, every operation rounded on its own (host code never contracts)
    std::vector<GoalAreaRec> recs(n_areas);
    for (uint32_t a = 0; a < n_areas; a++) {
        float lo[2], hi[2];
        for (int q = 0; q < 2; q++) {
            const float u = areas[a].mins[q], v = areas[a].maxs[q];
            if (!std::isfinite(u) || !std::isfinite(v)) return fail(MGX_ERR_INVALID, "goal area %u: a corner is not finite", a);
            lo[q] = std::min(u, v);
            hi[q] = std::max(u, v);
        }
        recs[a].cx = (lo[0] + hi[0]) * 0.5f; recs[a].cz = (lo[1] + hi[1]) * 0.5f;
        recs[a].hx = (hi[0] - lo[0]) * 0.5f; recs[a].hz = (hi[1] - lo[1]) * 0.5f;
    }
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::GoalAreas &g = w->goals;
    if (n_areas == 0) {
        if (g.enabled) HIP_TRY(hipStreamSynchronize(w->stream));
        goal_areas_drop(w);
        return MGX_OK;
    }
    if (g.enabled) return fail(MGX_ERR_STATE, "the goal areas are on (switch them off before handing in other areas)");
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", GOALS_UNSHARDED);
    hipStream_t s = w->stream;
    goal_areas_drop(w);
    g.n_areas = n_areas;
    g.clock = next_tick;
    hipError_t e = g.recs.upload(recs, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the records went up from pageable memory)
    if (e != hipSuccess) { goal_areas_drop(w); return fail(MGX_ERR_HIP, "goal areas: %s", hipGetErrorString(e)); }
    const int rc = goal_areas_size(w);  // (a world without robots yet: the table comes with the first pass)
    if (rc != MGX_OK) { goal_areas_drop(w); return rc; }
    g.enabled = true;
    return MGX_OK;
}

int mgx_goal_areas_set_clock(mgx_world *w, uint64_t next_tick) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->goals.enabled) return fail(MGX_ERR_STATE, "%s", GOALS_OFF);
    if (next_tick > GOALS_MAX_TICK) return fail(MGX_ERR_INVALID, "next_tick beyond 2^32 - 2");
    w->goals.clock = next_tick;
    return MGX_OK;
}

int mgx_goal_areas_update(mgx_world *w, const float *positions_xyz, uint64_t tick) {
    ObserverInputs in;
    const int rc = observers_update_begin(w, w && w->goals.enabled, GOALS_OFF, GOALS_UNSHARDED, tick > GOALS_MAX_TICK ? "tick beyond 2^32 - 2" : nullptr,
                                          positions_xyz, nullptr, in);
    if (rc != MGX_OK || !in.flags) return rc;
    return goal_areas_pass(w, in.pos, in.flags, tick, w->stream);
}

int mgx_goal_areas_read(mgx_world *w, mgx_goal_arrival *arrivals, uint64_t capacity, uint64_t *n_total, uint32_t *per_area) {
    MGX_ENTER(w);
    if (!w || (!arrivals && capacity)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::GoalAreas &g = w->goals;
    if (!g.enabled) return fail(MGX_ERR_STATE, "%s", GOALS_OFF);
    MGX_CONFIRM(w);
    hipStream_t s = w->stream;
    // the table comes down row by row (robots that joined since the last pass have arrived nowhere) and is compacted here
    const size_t n = std::min(g.n_sized, (size_t)g.stride), A = g.n_areas;
    std::vector<uint32_t> first(A * n);
    for (size_t a = 0; a < A && n; a++)
        HIP_TRY(hipMemcpyAsync(first.data() + a * n, g.first.p + a * g.stride, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<mgx_goal_arrival> out;
    if (per_area) std::fill(per_area, per_area + A, 0u);
    for (size_t a = 0; a < A; a++)
        for (size_t r = 0; r < n; r++) {
            const uint32_t v = first[a * n + r];
            if (!v) continue;
            out.push_back(mgx_goal_arrival{(uint64_t)v - 1u, (int32_t)a, (int32_t)r});
            if (per_area) per_area[a]++;
        }
    std::sort(out.begin(), out.end(), [](const mgx_goal_arrival &x, const mgx_goal_arrival &y) {
        if (x.tick != y.tick) return x.tick < y.tick;
        if (x.robot != y.robot) return x.robot < y.robot;
        return x.area < y.area;
    });
    if (n_total) *n_total = out.size();
    if (capacity && capacity < out.size())
        return fail(MGX_ERR_INVALID, "room for %llu arrivals, %llu recorded", (unsigned long long)capacity, (unsigned long long)out.size());
    if (capacity && !out.empty()) memcpy(arrivals, out.data(), sizeof(mgx_goal_arrival) * out.size());
    return check_device_error(w);
}

int mgx_goal_areas_clear(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::GoalAreas &g = w->goals;
    if (!g.enabled) return fail(MGX_ERR_STATE, "%s", GOALS_OFF);
    if (g.first.p) HIP_TRY(hipMemsetAsync(g.first.p, 0, sizeof(uint32_t) * g.first.cap, w->stream));
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
