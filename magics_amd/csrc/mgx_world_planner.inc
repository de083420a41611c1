// mgx_world_planner.inc — C ABI: the global planner (mgx_planner_enable, mgx_plan_paths, mgx_plan_tree).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a plan is: include/mgx.h; how a launch computes it: mgx_planner.hip.  The host's side here: the map goes up once
// (env_map_upload, shared with the robot-environment pass), a call sizes the trees for its requests, uploads one 64-byte state
// per request and launches slices of iterations_per_launch iterations until every state says DONE — one small read-back per slice.

static constexpr uint32_t PLAN_DEFAULT_NODES = 8192, PLAN_DEFAULT_SLICE = 1024, PLAN_MAX_NODES = 1u << 16;
static constexpr float PLAN_DEFAULT_HALF_EXTENT = 2000.f;
static const char *const PLAN_OFF = "the global planner is off (mgx_planner_enable)";

static void planner_drop(mgx_world *w) {
    mgx_world::Planner &p = w->planner;
    p.enabled = false;
    p.map.release();
    p.state.release(); p.x.release(); p.y.release(); p.cost.release(); p.parent.release(); p.path.release(); p.out.release();
    p.host_state.clear();
}

extern "C" {

int mgx_planner_enable(mgx_world *w, const mgx_env_desc *env, const mgx_plan_params *params) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Planner &p = w->planner;
    if (!env) {
        if (p.enabled) HIP_TRY(hipStreamSynchronize(w->stream));
        planner_drop(w);
        return MGX_OK;
    }
    if (!params) return fail(MGX_ERR_INVALID, "null params");
    mgx_plan_params q = *params;
    const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
    const auto not_negative = [](float v) { return std::isfinite(v) && v >= 0.f; };
    if (!positive(q.step_size) || !positive(q.neighbourhood_radius) || (q.smoothing_enabled && !positive(q.smoothing_step)))
        return fail(MGX_ERR_INVALID, "step_size, neighbourhood_radius and smoothing_step must be positive and finite");
    if (!not_negative(q.collision_radius) || !not_negative(q.sample_half_extent))
        return fail(MGX_ERR_INVALID, "collision_radius and sample_half_extent must be finite and not negative");
    if (q.max_nodes > PLAN_MAX_NODES) return fail(MGX_ERR_INVALID, "max_nodes beyond %u", PLAN_MAX_NODES);
    if (q.sample_half_extent == 0.f) q.sample_half_extent = PLAN_DEFAULT_HALF_EXTENT;
    if (q.max_nodes == 0) q.max_nodes = PLAN_DEFAULT_NODES;
    if (q.iterations_per_launch == 0) q.iterations_per_launch = PLAN_DEFAULT_SLICE;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the global planner runs on unsharded worlds");
    if (p.enabled) HIP_TRY(hipStreamSynchronize(w->stream));
    planner_drop(w);
    const int rc = env_map_upload(w, env, p.map);
    if (rc != MGX_OK) { planner_drop(w); return rc; }
    p.params = q;
    p.enabled = true;
    return MGX_OK;
}

int mgx_plan_paths(mgx_world *w, uint32_t n, const mgx_plan_request *requests, mgx_plan_result *results, float *path_xy,
                   uint32_t point_capacity, uint32_t *n_points) {
    MGX_ENTER(w);
    if (!w || !n_points || (n && (!requests || !results)) || (!path_xy && point_capacity)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the global planner runs on unsharded worlds");
    for (uint32_t i = 0; i < n; i++)
        for (int q = 0; q < 2; q++)
            if (!std::isfinite(requests[i].start[q]) || !std::isfinite(requests[i].end[q]))
                return fail(MGX_ERR_INVALID, "request %u: a coordinate is not finite", i);
    if (n > (1u << 20)) return fail(MGX_ERR_INVALID, "more than 2^20 requests");
    if (n == 0) { *n_points = 0; p.host_state.clear(); return MGX_OK; }
    MGX_CONFIRM(w);
    const mgx_plan_params &q = p.params;
    const size_t cap = q.max_nodes, N = n;
    hipStream_t s = w->stream;
    HIP_TRY(p.state.reserve(N));
    HIP_TRY(p.x.reserve(N * cap));
    HIP_TRY(p.y.reserve(N * cap));
    HIP_TRY(p.cost.reserve(N * cap));
    HIP_TRY(p.parent.reserve(N * cap));
    HIP_TRY(p.path.reserve(N * (cap + 1)));
    HIP_TRY(p.out.reserve(2 * N * (cap + 1)));
    std::vector<PlanState> &st = p.host_state;
    st.assign(N, PlanState{});
    for (size_t i = 0; i < N; i++) {
        st[i].rng = requests[i].wyrand_state;
        for (int k = 0; k < 2; k++) { st[i].start[k] = requests[i].start[k]; st[i].end[k] = requests[i].end[k]; }
        st[i].phase = PLAN_PHASE_INIT;
        st[i].goal = -1;
    }
    HIP_TRY(hipMemcpyAsync(p.state.p, st.data(), sizeof(PlanState) * N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (pageable memory)
    PlanDev d{};
    d.map = p.map.d;
    d.state = p.state.p; d.x = p.x.p; d.y = p.y.p; d.cost = p.cost.p; d.parent = p.parent.p; d.path = p.path.p; d.out = p.out.p;
    d.step = (double)q.step_size;
    d.radius2 = (double)q.neighbourhood_radius * (double)q.neighbourhood_radius;
    d.half_extent = (double)q.sample_half_extent;
    d.smoothing_step = (double)q.smoothing_step;
    d.collision_radius = q.collision_radius;
    d.max_iterations = q.max_iterations; d.max_nodes = q.max_nodes;
    d.smoothing = q.smoothing_enabled ? 1 : 0;
    d.smoothing_max = q.smoothing_max_iterations;
    d.budget = q.iterations_per_launch;
    // every launch takes `budget` off what a request has left (growth, then smoothing), and one more finishes it
    const uint64_t most = ((uint64_t)q.max_iterations + q.smoothing_max_iterations) / q.iterations_per_launch + 3;
    bool done = false;
    for (uint64_t l = 0; l < most && !done; l++) {
        HIP_TRY(launch_plan(d, (int)n, s));
        HIP_TRY(hipMemcpyAsync(st.data(), p.state.p, sizeof(PlanState) * N, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        done = true;
        for (size_t i = 0; i < N; i++) done = done && st[i].phase == PLAN_PHASE_DONE;
    }
    if (!done) return fail(MGX_ERR_STATE, "the planner's launches ran out before every request had ended");
    uint64_t total = 0;
    for (size_t i = 0; i < N; i++) {
        const bool ok = st[i].status == MGX_PLAN_OK;
        mgx_plan_result &r = results[i];
        r = mgx_plan_result{};
        r.status = st[i].status;
        r.first_point = (uint32_t)total;
        r.n_points = ok ? st[i].path_len : 0u;
        r.n_nodes = st[i].n_nodes;
        r.iterations = st[i].iterations;
        r.cost = ok ? st[i].cost : 0.0;
        r.wyrand_state = st[i].rng;
        total += r.n_points;
    }
    if (total > 0xffffffffull) return fail(MGX_ERR_INVALID, "more than 2^32 points");
    *n_points = (uint32_t)total;
    if (total > point_capacity) return fail(MGX_ERR_INVALID, "room for %u points, the paths have %llu", point_capacity, (unsigned long long)total);
    for (size_t i = 0; i < N; i++)
        if (results[i].n_points)
            HIP_TRY(hipMemcpyAsync(path_xy + 2 * (size_t)results[i].first_point, p.out.p + 2 * i * (cap + 1), sizeof(float) * 2 * results[i].n_points,
                                   hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return check_device_error(w);
}

int mgx_plan_tree(mgx_world *w, uint32_t request, uint32_t capacity, double *xy, int32_t *parent, double *cost, uint32_t *n_nodes) {
    MGX_ENTER(w);
    if (!w || !n_nodes) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (request >= p.host_state.size()) return fail(MGX_ERR_INVALID, "request %u: the last mgx_plan_paths had %zu", request, p.host_state.size());
    const size_t cap = p.params.max_nodes, nn = p.host_state[request].n_nodes, m = std::min<size_t>(std::min<size_t>(nn, capacity), cap);
    *n_nodes = (uint32_t)nn;
    if (m == 0) return MGX_OK;
    hipStream_t s = w->stream;
    if (xy) {
        std::vector<double> a(m), b(m);
        HIP_TRY(hipMemcpyAsync(a.data(), p.x.p + request * cap, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(b.data(), p.y.p + request * cap, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t k = 0; k < m; k++) { xy[2 * k] = a[k]; xy[2 * k + 1] = b[k]; }
    }
    if (parent) HIP_TRY(hipMemcpyAsync(parent, p.parent.p + request * cap, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
    if (cost) HIP_TRY(hipMemcpyAsync(cost, p.cost.p + request * cap, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
