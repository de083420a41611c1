// mgx_world_planner.inc — C ABI: the global planner (mgx_planner_enable, mgx_plan_paths, mgx_plan_tree; mgx_plan_submit, _advance,
// _collect, _cancel, _pending and mgx_planner_set_tick_budget for plans that ride the stream).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a plan is: include/mgx.h; how a launch computes it: mgx_planner.hip.  The host's side here: the map goes up once
// (env_map_upload, shared with the robot-environment pass), a call sizes the trees for its requests, uploads one 64-byte state
// per request and launches slices of iterations_per_launch iterations until every state says DONE — one small read-back per slice.
// Requests that ride the stream live in a pool instead (mgx_world::Planner::Pool; its bookkeeping: mgx_plan_pool.h): submit writes
// a state into a slot's host-mapped record, advance enqueues one launch over the slots still running and records an event behind
// it, and collect reads the completion log the launches append to — no call of the three waits unless it is asked to.

static constexpr uint32_t PLAN_DEFAULT_NODES = 8192, PLAN_DEFAULT_SLICE = 1024, PLAN_MAX_NODES = 1u << 16;
static constexpr float PLAN_DEFAULT_HALF_EXTENT = 2000.f;
static const char *const PLAN_OFF = "the global planner is off (mgx_planner_enable)";

static void planner_drop(mgx_world *w) {
    mgx_world::Planner &p = w->planner;
    p.enabled = false;
    p.map.release();
    p.state.release(); p.x.release(); p.y.release(); p.cost.release(); p.parent.release(); p.path.release(); p.out.release();
    p.host_state.clear();
    p.pool.release();
}

// what a launch is handed apart from its arrays and its budget
static PlanDev plan_dev_params(const mgx_world::Planner &p) {
    const mgx_plan_params &q = p.params;
    PlanDev d{};
    d.map = p.map.d;
    d.step = (double)q.step_size;
    d.radius2 = (double)q.neighbourhood_radius * (double)q.neighbourhood_radius;
    d.half_extent = (double)q.sample_half_extent;
    d.smoothing_step = (double)q.smoothing_step;
    d.collision_radius = q.collision_radius;
    d.max_iterations = q.max_iterations; d.max_nodes = q.max_nodes;
    d.smoothing = q.smoothing_enabled ? 1 : 0;
    d.smoothing_max = q.smoothing_max_iterations;
    return d;
}

static bool plan_request_finite(const mgx_plan_request &r) {
    return std::isfinite(r.start[0]) && std::isfinite(r.start[1]) && std::isfinite(r.end[0]) && std::isfinite(r.end[1]);
}
static PlanState plan_initial_state(const mgx_plan_request &r) {
    PlanState st{};
    st.rng = r.wyrand_state;
    for (int k = 0; k < 2; k++) { st.start[k] = r.start[k]; st.end[k] = r.end[k]; }
    st.phase = PLAN_PHASE_INIT;
    st.goal = -1;
    return st;
}
static void plan_result_of(const PlanState &st, uint32_t first_point, mgx_plan_result &r) {
    const bool ok = st.status == MGX_PLAN_OK;
    r = mgx_plan_result{};
    r.status = st.status;
    r.first_point = first_point;
    r.n_points = ok ? st.path_len : 0u;
    r.n_nodes = st.n_nodes;
    r.iterations = st.iterations;
    r.smoothing_iterations = st.smooth_done;
    r.cost = ok ? st.cost : 0.0;
    r.wyrand_state = st.rng;
}

// ---- the pool ----------------------------------------------------------------------------------------------------------------------
template <class T>
static hipError_t plan_host_mapped(T **host, size_t count) {
    *host = nullptr;
    const hipError_t e = hipHostMalloc((void **)host, sizeof(T) * count, hipHostMallocMapped);
    if (e == hipSuccess) memset((void *)*host, 0, sizeof(T) * count);
    return e;
}
template <class T>
static hipError_t plan_dev_view(T *host, T **dev) {
    void *d = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&d, (void *)host, 0);
    *dev = (T *)d;
    return e;
}

// what the device has reported since the last look: the event behind the last slice (never waited for here), then the log
static void plan_pool_poll(mgx_world::Planner &p) {
    mgx_world::Planner::Pool &pl = p.pool;
    if (pl.ev && pl.ev_seq > pl.book.completed && hipEventQuery(pl.ev) == hipSuccess) pl.book.complete(pl.ev_seq);
    if (!pl.log) return;
    for (;;) {
        PlanLogEntry &e = pl.log[pl.log_taken % mgx_world::Planner::Pool::LOG_CAP];
        const unsigned long long ticket = __atomic_load_n(&e.ticket, __ATOMIC_ACQUIRE);
        if (!ticket) break;
        pl.book.finished(ticket, e.slices);
        __atomic_store_n(&e.ticket, 0ull, __ATOMIC_RELAXED);
        pl.log_taken += 1;
    }
}

static int plan_pool_add_block(mgx_world *w) {
    mgx_world::Planner &p = w->planner;
    mgx_world::Planner::Pool &pl = p.pool;
    const size_t S = PlanPoolBook::SLOTS_PER_BLOCK, cap = p.params.max_nodes, b = pl.blocks.size();
    if (b >= PlanPoolBook::MAX_BLOCKS) return fail(MGX_ERR_INVALID, "more than %u requests pending", PlanPoolBook::MAX_SLOTS);
    if (!pl.table) {
        HIP_TRY(plan_host_mapped(&pl.table, (size_t)PlanPoolBook::MAX_BLOCKS));
        HIP_TRY(plan_host_mapped(&pl.log, (size_t)mgx_world::Planner::Pool::LOG_CAP + 1));  // (the counter is the word behind the ring)
        pl.log_count = reinterpret_cast<unsigned int *>(pl.log + mgx_world::Planner::Pool::LOG_CAP);
        HIP_TRY(hipEventCreateWithFlags(&pl.ev, hipEventDisableTiming));
    }
    mgx_world::Planner::Pool::Block blk;
    const size_t f64s = 3 * S * cap, i32s = S * cap + S * (cap + 1);
    HIP_TRY(hipMalloc(&blk.dev, sizeof(double) * f64s + sizeof(int32_t) * i32s));
    char *host = nullptr;
    const hipError_t e = plan_host_mapped(&host, sizeof(PlanState) * S + sizeof(float) * 2 * S * (cap + 1));
    if (e != hipSuccess) { (void)hipFree(blk.dev); HIP_TRY(e); }
    blk.state = reinterpret_cast<PlanState *>(host);
    blk.out = reinterpret_cast<float *>(host + sizeof(PlanState) * S);
    pl.blocks.push_back(blk);  // (owned from here on)
    PlanBlockDev d{};
    d.x = (double *)blk.dev; d.y = d.x + S * cap; d.cost = d.y + S * cap;
    d.parent = (int32_t *)(d.cost + S * cap); d.path = d.parent + S * cap;
    HIP_TRY(plan_dev_view(blk.state, &d.state));
    HIP_TRY(plan_dev_view(blk.out, &d.out));
    pl.table[b] = d;
    pl.book.add_block();
    return MGX_OK;
}

// the list of the slots still running, in a buffer no launch in flight reads
static int plan_pool_write_list(mgx_world::Planner::Pool &pl) {
    using List = mgx_world::Planner::Pool::List;
    const size_t n = pl.book.n_running;
    int k = -1;
    for (size_t i = 0; i < pl.lists.size() && k < 0; i++)
        if (pl.lists[i].last_seq <= pl.book.completed && pl.lists[i].cap >= n) k = (int)i;
    if (k < 0) {
        List l;
        l.cap = std::max<size_t>(64, 2 * n);
        HIP_TRY(plan_host_mapped(&l.p, l.cap));
        pl.lists.push_back(l);
        k = (int)pl.lists.size() - 1;
    }
    PlanActive *out = pl.lists[(size_t)k].p;
    size_t m = 0;
    pl.book.for_running([&](uint32_t s, const PlanPoolBook::Slot &q) {
        PlanActive a{};
        a.ticket = q.ticket; a.slot = s; a.first_seq = (uint32_t)q.first_seq;
        if (m < n) out[m++] = a;
    });
    pl.cur = k;
    pl.cur_n = (uint32_t)m;
    pl.book.list_dirty = false;
    return MGX_OK;
}

// one slice for every request still running, enqueued behind whatever the stream holds; nothing running: nothing is launched
static int plan_pool_advance(mgx_world *w, uint32_t iterations) {
    mgx_world::Planner &p = w->planner;
    mgx_world::Planner::Pool &pl = p.pool;
    plan_pool_poll(p);
    if (pl.book.n_running == 0) return MGX_OK;
    if (pl.book.list_dirty || pl.cur < 0) {
        const int rc = plan_pool_write_list(pl);
        if (rc != MGX_OK) return rc;
    }
    PlanDev d = plan_dev_params(p);
    d.budget = iterations;
    PlanPoolDev pd{};
    HIP_TRY(plan_dev_view(pl.table, const_cast<PlanBlockDev **>(&pd.blocks)));
    HIP_TRY(plan_dev_view(pl.lists[(size_t)pl.cur].p, const_cast<PlanActive **>(&pd.active)));
    HIP_TRY(plan_dev_view(pl.log, &pd.log));
    HIP_TRY(plan_dev_view(pl.log_count, &pd.log_count));
    pd.log_cap = mgx_world::Planner::Pool::LOG_CAP;
    pd.slots_per_block = PlanPoolBook::SLOTS_PER_BLOCK;
    const uint64_t seq = pl.book.advance();
    pd.seq = (uint32_t)seq;
    pl.lists[(size_t)pl.cur].last_seq = seq;
    HIP_TRY(launch_plan_pool(d, pd, (int)pl.cur_n, w->stream));
    HIP_TRY(hipEventRecord(pl.ev, w->stream));
    pl.ev_seq = seq;
    return MGX_OK;
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
    if (p.pool.book.pending()) return fail(MGX_ERR_STATE, "%u requests are pending (mgx_plan_collect, mgx_plan_cancel)", p.pool.book.pending());
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
        if (!plan_request_finite(requests[i])) return fail(MGX_ERR_INVALID, "request %u: a coordinate is not finite", i);
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
    st.resize(N);
    for (size_t i = 0; i < N; i++) st[i] = plan_initial_state(requests[i]);
    HIP_TRY(hipMemcpyAsync(p.state.p, st.data(), sizeof(PlanState) * N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (pageable memory)
    PlanDev d = plan_dev_params(p);
    d.state = p.state.p; d.x = p.x.p; d.y = p.y.p; d.cost = p.cost.p; d.parent = p.parent.p; d.path = p.path.p; d.out = p.out.p;
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
        plan_result_of(st[i], (uint32_t)total, results[i]);
        total += results[i].n_points;
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

int mgx_plan_submit(mgx_world *w, uint32_t n, const mgx_plan_request *requests, uint64_t *tickets) {
    MGX_ENTER(w);
    if (!w || (n && (!requests || !tickets))) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the global planner runs on unsharded worlds");
    for (uint32_t i = 0; i < n; i++)
        if (!plan_request_finite(requests[i])) return fail(MGX_ERR_INVALID, "request %u: a coordinate is not finite", i);
    mgx_world::Planner::Pool &pl = p.pool;
    plan_pool_poll(p);  // (before a slot changes its tenant: what the log says of the one before is taken)
    if ((uint64_t)pl.book.pending() + n > PlanPoolBook::MAX_SLOTS) return fail(MGX_ERR_INVALID, "more than %u requests pending", PlanPoolBook::MAX_SLOTS);
    std::vector<uint32_t> slots;
    slots.reserve(n);
    while (slots.size() < n) {
        int s = pl.book.take_slot();
        if (s < 0) {
            const int rc = plan_pool_add_block(w);
            if (rc != MGX_OK) {
                for (size_t i = slots.size(); i-- > 0;) pl.book.give_back(slots[i]);
                return rc;
            }
            continue;
        }
        slots.push_back((uint32_t)s);
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t s = slots[i];
        pl.blocks[s / PlanPoolBook::SLOTS_PER_BLOCK].state[s % PlanPoolBook::SLOTS_PER_BLOCK] = plan_initial_state(requests[i]);
        tickets[i] = pl.book.submit(s);
    }
    return MGX_OK;
}

int mgx_plan_advance(mgx_world *w, uint32_t iterations) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (iterations == 0) return fail(MGX_ERR_INVALID, "a slice of 0 iterations");
    if (!w->planner.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    return plan_pool_advance(w, iterations);
}

int mgx_planner_set_tick_budget(mgx_world *w, uint32_t iterations) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    w->planner.pool.tick_budget = iterations;
    return MGX_OK;
}

int mgx_plan_collect(mgx_world *w, uint32_t flags, uint32_t capacity, mgx_plan_done *done, float *path_xy, uint32_t point_capacity,
                     uint32_t *n_done, uint32_t *n_points) {
    MGX_ENTER(w);
    if (!w || !n_done || !n_points || (capacity && !done) || (point_capacity && !path_xy)) return fail(MGX_ERR_INVALID, "null argument");
    if (flags & ~(uint32_t)MGX_PLAN_WAIT) return fail(MGX_ERR_INVALID, "unknown flags");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    mgx_world::Planner::Pool &pl = p.pool;
    if ((flags & MGX_PLAN_WAIT) && pl.ev && pl.ev_seq > pl.book.completed) {
        HIP_TRY(hipEventSynchronize(pl.ev));
        pl.book.complete(pl.ev_seq);
    }
    plan_pool_poll(p);
    const size_t cap = p.params.max_nodes;
    uint32_t nd = 0, np = 0, slices = 0, slot = 0;
    uint64_t ticket = 0;
    while (nd < capacity && pl.book.next_done(&ticket, &slices, &slot)) {
        const mgx_world::Planner::Pool::Block &b = pl.blocks[slot / PlanPoolBook::SLOTS_PER_BLOCK];
        const size_t i = slot % PlanPoolBook::SLOTS_PER_BLOCK;
        mgx_plan_done d{};
        plan_result_of(b.state[i], np, d.result);
        if (d.result.n_points > cap + 1) return fail(MGX_ERR_STATE, "ticket %llu: a path of %u points", (unsigned long long)ticket, d.result.n_points);
        if (d.result.n_points > point_capacity - np) break;  // (it stays for the next call)
        d.ticket = ticket;
        d.slices = slices;
        if (d.result.n_points) memcpy(path_xy + 2 * (size_t)np, b.out + 2 * i * (cap + 1), sizeof(float) * 2 * d.result.n_points);
        np += d.result.n_points;
        done[nd++] = d;
        pl.book.pop_done();
    }
    *n_done = nd;
    *n_points = np;
    return MGX_OK;
}

int mgx_plan_cancel(mgx_world *w, uint64_t ticket) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    plan_pool_poll(w->planner);
    if (!w->planner.pool.book.cancel(ticket)) return fail(MGX_ERR_INVALID, "ticket %llu is not pending", (unsigned long long)ticket);
    return MGX_OK;
}

int mgx_plan_pending(mgx_world *w, uint32_t *n) {
    MGX_ENTER_SCHEDULE(w);
    if (!w || !n) return fail(MGX_ERR_INVALID, "null argument");
    *n = w->planner.pool.book.pending();
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
