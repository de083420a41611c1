// mgx_world_planner.inc — C ABI: the global planner (mgx_planner_enable, mgx_plan_paths, mgx_plan_tree; mgx_plan_submit, _advance,
// _collect, _cancel, _pending and mgx_planner_set_tick_budget for plans that ride the stream; mgx_planner_set_group_params,
// mgx_planner_group_params and the _groups forms of paths and submit for a parameter set per robot group).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a plan is: include/mgx.h; how a launch computes it: mgx_planner.hip.  The host's side here: the map goes up once
// (env_map_upload, shared with the robot-environment pass), and every request lives in a slot of a pool (mgx_world::Planner::Pool;
// its bookkeeping: mgx_plan_pool.h).  ONE lifecycle: plan_pool_submit writes a state into a slot's host-mapped record,
// plan_pool_advance enqueues one launch over the slots still running with an event behind it, plan_pool_poll learns what has ended
// from the completion log the launches append to, plan_pool_result reads it in place.  mgx_plan_submit / _advance / _collect are
// those steps for requests that ride the stream; mgx_plan_paths is the same steps with a wait behind every slice, on a pool of
// its own (Planner::call: no ticket or slice number of a pending request moves).

static constexpr uint32_t PLAN_DEFAULT_NODES = 8192, PLAN_DEFAULT_SLICE = 1024, PLAN_MAX_NODES = 1u << 16;
static constexpr float PLAN_DEFAULT_HALF_EXTENT = 2000.f;
static const char *const PLAN_OFF = "the global planner is off (mgx_planner_enable)";

// the pool of mgx_plan_paths goes with the last call's trees (the stream is synchronised); the next call builds one of its size
static void plan_call_drop(mgx_world::Planner &p) {
    p.call_slots.clear();
    p.call.release();
    p.call.book.reset(1, 1);
}
static void planner_drop(mgx_world *w) {
    mgx_world::Planner &p = w->planner;
    p.enabled = false;
    p.map.release();
    p.pool.release();
    p.sets.release();
    plan_call_drop(p);
}

// the fields a request may have of its own, as the device reads them: a row of the table of sets, and the same fields of a launch
static PlanSetDev plan_set_dev(const mgx_plan_params &q) {
    PlanSetDev g{};
    g.step = (double)q.step_size;
    g.radius2 = (double)q.neighbourhood_radius * (double)q.neighbourhood_radius;
    g.half_extent = (double)q.sample_half_extent;
    g.smoothing_step = (double)q.smoothing_step;
    g.collision_radius = q.collision_radius;
    g.max_iterations = q.max_iterations;
    g.smoothing_max = q.smoothing_max_iterations;
    g.smoothing = q.smoothing_enabled ? 1 : 0;
    return g;
}
// what a launch is handed apart from its arrays and its budget
static PlanDev plan_dev_params(const mgx_world::Planner &p) {
    const PlanSetDev g = plan_set_dev(p.params);
    PlanDev d{};
    d.map = p.map.d;
    d.step = g.step; d.radius2 = g.radius2; d.half_extent = g.half_extent; d.smoothing_step = g.smoothing_step;
    d.collision_radius = g.collision_radius;
    d.max_iterations = g.max_iterations; d.max_nodes = p.params.max_nodes;
    d.smoothing = g.smoothing;
    d.smoothing_max = g.smoothing_max;
    return d;
}
// the parameters a request of `group` runs under: its own set, or the world's
static const mgx_plan_params &plan_params_of(const mgx_world::Planner &p, uint32_t group) {
    const uint32_t k = p.sets.of(group);
    return k ? p.sets.params[k - 1] : p.params;
}

// the value checks of a parameter struct (mgx_planner_enable, mgx_planner_set_group_params)
static int plan_params_check(const mgx_plan_params &q) {
    const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
    const auto not_negative = [](float v) { return std::isfinite(v) && v >= 0.f; };
    if (!positive(q.step_size) || !positive(q.neighbourhood_radius) || (q.smoothing_enabled && !positive(q.smoothing_step)))
        return fail(MGX_ERR_INVALID, "step_size, neighbourhood_radius and smoothing_step must be positive and finite");
    if (!not_negative(q.collision_radius) || !not_negative(q.sample_half_extent))
        return fail(MGX_ERR_INVALID, "collision_radius and sample_half_extent must be finite and not negative");
    if (q.max_nodes > PLAN_MAX_NODES) return fail(MGX_ERR_INVALID, "max_nodes beyond %u", PLAN_MAX_NODES);
    return MGX_OK;
}

static bool plan_request_finite(const mgx_plan_request &r) {
    return std::isfinite(r.start[0]) && std::isfinite(r.start[1]) && std::isfinite(r.end[0]) && std::isfinite(r.end[1]);
}
static PlanState plan_initial_state(const mgx_plan_request &r, uint32_t set) {
    PlanState st{};
    st.set = set;
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

using PlanPool = mgx_world::Planner::Pool;

// what the device has reported since the last look: the event behind the last slice (waited for only if `wait`), then the log
static int plan_pool_poll(PlanPool &pl, bool wait = false) {
    if (pl.ev && pl.ev_seq > pl.book.completed) {
        if (wait) HIP_TRY(hipEventSynchronize(pl.ev));
        if (wait || hipEventQuery(pl.ev) == hipSuccess) pl.book.complete(pl.ev_seq);
    }
    if (!pl.log) return MGX_OK;
    for (;;) {
        PlanLogEntry &e = pl.log[pl.log_taken % pl.log_cap];
        const unsigned long long ticket = __atomic_load_n(&e.ticket, __ATOMIC_ACQUIRE);
        if (!ticket) break;
        pl.book.finished(ticket, e.slices);
        __atomic_store_n(&e.ticket, 0ull, __ATOMIC_RELAXED);
        pl.log_taken += 1;
    }
    return MGX_OK;
}

static int plan_pool_add_block(PlanPool &pl, const mgx_plan_params &q, hipStream_t stream) {
    const size_t S = pl.book.slots_per_block, cap = q.max_nodes, b = pl.blocks.size();
    if (b >= pl.book.max_blocks) return fail(MGX_ERR_INVALID, "more than %u requests pending", pl.book.max_slots());
    if (!pl.table) {
        // more entries than can be unread, and a power of two: the device's 32-bit counter and the host's 64-bit one agree for ever
        for (pl.log_cap = 1; pl.log_cap < 2 * pl.book.max_slots();) pl.log_cap *= 2;
        HIP_TRY(plan_host_mapped(&pl.table, (size_t)pl.book.max_blocks));
        HIP_TRY(plan_host_mapped(&pl.log, (size_t)pl.log_cap));
        // the counter of claimed entries is the device's alone: in device memory, or workgroups that end together queue up for one
        // word across the bus (1 us each, profiles/global_planner.md); zeroed on the launches' stream: a submit waits for nothing
        HIP_TRY(hipMalloc((void **)&pl.log_count, sizeof(unsigned int)));
        HIP_TRY(hipMemsetAsync(pl.log_count, 0, sizeof(unsigned int), stream));
        HIP_TRY(hipEventCreateWithFlags(&pl.ev, hipEventDisableTiming));
    }
    PlanPool::Block blk;
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

// n requests into n slots that nothing in flight can touch (blocks are added as needed; on failure what was taken goes back): each
// slot gets its request's initial state and a ticket (book.slots[slot].ticket)
static int plan_pool_submit(PlanPool &pl, const mgx_world::Planner &p, hipStream_t stream, uint32_t n, const mgx_plan_request *requests,
                            const uint32_t *groups, std::vector<uint32_t> &slots) {
    const mgx_plan_params &q = p.params;
    (void)plan_pool_poll(pl);  // (before a slot changes its tenant: what the log says of the one before is taken)
    slots.clear();
    slots.reserve(n);
    while (slots.size() < n) {
        const int s = pl.book.take_slot();
        if (s >= 0) { slots.push_back((uint32_t)s); continue; }
        const int rc = plan_pool_add_block(pl, q, stream);
        if (rc != MGX_OK) {
            for (size_t i = slots.size(); i-- > 0;) pl.book.give_back(slots[i]);
            slots.clear();
            return rc;
        }
    }
    if (pl.slot_group.size() < pl.book.slots.size()) { pl.slot_group.resize(pl.book.slots.size(), 0u); pl.slot_set.resize(pl.book.slots.size(), 0u); }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t group = groups ? groups[i] : 0u;
        const uint32_t set = p.sets.of(group);
        pl.blocks[slots[i] / pl.book.slots_per_block].state[slots[i] % pl.book.slots_per_block] = plan_initial_state(requests[i], set);
        pl.slot_group[slots[i]] = group;
        pl.slot_set[slots[i]] = set;
        (void)pl.book.submit(slots[i]);
    }
    return MGX_OK;
}

// the result of the request that ended in `slot`, and its points: both are read in place
static int plan_pool_result(const PlanPool &pl, uint32_t slot, size_t cap, uint32_t first_point, mgx_plan_result &r) {
    plan_result_of(pl.blocks[slot / pl.book.slots_per_block].state[slot % pl.book.slots_per_block], first_point, r);
    return r.n_points <= cap + 1 ? MGX_OK : fail(MGX_ERR_STATE, "slot %u: a path of %u points", slot, r.n_points);
}
static void plan_pool_points(const PlanPool &pl, uint32_t slot, size_t cap, const mgx_plan_result &r, float *path_xy) {
    const float *from = pl.blocks[slot / pl.book.slots_per_block].out + 2 * (size_t)(slot % pl.book.slots_per_block) * (cap + 1);
    if (r.n_points) memcpy(path_xy + 2 * (size_t)r.first_point, from, sizeof(float) * 2 * r.n_points);
}

// the list of the slots still running, in a buffer no launch in flight reads
static int plan_pool_write_list(PlanPool &pl) {
    using List = PlanPool::List;
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
    bool sets = false;
    pl.book.for_running([&](uint32_t s, const PlanPoolBook::Slot &q) {
        PlanActive a{};
        a.ticket = q.ticket; a.slot = s; a.first_seq = (uint32_t)q.first_seq;
        if (m < n) out[m++] = a;
        sets = sets || pl.slot_set[s] != 0;
    });
    pl.cur_sets = sets;
    pl.cur = k;
    pl.cur_n = (uint32_t)m;
    pl.book.list_dirty = false;
    return MGX_OK;
}

// one slice for every request of the pool still running, enqueued behind whatever the stream holds; nothing running: nothing is launched
static int plan_pool_advance(PlanPool &pl, const mgx_world::Planner &p, hipStream_t stream, uint32_t iterations) {
    (void)plan_pool_poll(pl);
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
    pd.log_count = pl.log_count;
    pd.log_cap = pl.log_cap;
    pd.slots_per_block = pl.book.slots_per_block;
    pd.sets = pl.cur_sets ? p.sets.dev : nullptr;
    const uint64_t seq = pl.book.seq + 1;
    pd.seq = (uint32_t)seq;
    HIP_TRY(launch_plan_pool(d, pd, (int)pl.cur_n, stream));
    (void)pl.book.advance();  // (a launch that was refused is no advance: nothing of it is in flight)
    pl.lists[(size_t)pl.cur].last_seq = seq;
    HIP_TRY(hipEventRecord(pl.ev, stream));
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
    const int rc_check = plan_params_check(q);
    if (rc_check != MGX_OK) return rc_check;
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
    return mgx_plan_paths_groups(w, n, requests, nullptr, results, path_xy, point_capacity, n_points);
}

int mgx_plan_paths_groups(mgx_world *w, uint32_t n, const mgx_plan_request *requests, const uint32_t *groups, mgx_plan_result *results,
                          float *path_xy, uint32_t point_capacity, uint32_t *n_points) {
    MGX_ENTER(w);
    if (!w || !n_points || (n && (!requests || !results)) || (!path_xy && point_capacity)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the global planner runs on unsharded worlds");
    for (uint32_t i = 0; i < n; i++)
        if (!plan_request_finite(requests[i])) return fail(MGX_ERR_INVALID, "request %u: a coordinate is not finite", i);
    for (uint32_t i = 0; groups && i < n; i++)
        if (groups[i] >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "request %u: group %u beyond %u", i, groups[i], MGX_GROUPS_MAX - 1);
    if (n > (1u << 20)) return fail(MGX_ERR_INVALID, "more than 2^20 requests");
    if (n == 0) { *n_points = 0; p.call_slots.clear(); return MGX_OK; }
    MGX_CONFIRM(w);
    const mgx_plan_params &q = p.params;
    PlanPool &pl = p.call;
    // nothing of this pool is in flight between two calls: one that needs more slots builds it again, with a quarter to spare
    if (n > pl.book.slots_per_block) {
        HIP_TRY(hipStreamSynchronize(w->stream));
        plan_call_drop(p);
        pl.book.reset(n + n / 4, 1);
    }
    int rc = plan_pool_submit(pl, p, w->stream, n, requests, groups, p.call_slots);
    // every launch takes `budget` off what a request has left (growth, then smoothing), and one more finishes it: the longest a
    // request of these groups can take
    uint64_t longest = (uint64_t)q.max_iterations + q.smoothing_max_iterations;
    for (uint32_t i = 0; groups && i < n; i++) {
        const mgx_plan_params &g = plan_params_of(p, groups[i]);
        longest = std::max(longest, (uint64_t)g.max_iterations + g.smoothing_max_iterations);
    }
    const uint64_t most = longest / q.iterations_per_launch + 3;
    for (uint64_t l = 0; l < most && rc == MGX_OK && pl.book.n_running; l++) {
        rc = plan_pool_advance(pl, p, w->stream, q.iterations_per_launch);
        if (rc == MGX_OK) rc = plan_pool_poll(pl, true);
    }
    if (rc != MGX_OK) {  // an allocation, a launch or a wait failed: the pool goes, and a smaller call can build its own
        (void)hipStreamSynchronize(w->stream);
        plan_call_drop(p);
        (void)hipGetLastError();  // (the failure has been reported: the next launch's check does not find it again)
        return rc;
    }
    if (pl.book.n_running) rc = fail(MGX_ERR_STATE, "the planner's launches ran out before every request had ended");
    // the slots are given up; what is in them stays until the next call takes them (mgx_plan_tree)
    for (const uint32_t s : p.call_slots) (void)pl.book.cancel(pl.book.slots[s].ticket);
    pl.book.complete(pl.book.completed);
    if (rc != MGX_OK) return rc;
    const size_t cap = q.max_nodes;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        rc = plan_pool_result(pl, p.call_slots[i], cap, (uint32_t)total, results[i]);
        if (rc != MGX_OK) return rc;
        total += results[i].n_points;
    }
    if (total > 0xffffffffull) return fail(MGX_ERR_INVALID, "more than 2^32 points");
    *n_points = (uint32_t)total;
    if (total > point_capacity) return fail(MGX_ERR_INVALID, "room for %u points, the paths have %llu", point_capacity, (unsigned long long)total);
    for (uint32_t i = 0; i < n; i++) plan_pool_points(pl, p.call_slots[i], cap, results[i], path_xy);
    return check_device_error(w);
}

int mgx_plan_tree(mgx_world *w, uint32_t request, uint32_t capacity, double *xy, int32_t *parent, double *cost, uint32_t *n_nodes) {
    MGX_ENTER(w);
    if (!w || !n_nodes) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (request >= p.call_slots.size()) return fail(MGX_ERR_INVALID, "request %u: the last mgx_plan_paths had %zu", request, p.call_slots.size());
    const size_t slot = p.call_slots[request];  // (the call's pool is one block: the slot is the index into its arrays)
    const PlanBlockDev &b = p.call.table[0];
    const size_t cap = p.params.max_nodes, nn = p.call.blocks[0].state[slot].n_nodes, m = std::min<size_t>(std::min<size_t>(nn, capacity), cap);
    *n_nodes = (uint32_t)nn;
    if (m == 0) return MGX_OK;
    hipStream_t s = w->stream;
    if (xy) {
        std::vector<double> x(m), y(m);
        HIP_TRY(hipMemcpyAsync(x.data(), b.x + slot * cap, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(y.data(), b.y + slot * cap, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t k = 0; k < m; k++) { xy[2 * k] = x[k]; xy[2 * k + 1] = y[k]; }
    }
    if (parent) HIP_TRY(hipMemcpyAsync(parent, b.parent + slot * cap, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
    if (cost) HIP_TRY(hipMemcpyAsync(cost, b.cost + slot * cap, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGX_OK;
}

int mgx_plan_submit(mgx_world *w, uint32_t n, const mgx_plan_request *requests, uint64_t *tickets) {
    return mgx_plan_submit_groups(w, n, requests, nullptr, tickets);
}

int mgx_plan_submit_groups(mgx_world *w, uint32_t n, const mgx_plan_request *requests, const uint32_t *groups, uint64_t *tickets) {
    MGX_ENTER(w);
    if (!w || (n && (!requests || !tickets))) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the global planner runs on unsharded worlds");
    for (uint32_t i = 0; i < n; i++)
        if (!plan_request_finite(requests[i])) return fail(MGX_ERR_INVALID, "request %u: a coordinate is not finite", i);
    for (uint32_t i = 0; groups && i < n; i++)
        if (groups[i] >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "request %u: group %u beyond %u", i, groups[i], MGX_GROUPS_MAX - 1);
    PlanPool &pl = p.pool;
    if ((uint64_t)pl.book.pending() + n > pl.book.max_slots()) return fail(MGX_ERR_INVALID, "more than %u requests pending", pl.book.max_slots());
    std::vector<uint32_t> slots;
    const int rc = plan_pool_submit(pl, p, w->stream, n, requests, groups, slots);
    if (rc != MGX_OK) return rc;
    for (uint32_t i = 0; i < n; i++) tickets[i] = pl.book.slots[slots[i]].ticket;
    return MGX_OK;
}

int mgx_plan_advance(mgx_world *w, uint32_t iterations) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (iterations == 0) return fail(MGX_ERR_INVALID, "a slice of 0 iterations");
    if (!w->planner.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    return plan_pool_advance(w->planner.pool, w->planner, w->stream, iterations);
}

int mgx_planner_set_tick_budget(mgx_world *w, uint32_t iterations) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    w->planner.tick_budget = iterations;
    return MGX_OK;
}

int mgx_plan_collect(mgx_world *w, uint32_t flags, uint32_t capacity, mgx_plan_done *done, float *path_xy, uint32_t point_capacity,
                     uint32_t *n_done, uint32_t *n_points) {
    MGX_ENTER(w);
    if (!w || !n_done || !n_points || (capacity && !done) || (point_capacity && !path_xy)) return fail(MGX_ERR_INVALID, "null argument");
    if (flags & ~(uint32_t)MGX_PLAN_WAIT) return fail(MGX_ERR_INVALID, "unknown flags");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    PlanPool &pl = p.pool;
    const int rc_poll = plan_pool_poll(pl, (flags & MGX_PLAN_WAIT) != 0);
    if (rc_poll != MGX_OK) return rc_poll;
    const size_t cap = p.params.max_nodes;
    uint32_t nd = 0, np = 0, slices = 0, slot = 0;
    uint64_t ticket = 0;
    while (nd < capacity && pl.book.next_done(&ticket, &slices, &slot)) {
        mgx_plan_done d{};
        const int rc = plan_pool_result(pl, slot, cap, np, d.result);
        if (rc != MGX_OK) return rc;
        if (d.result.n_points > point_capacity - np) break;  // (it stays for the next call)
        d.ticket = ticket;
        d.slices = slices;
        d.group = pl.slot_group[slot];
        plan_pool_points(pl, slot, cap, d.result, path_xy);
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
    (void)plan_pool_poll(w->planner.pool);
    if (!w->planner.pool.book.cancel(ticket)) return fail(MGX_ERR_INVALID, "ticket %llu is not pending", (unsigned long long)ticket);
    return MGX_OK;
}

int mgx_planner_set_group_params(mgx_world *w, uint32_t group, const mgx_plan_params *params) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Planner &p = w->planner;
    if (!p.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (group >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "group %u beyond %u", group, MGX_GROUPS_MAX - 1);
    mgx_plan_params q = params ? *params : p.params;
    if (params) {
        const int rc = plan_params_check(q);
        if (rc != MGX_OK) return rc;
        if ((q.max_nodes && q.max_nodes != p.params.max_nodes) || (q.iterations_per_launch && q.iterations_per_launch != p.params.iterations_per_launch))
            return fail(MGX_ERR_INVALID, "max_nodes and iterations_per_launch are the launch's: 0, or the world's %u and %u", p.params.max_nodes,
                        p.params.iterations_per_launch);
        if (q.sample_half_extent == 0.f) q.sample_half_extent = PLAN_DEFAULT_HALF_EXTENT;
        q.max_nodes = p.params.max_nodes;
        q.iterations_per_launch = p.params.iterations_per_launch;
    }
    if (p.pool.book.pending())
        return fail(MGX_ERR_STATE, "%u requests are pending (mgx_plan_collect, mgx_plan_cancel): a set does not change under them", p.pool.book.pending());
    mgx_world::Planner::Sets &s = p.sets;
    if (!params) {
        if (s.of(group)) s.set_of[group] = 0;
        return MGX_OK;
    }
    // the group's row: the one it had, or a new one — in a table that grows by doubling (nothing in flight reads it: no request
    // pends, and mgx_plan_paths leaves none running)
    const bool fresh = s.row_of.empty() || s.row_of[group] == 0;
    const size_t rows = s.params.size() + (fresh ? 1 : 0);
    if (rows > s.dev_cap) {
        size_t cap = std::max<size_t>(16, s.dev_cap);
        while (cap < rows) cap *= 2;
        PlanSetDev *grown = nullptr;
        HIP_TRY(hipStreamSynchronize(w->stream));
        HIP_TRY(hipMalloc((void **)&grown, sizeof(PlanSetDev) * cap));
        if (s.dev) {
            const hipError_t e = hipMemcpyAsync(grown, s.dev, sizeof(PlanSetDev) * s.params.size(), hipMemcpyDeviceToDevice, w->stream);
            if (e != hipSuccess) { (void)hipFree(grown); HIP_TRY(e); }
            HIP_TRY(hipStreamSynchronize(w->stream));
            (void)hipFree(s.dev);
        }
        s.dev = grown;
        s.dev_cap = cap;
    }
    const size_t row = fresh ? s.params.size() : s.row_of[group] - 1;
    const PlanSetDev g = plan_set_dev(q);
    HIP_TRY(hipMemcpyAsync(s.dev + row, &g, sizeof(g), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));  // (the row is read from this frame)
    if (s.row_of.empty()) { s.row_of.assign(MGX_GROUPS_MAX, 0u); s.set_of.assign(MGX_GROUPS_MAX, 0u); }
    if (fresh) { s.params.push_back(q); s.row_of[group] = (uint32_t)s.params.size(); }
    else s.params[row] = q;
    s.set_of[group] = s.row_of[group];
    return MGX_OK;
}

int mgx_planner_group_params(mgx_world *w, uint32_t group, mgx_plan_params *out) {
    MGX_ENTER_SCHEDULE(w);
    if (!w || !out) return fail(MGX_ERR_INVALID, "null argument");
    if (!w->planner.enabled) return fail(MGX_ERR_STATE, "%s", PLAN_OFF);
    if (group >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "group %u beyond %u", group, MGX_GROUPS_MAX - 1);
    *out = plan_params_of(w->planner, group);
    return MGX_OK;
}

int mgx_plan_pending(mgx_world *w, uint32_t *n) {
    MGX_ENTER_SCHEDULE(w);
    if (!w || !n) return fail(MGX_ERR_INVALID, "null argument");
    *n = w->planner.pool.book.pending();
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
