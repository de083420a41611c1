// mgx_world_collisions.inc — C ABI: robot-robot and robot-environment collision bookkeeping on the device (the passes
// mgx_mission_tick_end enqueues).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a pass computes and how its state is kept: mgx_collisions.hip.  The host's side here: the arrays follow the world's robots
// (ids never change, so commit / mgx_robot_remove move nothing: robots that join make the per-robot arrays and the stride of the
// pair bits grow, and the bits are set again from the pair list), a pass is enqueued on the world's stream without a
// synchronisation or a read-back, and mgx_collisions_read is the one call that waits.

// What a read call hands out, for either log (32-byte records of the same layout on both sides).  The log only grows and every
// pass enqueued so far is complete: what was fetched before keeps its place, the rest is put in `less` order — which lane won
// an atomic never shows.  per_robot: robots that joined since the last pass have no contact yet.
template <class Event, class DevEvent, class Less>
static int collisions_fetch(mgx_world *w, std::vector<Event> &host_log, const DevEvent *log_d, uint64_t total, Less less, uint64_t first, Event *events,
                            uint64_t capacity, const uint32_t *per_robot_d, size_t n_sized, uint32_t *per_robot) {
    static_assert(sizeof(Event) == sizeof(DevEvent), "the device's record is the ABI's");
    hipStream_t s = w->stream;
    if (host_log.size() < total) {
        const size_t have = host_log.size();
        host_log.resize((size_t)total);
        HIP_TRY(hipMemcpyAsync(host_log.data() + have, log_d + have, sizeof(Event) * ((size_t)total - have), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::sort(host_log.begin() + (long)have, host_log.end(), less);
    }
    for (uint64_t i = first, k = 0; events && i < total && k < capacity; i++, k++) events[k] = host_log[(size_t)i];
    if (per_robot) {
        const size_t R = w->robots.size(), n = std::min(R, n_sized);
        std::fill(per_robot, per_robot + R, 0u);
        if (n) {
            HIP_TRY(hipMemcpyAsync(per_robot, per_robot_d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return MGX_OK;
}

extern "C" {

static constexpr uint64_t COLL_DEFAULT_EVENTS = 1ull << 18;  // 8 MB of 32-byte records
static constexpr uint32_t COLL_LIST_CAP = 1u << 16;          // pairs overlapping at the same time
static constexpr uint32_t COLL_MAX_STRIDE = 46336u;          // stride^2 bits stay below 2^31 (256 MB)

static bool collisions_sharded(const mgx_world *w) {
    for (const Robot &q : w->robots)
        if (q.ghost) return true;
    return false;
}

// who is alive, and the caller's positions (NULL: none): up from a pinned slot, behind whatever the stream is busy with
static int collisions_stage(mgx_world *w, const float *positions_xyz, DevBuf<float> &pos, DevBuf<uint8_t> &alive, hipStream_t s) {
    const size_t R = w->robots.size(), pos_bytes = positions_xyz ? sizeof(float) * 3 * R : 0;
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(alive.reserve(R));
    if (positions_xyz) HIP_TRY(pos.reserve(3 * R));
    HIP_TRY(w->stage.acquire(pos_bytes + R, &hp, &slot));
    char *h = static_cast<char *>(hp);
    if (positions_xyz) memcpy(h, positions_xyz, pos_bytes);
    for (size_t r = 0; r < R; r++) h[pos_bytes + r] = (!w->robots[r].removed && !w->robots[r].ghost) ? 1 : 0;
    if (positions_xyz) HIP_TRY(hipMemcpyAsync(pos.p, h, pos_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(alive.p, h + pos_bytes, R, hipMemcpyHostToDevice, s));
    HIP_TRY(w->stage.release(slot, s));
    return MGX_OK;
}

// the per-robot arrays for the robots the world has NOW (radii, contact counts, grid links, pair bits)
static int collisions_size(mgx_world *w) {
    mgx_world::Collisions &c = w->coll;
    const size_t R = w->robots.size();
    if (R == c.n_sized) return MGX_OK;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "collision bookkeeping runs on unsharded worlds");
    hipStream_t s = w->stream;
    std::vector<float> rad(R);
    for (size_t r = 0; r < R; r++) rad[r] = (float)w->robots[r].radius;
    HIP_TRY(c.radius.upload(rad, s));
    HIP_TRY(c.next.reserve(R));
    if (c.per_robot.cap < R) {  // the counts so far move to the front of a longer array
        DevBuf<uint32_t> grown;
        HIP_TRY(grown.reserve(R));
        HIP_TRY(hipMemsetAsync(grown.p, 0, sizeof(uint32_t) * grown.cap, s));
        if (c.n_sized) HIP_TRY(hipMemcpyAsync(grown.p, c.per_robot.p, sizeof(uint32_t) * c.n_sized, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        c.per_robot.swap(grown);
    }
    uint32_t M = 64;
    while (M < 2u * (uint32_t)R) M <<= 1;
    if (c.head.cap < M) {
        HIP_TRY(c.head.reserve(M));
        HIP_TRY(hipMemsetAsync(c.head.p, 0, sizeof(unsigned long long) * c.head.cap, s));
    }
    c.n_buckets = M;
    if (R > c.stride) {
        const uint64_t stride = ((uint64_t)R + R / 4 + 64 + 31) & ~31ull;
        if (stride > COLL_MAX_STRIDE) return fail(MGX_ERR_NOMEM, "collision bookkeeping: %zu robots are more than the pair bits hold", R);
        DevBuf<uint32_t> grown;
        HIP_TRY(grown.reserve((size_t)(stride * stride / 32)));
        HIP_TRY(hipMemsetAsync(grown.p, 0, sizeof(uint32_t) * grown.cap, s));
        c.bits.swap(grown);
        c.stride = (uint32_t)stride;
        c.d.bits = c.bits.p;
        c.d.stride = c.stride;
        c.d.pass = c.pass;
        HIP_TRY(launch_collisions_rebits(c.d, s));
        HIP_TRY(hipStreamSynchronize(s));  // (before the bits of the old stride are freed)
    }
    HIP_TRY(hipStreamSynchronize(s));  // (the radii go up from pageable memory)
    c.d.radius = c.radius.p;
    c.d.per_robot = c.per_robot.p;
    c.d.head = c.head.p;
    c.d.next = c.next.p;
    c.n_sized = R;
    return MGX_OK;
}

// one pass over device-resident positions [R][3] and alive bytes [R], enqueued on `s`
static int collisions_pass(mgx_world *w, const float *pos_d, const uint8_t *alive_d, hipStream_t s) {
    mgx_world::Collisions &c = w->coll;
    int rc = collisions_size(w);
    if (rc != MGX_OK) return rc;
    const size_t R = w->robots.size();
    size_t n_alive = 0;
    float r_max = 0.f;
    bool radii_ok = true;
    for (size_t r = 0; r < R; r++) {
        const Robot &rb = w->robots[r];
        if (rb.removed || rb.ghost) continue;
        const float rr = (float)rb.radius;
        n_alive++;
        if (!std::isfinite(rr)) radii_ok = false;
        else r_max = std::max(r_max, rr);
    }
    bool grid = c.method == MGX_NEIGHBOURS_GRID || (c.method == MGX_NEIGHBOURS_AUTO && n_alive >= 512);
    if (!radii_ok || !(r_max > 0.f)) grid = false;  // every pair has to see the predicate
    const double cell = 2.0 * (double)r_max * 1.001;  // (the margin covers the roundings of the f32 predicate)
    if (!std::isfinite(cell)) grid = false;
    c.d.pos = pos_d;
    c.d.alive = alive_d;
    c.d.n = (int)R;
    c.d.pass = c.pass;
    HIP_TRY(launch_collisions_pass(c.d, grid, cell, c.n_buckets, s));
    c.pass += 1;
    return MGX_OK;
}

static int collisions_reset(mgx_world *w) {  // everybody Free, nothing logged, nothing counted
    mgx_world::Collisions &c = w->coll;
    hipStream_t s = w->stream;
    if (c.bits.p) HIP_TRY(hipMemsetAsync(c.bits.p, 0, sizeof(uint32_t) * c.bits.cap, s));
    if (c.per_robot.p) HIP_TRY(hipMemsetAsync(c.per_robot.p, 0, sizeof(uint32_t) * c.per_robot.cap, s));
    if (c.head.p) HIP_TRY(hipMemsetAsync(c.head.p, 0, sizeof(unsigned long long) * c.head.cap, s));
    HIP_TRY(hipMemsetAsync(c.cnt.p, 0, sizeof(uint32_t) * 3, s));
    HIP_TRY(hipMemsetAsync(c.words.p, 0, sizeof(unsigned long long) * 2, s));
    c.pass = 0;
    c.host_log.clear();
    return MGX_OK;
}

int mgx_collisions_enable(mgx_world *w, int32_t enabled, uint32_t method, uint64_t event_capacity) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    mgx_world::Collisions &c = w->coll;
    if (!enabled) {  // the state goes with it: enabling again starts from everybody Free
        if (c.enabled) HIP_TRY(hipStreamSynchronize(w->stream));
        c.enabled = false;
        c.bits.release(); c.cnt.release(); c.per_robot.release(); c.list[0].release(); c.list[1].release(); c.log.release();
        c.words.release(); c.head.release(); c.next.release(); c.radius.release(); c.pos.release(); c.alive.release();
        c.n_sized = 0; c.stride = 0; c.pass = 0; c.log_cap = 0;
        c.host_log.clear();
        c.d = CollDev{};
        return MGX_OK;
    }
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "collision bookkeeping runs on unsharded worlds");
    if (c.enabled) {  // the capacities were chosen when it was switched on
        if (event_capacity && event_capacity != c.log_cap) return fail(MGX_ERR_STATE, "collision bookkeeping is on with room for %llu events", (unsigned long long)c.log_cap);
        c.method = method;
        return MGX_OK;
    }
    const uint64_t cap = event_capacity ? event_capacity : COLL_DEFAULT_EVENTS;
    if (cap > (1ull << 31)) return fail(MGX_ERR_INVALID, "event capacity beyond 2^31");
    HIP_TRY(c.log.reserve((size_t)cap));
    HIP_TRY(c.list[0].reserve(COLL_LIST_CAP));
    HIP_TRY(c.list[1].reserve(COLL_LIST_CAP));
    HIP_TRY(c.cnt.reserve(3));
    HIP_TRY(c.words.reserve(2));
    c.log_cap = cap;
    c.method = method;
    c.n_sized = 0;
    c.stride = 0;
    c.d = CollDev{};
    c.d.list[0] = c.list[0].p; c.d.list[1] = c.list[1].p; c.d.cnt = c.cnt.p; c.d.list_cap = COLL_LIST_CAP;
    c.d.log = c.log.p; c.d.log_cap = cap; c.d.words = c.words.p;
    const int rc = collisions_reset(w);
    if (rc != MGX_OK) return rc;
    c.enabled = true;
    return MGX_OK;
}

int mgx_collisions_update(mgx_world *w, const float *positions_xyz) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Collisions &c = w->coll;
    if (!c.enabled) return fail(MGX_ERR_STATE, "collision bookkeeping is off (mgx_collisions_enable)");
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "collision bookkeeping runs on unsharded worlds");
    const size_t R = w->robots.size();
    if (R == 0) { c.pass += 1; return MGX_OK; }
    const mgx_world::Mission &ms = w->mission;
    if (!positions_xyz && (!ms.uploaded || ms.dirty || ms.has.size() != R))
        return fail(MGX_ERR_STATE, "the device holds no Transforms of these robots (mgx_mission_tick)");
    hipStream_t s = w->stream;
    const int rc = collisions_stage(w, positions_xyz, c.pos, c.alive, s);
    if (rc != MGX_OK) return rc;
    return collisions_pass(w, positions_xyz ? c.pos.p : ms.translation_d.p, c.alive.p, s);
}

int mgx_collisions_read(mgx_world *w, uint64_t first, mgx_collision_event *events, uint64_t capacity, uint64_t *n_total, uint64_t *dropped,
                        uint32_t *per_robot) {
    MGX_ENTER(w);
    if (!w || (!events && capacity)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Collisions &c = w->coll;
    if (!c.enabled) return fail(MGX_ERR_STATE, "collision bookkeeping is off (mgx_collisions_enable)");
    if (w->pending.active) { const int rcc = confirm_resident(w); if (rcc != MGX_OK) return rcc; }
    hipStream_t s = w->stream;
    unsigned long long words[2] = {0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(words, c.words.p, sizeof words, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = std::min<uint64_t>(words[0], c.log_cap);
    if (n_total) *n_total = total;
    if (dropped) *dropped = words[0] - total;
    const int rc = collisions_fetch(w, c.host_log, c.log.p, total, [](const mgx_collision_event &x, const mgx_collision_event &y) {
        if (x.pass != y.pass) return x.pass < y.pass;
        if (x.robot_a != y.robot_a) return x.robot_a < y.robot_a;
        return x.robot_b < y.robot_b;
    }, first, events, capacity, c.per_robot.p, c.n_sized, per_robot);
    if (rc != MGX_OK) return rc;
    if (words[1])
        return fail(MGX_ERR_STATE, "more than %u pairs overlapped at once: the overlap state overflowed, later passes may have missed contacts", COLL_LIST_CAP);
    return check_device_error(w);
}

int mgx_collisions_clear(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->coll.enabled) return fail(MGX_ERR_STATE, "collision bookkeeping is off (mgx_collisions_enable)");
    return collisions_reset(w);
}

// ---- robot-environment collisions (mgx_env_collisions_*): the map's side goes up once, the robots' side follows the world ----
static constexpr double ENV_COLL_PAD = 1e-4;  // of a tile, added to a robot's reach when its cells are chosen

static int env_cell_of_host(double v, double origin, double inv_cell, int n) {  // == env_cell_of (mgx_collisions.hip)
    const double c = std::floor((v - origin) * inv_cell);
    return (int)std::fmin(std::fmax(c, 0.0), (double)(n - 1));
}

static void env_collisions_drop(mgx_world *w) {
    mgx_world::EnvCollisions &c = w->envcoll;
    c.enabled = false;
    c.colliders.release(); c.verts.release(); c.radius.release(); c.pos.release(); c.cell_ptr.release(); c.per_robot.release();
    c.cell_idx.release(); c.touching.release(); c.log.release(); c.words.release(); c.alive.release();
    c.n_sized = 0; c.pass = 0; c.log_cap = 0;
    c.host_log.clear();
    c.d = EnvCollDev{};
}

// the per-robot arrays for the robots the world has NOW: radii; counts and touched colliders of the robots so far keep their place
static int env_collisions_size(mgx_world *w) {
    mgx_world::EnvCollisions &c = w->envcoll;
    const size_t R = w->robots.size();
    if (R == c.n_sized) return MGX_OK;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "collision bookkeeping runs on unsharded worlds");
    hipStream_t s = w->stream;
    std::vector<float> rad(R);
    for (size_t r = 0; r < R; r++) rad[r] = (float)w->robots[r].radius;
    HIP_TRY(c.radius.upload(rad, s));
    if (c.per_robot.cap < R) {
        DevBuf<uint32_t> counts;
        DevBuf<int32_t> slots;
        HIP_TRY(counts.reserve(R));
        HIP_TRY(slots.reserve(counts.cap * ENV_COLL_SLOTS));  // (slots for every robot the counts have room for)
        HIP_TRY(hipMemsetAsync(counts.p, 0, sizeof(uint32_t) * counts.cap, s));
        HIP_TRY(hipMemsetAsync(slots.p, 0xff, sizeof(int32_t) * slots.cap, s));  // -1: a new robot touches nothing
        if (c.n_sized) {
            HIP_TRY(hipMemcpyAsync(counts.p, c.per_robot.p, sizeof(uint32_t) * c.n_sized, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(slots.p, c.touching.p, sizeof(int32_t) * ENV_COLL_SLOTS * c.n_sized, hipMemcpyDeviceToDevice, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        c.per_robot.swap(counts);
        c.touching.swap(slots);
    }
    HIP_TRY(hipStreamSynchronize(s));  // (the radii go up from pageable memory)
    c.d.radius = c.radius.p;
    c.d.per_robot = c.per_robot.p;
    c.d.touching = c.touching.p;
    c.n_sized = R;
    return MGX_OK;
}

// one pass over device-resident positions [R][3] and alive bytes [R], enqueued on `s`
static int env_collisions_pass(mgx_world *w, const float *pos_d, const uint8_t *alive_d, hipStream_t s) {
    mgx_world::EnvCollisions &c = w->envcoll;
    const int rc = env_collisions_size(w);
    if (rc != MGX_OK) return rc;
    c.d.pos = pos_d;
    c.d.alive = alive_d;
    c.d.n = (int)w->robots.size();
    c.d.pass = c.pass;
    HIP_TRY(launch_env_collisions_pass(c.d, s));
    c.pass += 1;
    return MGX_OK;
}

static int env_collisions_reset(mgx_world *w) {  // everybody Free, nothing logged, nothing counted
    mgx_world::EnvCollisions &c = w->envcoll;
    hipStream_t s = w->stream;
    if (c.per_robot.p) HIP_TRY(hipMemsetAsync(c.per_robot.p, 0, sizeof(uint32_t) * c.per_robot.cap, s));
    if (c.touching.p) HIP_TRY(hipMemsetAsync(c.touching.p, 0xff, sizeof(int32_t) * c.touching.cap, s));
    HIP_TRY(hipMemsetAsync(c.words.p, 0, sizeof(unsigned long long) * 2, s));
    c.pass = 0;
    c.host_log.clear();
    return MGX_OK;
}

static int env_collisions_upload(mgx_world *w, const std::vector<EnvCollider> &dev, const std::vector<float> &verts, const std::vector<uint32_t> &ptr,
                                 const std::vector<int32_t> &idx, uint64_t cap) {  // (a failure leaves the caller to drop what went up)
    mgx_world::EnvCollisions &c = w->envcoll;
    hipStream_t s = w->stream;
    HIP_TRY(c.colliders.upload(dev, s));
    HIP_TRY(c.verts.upload(verts, s));
    HIP_TRY(c.cell_ptr.upload(ptr, s));
    HIP_TRY(c.cell_idx.upload(idx, s));
    HIP_TRY(c.log.reserve((size_t)cap));
    HIP_TRY(c.words.reserve(2));
    HIP_TRY(hipStreamSynchronize(s));  // (the tables go up from pageable memory)
    return MGX_OK;
}

int mgx_env_collisions_enable(mgx_world *w, const mgx_env_desc *env, uint64_t event_capacity) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::EnvCollisions &c = w->envcoll;
    if (!env) {  // the state goes with it
        if (c.enabled) HIP_TRY(hipStreamSynchronize(w->stream));
        env_collisions_drop(w);
        return MGX_OK;
    }
    if (c.enabled) return fail(MGX_ERR_STATE, "environment collision bookkeeping is on (switch it off before handing in another map)");
    uint32_t n = 0, nv = 0;
    int rc = mgx_env_colliders(env, nullptr, 0, &n, nullptr, 0, &nv);
    if (rc != MGX_OK) return rc;
    std::vector<mgx_env_collider> cols(n);
    std::vector<float> verts(2 * (size_t)nv);
    if (n && (rc = mgx_env_colliders(env, cols.data(), n, &n, verts.data(), nv, &nv)) != MGX_OK) return rc;
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "collision bookkeeping runs on unsharded worlds");
    const uint64_t cap = event_capacity ? event_capacity : COLL_DEFAULT_EVENTS;
    if (cap > (1ull << 31)) return fail(MGX_ERR_INVALID, "event capacity beyond 2^31");
    if ((uint64_t)env->n_cols * env->n_rows > (1ull << 24)) return fail(MGX_ERR_INVALID, "more than 2^24 tiles");
    // the grid: a cell is one tile, the world is centred on the origin (map_generator.rs:563-579)
    const int ncx = (int)env->n_cols, ncz = (int)env->n_rows;
    const double ts = (double)env->tile_size, x0 = -0.5 * ts * ncx, z0 = -0.5 * ts * ncz, inv = 1.0 / ts;
    std::vector<EnvCollider> dev(n);
    std::vector<uint32_t> ptr((size_t)ncx * ncz + 1, 0u);
    for (uint32_t k = 0; k < n; k++) {
        const mgx_env_collider &a = cols[k];
        EnvCollider &e = dev[k];
        e.kind = a.kind; e.first_vertex = a.first_vertex; e.n_vertices = a.n_vertices; e.radius = a.radius;
        e.tx = a.tx; e.tz = a.tz; e.hx = a.half_extents[0]; e.hz = a.half_extents[1];
        for (int q = 0; q < 2; q++) { e.mins[q] = a.mins[q]; e.maxs[q] = a.maxs[q]; }
        if (a.kind == MGX_COLLIDER_POLYGON && (uint64_t)a.first_vertex + a.n_vertices > nv) return fail(MGX_ERR_INVALID, "collider %u: vertices out of range", k);
        e.cx0 = env_cell_of_host(a.mins[0], x0, inv, ncx); e.cx1 = env_cell_of_host(a.maxs[0], x0, inv, ncx);
        e.cz0 = env_cell_of_host(a.mins[1], z0, inv, ncz); e.cz1 = env_cell_of_host(a.maxs[1], z0, inv, ncz);
        for (int cz = e.cz0; cz <= e.cz1; cz++)
            for (int cx = e.cx0; cx <= e.cx1; cx++) ptr[(size_t)cz * ncx + cx + 1]++;
    }
    for (size_t i = 1; i < ptr.size(); i++) ptr[i] += ptr[i - 1];
    std::vector<int32_t> idx(ptr.back());
    {
        std::vector<uint32_t> at(ptr.begin(), ptr.end() - 1);
        for (uint32_t k = 0; k < n; k++)
            for (int cz = dev[k].cz0; cz <= dev[k].cz1; cz++)
                for (int cx = dev[k].cx0; cx <= dev[k].cx1; cx++) idx[at[(size_t)cz * ncx + cx]++] = (int32_t)k;
    }
    if ((rc = env_collisions_upload(w, dev, verts, ptr, idx, cap)) != MGX_OK) { env_collisions_drop(w); return rc; }
    c.log_cap = cap;
    c.n_sized = 0;
    c.d = EnvCollDev{};
    c.d.colliders = c.colliders.p; c.d.n_colliders = (int)n; c.d.verts = c.verts.p;
    c.d.cell_ptr = c.cell_ptr.p; c.d.cell_idx = c.cell_idx.p; c.d.n_cx = ncx; c.d.n_cz = ncz;
    c.d.x0 = x0; c.d.z0 = z0; c.d.inv_cell = inv; c.d.pad = ENV_COLL_PAD * ts;
    c.d.log = c.log.p; c.d.log_cap = cap; c.d.words = c.words.p;
    rc = env_collisions_reset(w);
    if (rc != MGX_OK) { env_collisions_drop(w); return rc; }
    c.enabled = true;
    return MGX_OK;
}

int mgx_env_collisions_update(mgx_world *w, const float *positions_xyz) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::EnvCollisions &c = w->envcoll;
    if (!c.enabled) return fail(MGX_ERR_STATE, "environment collision bookkeeping is off (mgx_env_collisions_enable)");
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "collision bookkeeping runs on unsharded worlds");
    const size_t R = w->robots.size();
    if (R == 0) { c.pass += 1; return MGX_OK; }
    const mgx_world::Mission &ms = w->mission;
    if (!positions_xyz && (!ms.uploaded || ms.dirty || ms.has.size() != R))
        return fail(MGX_ERR_STATE, "the device holds no Transforms of these robots (mgx_mission_tick)");
    hipStream_t s = w->stream;
    const int rc = collisions_stage(w, positions_xyz, c.pos, c.alive, s);
    if (rc != MGX_OK) return rc;
    return env_collisions_pass(w, positions_xyz ? c.pos.p : ms.translation_d.p, c.alive.p, s);
}

int mgx_env_collisions_read(mgx_world *w, uint64_t first, mgx_env_collision_event *events, uint64_t capacity, uint64_t *n_total, uint64_t *dropped,
                            uint32_t *per_robot) {
    MGX_ENTER(w);
    if (!w || (!events && capacity)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::EnvCollisions &c = w->envcoll;
    if (!c.enabled) return fail(MGX_ERR_STATE, "environment collision bookkeeping is off (mgx_env_collisions_enable)");
    if (w->pending.active) { const int rcc = confirm_resident(w); if (rcc != MGX_OK) return rcc; }
    hipStream_t s = w->stream;
    unsigned long long words[2] = {0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(words, c.words.p, sizeof words, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = std::min<uint64_t>(words[0], c.log_cap);
    if (n_total) *n_total = total;
    if (dropped) *dropped = words[0] - total;
    const int rc = collisions_fetch(w, c.host_log, c.log.p, total, [](const mgx_env_collision_event &x, const mgx_env_collision_event &y) {
        if (x.pass != y.pass) return x.pass < y.pass;
        if (x.robot != y.robot) return x.robot < y.robot;
        return x.collider < y.collider;
    }, first, events, capacity, c.per_robot.p, c.n_sized, per_robot);
    if (rc != MGX_OK) return rc;
    if (words[1])
        return fail(MGX_ERR_STATE, "a robot touched more than %d colliders at once: contacts beyond that may have been logged again", ENV_COLL_SLOTS);
    return check_device_error(w);
}

int mgx_env_collisions_clear(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->envcoll.enabled) return fail(MGX_ERR_STATE, "environment collision bookkeeping is off (mgx_env_collisions_enable)");
    return env_collisions_reset(w);
}

}  // extern "C" (continued in the next part)
