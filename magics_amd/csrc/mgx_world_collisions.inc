// mgx_world_collisions.inc — C ABI: robot-robot collision bookkeeping on the device (the pass mgx_mission_tick_end enqueues).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a pass computes and how its state is kept: mgx_collisions.hip.  The host's side here: the arrays follow the world's robots
// (ids never change, so commit / mgx_robot_remove move nothing: robots that join make the per-robot arrays and the stride of the
// pair bits grow, and the bits are set again from the pair list), a pass is enqueued on the world's stream without a
// synchronisation or a read-back, and mgx_collisions_read is the one call that waits.
extern "C" {

static constexpr uint64_t COLL_DEFAULT_EVENTS = 1ull << 18;  // 8 MB of 32-byte records
static constexpr uint32_t COLL_LIST_CAP = 1u << 16;          // pairs overlapping at the same time
static constexpr uint32_t COLL_MAX_STRIDE = 46336u;          // stride^2 bits stay below 2^31 (256 MB)

static bool collisions_sharded(const mgx_world *w) {
    for (const Robot &q : w->robots)
        if (q.ghost) return true;
    return false;
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
    // who is alive, and the caller's positions: up from a pinned slot, behind whatever the stream is busy with
    const size_t pos_bytes = positions_xyz ? sizeof(float) * 3 * R : 0;
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(c.alive.reserve(R));
    if (positions_xyz) HIP_TRY(c.pos.reserve(3 * R));
    HIP_TRY(w->stage.acquire(pos_bytes + R, &hp, &slot));
    char *h = static_cast<char *>(hp);
    if (positions_xyz) memcpy(h, positions_xyz, pos_bytes);
    for (size_t r = 0; r < R; r++) h[pos_bytes + r] = (!w->robots[r].removed && !w->robots[r].ghost) ? 1 : 0;
    if (positions_xyz) HIP_TRY(hipMemcpyAsync(c.pos.p, h, pos_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c.alive.p, h + pos_bytes, R, hipMemcpyHostToDevice, s));
    HIP_TRY(w->stage.release(slot, s));
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
    // the log only grows and every pass enqueued so far is complete: what was fetched before keeps its place, the rest is put
    // in (pass, robot_a, robot_b) order — which lane won an atomic never shows
    if (c.host_log.size() < total) {
        const size_t have = c.host_log.size();
        c.host_log.resize((size_t)total);
        HIP_TRY(hipMemcpyAsync(c.host_log.data() + have, c.log.p + have, sizeof(mgx_collision_event) * ((size_t)total - have), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::sort(c.host_log.begin() + (long)have, c.host_log.end(), [](const mgx_collision_event &x, const mgx_collision_event &y) {
            if (x.pass != y.pass) return x.pass < y.pass;
            if (x.robot_a != y.robot_a) return x.robot_a < y.robot_a;
            return x.robot_b < y.robot_b;
        });
    }
    if (n_total) *n_total = total;
    if (dropped) *dropped = words[0] - total;
    for (uint64_t i = first, k = 0; events && i < total && k < capacity; i++, k++) events[k] = c.host_log[(size_t)i];
    if (per_robot) {
        const size_t R = w->robots.size(), n = std::min(R, c.n_sized);
        std::fill(per_robot, per_robot + R, 0u);  // (robots that joined since the last pass have met nobody)
        if (n) {
            HIP_TRY(hipMemcpyAsync(per_robot, c.per_robot.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
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

}  // extern "C" (continued in the next part)
