// mgx_world_collisions.inc — C ABI: robot-robot and robot-environment collision bookkeeping on the device (the passes
// mgx_mission_tick_end enqueues).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a pass computes and how its state is kept: mgx_collisions.hip.  The host's side here: the books' own per-robot arrays follow
// the world's robots under the rule of mgx_world_observers.inc (a longer stride of the pair bits: the bits are set again from the
// pair list), a pass is enqueued on the world's stream without a synchronisation or a read-back, and mgx_collisions_read /
// mgx_env_collisions_read are the calls that wait.  What the two bookkeepings share (ContactBook, mgx_world_types.h) is written
// once, as contacts_*; the entry points hand in what differs.

static constexpr uint64_t COLL_DEFAULT_EVENTS = 1ull << 18;  // 8 MB of 32-byte records
static constexpr uint32_t COLL_LIST_CAP = 1u << 16;          // pairs overlapping at the same time
static constexpr uint32_t COLL_MAX_STRIDE = 46336u;          // stride^2 bits stay below 2^31 (256 MB)
static constexpr double ENV_COLL_PAD = 1e-4;                 // of a tile, added to a robot's reach when its cells are chosen
static const char *const COLL_OFF = "collision bookkeeping is off (mgx_collisions_enable)";
static const char *const ENV_COLL_OFF = "environment collision bookkeeping is off (mgx_env_collisions_enable)";
static const char *const COLL_UNSHARDED = "collision bookkeeping runs on unsharded worlds";
using ContactBook = mgx_world::ContactBook;
using ContactPass = int (*)(mgx_world *w, const float *pos_d, const uint8_t *alive_d, hipStream_t s);

// ---- what both bookkeepings do ------------------------------------------------------------------------------------------------
// switched on: room for the log (event_capacity 0: the default) and its two words; `d` is the pass's argument, fresh
static int contacts_open(ContactBook &b, ContactDev &d, uint64_t event_capacity) {
    const uint64_t cap = event_capacity ? event_capacity : COLL_DEFAULT_EVENTS;
    if (cap > (1ull << 31)) return fail(MGX_ERR_INVALID, "event capacity beyond 2^31");
    HIP_TRY(b.log.reserve((size_t)cap));
    HIP_TRY(b.words.reserve(2));
    b.log_cap = cap;
    b.n_sized = 0;
    d.log = ContactLog{b.log.p, cap, b.words.p};
    return MGX_OK;
}

static void contacts_drop(ContactBook &b) {  // switched off: the state goes with it
    b.enabled = false;
    b.log.release(); b.words.release(); b.per_robot.release();
    b.n_sized = 0; b.pass = 0; b.log_cap = 0;
    b.host_log.clear();
}

static int contacts_reset(ContactBook &b, hipStream_t s) {  // nothing logged, nothing counted
    if (b.per_robot.p) HIP_TRY(hipMemsetAsync(b.per_robot.p, 0, sizeof(uint32_t) * b.per_robot.cap, s));
    HIP_TRY(hipMemsetAsync(b.words.p, 0, sizeof(unsigned long long) * 2, s));
    b.pass = 0;
    b.host_log.clear();
    return MGX_OK;
}

// the robots' side of a sizing, for the robots the world has NOW: the shared radii complete, the counts so far in a longer array
static int contacts_size(mgx_world *w, ContactBook &b, ContactDev &d, Outgrown &out) {
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", COLL_UNSHARDED);
    const int rc = observers_radii(w, out);
    if (rc != MGX_OK) return rc;
    if (w->robots.size() > b.per_robot.cap) HIP_TRY(out.grow(b.per_robot, observers_room(w, w->robots.size()), b.n_sized, 0));
    d.radius = w->obs.radius.p;
    d.per_robot = b.per_robot.p;
    return MGX_OK;
}

// mgx_*collisions_update: one pass over the caller's positions, or over the device's mission Transforms (no robots: it counts too)
static int contacts_update(mgx_world *w, ContactBook *b, const float *positions_xyz, const char *off, ContactPass pass) {
    ObserverInputs in;
    const int rc = observers_update_begin(w, b && b->enabled, off, COLL_UNSHARDED, nullptr, positions_xyz, nullptr, in);
    if (rc != MGX_OK) return rc;
    if (!in.flags) { b->pass += 1; return MGX_OK; }
    return pass(w, in.pos, in.flags, w->stream);
}

// what a read call hands out.  The log only grows and every pass enqueued so far is complete: what was fetched before keeps its
// place, the rest is put in (pass, a, b) order — which lane won an atomic never shows.  per_robot: robots that joined since the
// last pass have no contact yet.
static int collisions_fetch(mgx_world *w, ContactBook &b, uint64_t total, uint64_t first, void *events, uint64_t capacity, uint32_t *per_robot) {
    hipStream_t s = w->stream;
    std::vector<ContactEvent> &host_log = b.host_log;
    if (host_log.size() < total) {
        const size_t have = host_log.size();
        host_log.resize((size_t)total);
        HIP_TRY(hipMemcpyAsync(host_log.data() + have, b.log.p + have, sizeof(ContactEvent) * ((size_t)total - have), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::sort(host_log.begin() + (long)have, host_log.end(), [](const ContactEvent &x, const ContactEvent &y) {
            if (x.pass != y.pass) return x.pass < y.pass;
            if (x.a != y.a) return x.a < y.a;
            return x.b < y.b;
        });
    }
    if (events && first < total)  // (the ABI's records are ContactEvent's layout: mgx_collisions.hip asserts it)
        memcpy(events, host_log.data() + first, sizeof(ContactEvent) * (size_t)std::min<uint64_t>(total - first, capacity));
    if (per_robot) {
        const size_t R = w->robots.size(), n = std::min(R, b.n_sized);
        std::fill(per_robot, per_robot + R, 0u);
        if (n) {
            HIP_TRY(hipMemcpyAsync(per_robot, b.per_robot.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return MGX_OK;
}

// mgx_*collisions_read; overflow: the text for a set sticky word (one %u: overflow_n), reported with every output filled
static int contacts_read(mgx_world *w, ContactBook *b, uint64_t first, void *events, uint64_t capacity, uint64_t *n_total, uint64_t *dropped,
                         uint32_t *per_robot, const char *off, const char *overflow, unsigned overflow_n) {
    MGX_ENTER(w);
    if (!w || (!events && capacity)) return fail(MGX_ERR_INVALID, "null argument");
    if (!b->enabled) return fail(MGX_ERR_STATE, "%s", off);
    MGX_CONFIRM(w);
    hipStream_t s = w->stream;
    unsigned long long words[2] = {0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(words, b->words.p, sizeof words, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = std::min<uint64_t>(words[0], b->log_cap);
    if (n_total) *n_total = total;
    if (dropped) *dropped = words[0] - total;
    const int rc = collisions_fetch(w, *b, total, first, events, capacity, per_robot);
    if (rc != MGX_OK) return rc;
    if (words[1]) return fail(MGX_ERR_STATE, overflow, overflow_n);
    return check_device_error(w);
}

static int contacts_clear(mgx_world *w, ContactBook *b, const char *off, int (*reset)(mgx_world *)) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!b->enabled) return fail(MGX_ERR_STATE, "%s", off);
    return reset(w);
}

// ---- robot-robot: pair bits, pair lists, the hash grid's links ----------------------------------------------------------------
// the per-robot arrays for the robots the world has NOW (contact counts, grid links, pair bits)
static int collisions_size(mgx_world *w) {
    mgx_world::Collisions &c = w->coll;
    const size_t R = w->robots.size();
    if (R <= c.n_sized) return MGX_OK;
    hipStream_t s = w->stream;
    Outgrown out{s};
    const int rc = contacts_size(w, c, c.d, out);
    if (rc != MGX_OK) return rc;
    if (R > c.next.cap) HIP_TRY(out.grow(c.next, observers_room(w, R), 0, 0));
    uint32_t M = 64;
    while (M < 2u * (uint32_t)R) M <<= 1;
    if (c.head.cap < M) {
        HIP_TRY(c.head.reserve(M));
        HIP_TRY(hipMemsetAsync(c.head.p, 0, sizeof(unsigned long long) * c.head.cap, s));
    }
    c.n_buckets = M;
    if (R > c.stride) {  // a new stride: every bit clear, then the bits of the listed pairs again
        const uint64_t stride = robots_room(R);
        if (stride > COLL_MAX_STRIDE) return fail(MGX_ERR_NOMEM, "collision bookkeeping: %zu robots are more than the pair bits hold", R);
        HIP_TRY(out.grow(c.bits, (size_t)(stride * stride / 32), 0, 0));
        c.stride = (uint32_t)stride;
        c.d.bits = c.bits.p;
        c.d.stride = c.stride;
        c.d.pass = c.pass;
        HIP_TRY(launch_collisions_rebits(c.d, s));
    }
    HIP_TRY(out.retire());
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
    c.d.group = nullptr;
    if (w->sets.n_grouped) {  // a grouped world: the pass compares the robots' groups
        Outgrown out{s};
        if ((rc = observers_groups(w, out)) != MGX_OK) return rc;
        HIP_TRY(out.retire());
        c.d.group = w->obs.group.p;
    }
    const size_t R = w->robots.size();
    size_t n_alive = 0;
    float r_max = 0.f;
    bool radii_ok = true;
    for (size_t r = 0; r < R; r++) {
        const Robot &rb = w->robots[r];
        if (!observed(rb)) continue;
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
    if (c.head.p) HIP_TRY(hipMemsetAsync(c.head.p, 0, sizeof(unsigned long long) * c.head.cap, s));
    HIP_TRY(hipMemsetAsync(c.cnt.p, 0, sizeof(uint32_t) * 3, s));
    return contacts_reset(c, s);
}

// ---- robot-environment: the map's side goes up once, the robots' side follows the world ---------------------------------------
static void env_collisions_drop(mgx_world *w) {
    mgx_world::EnvCollisions &c = w->envcoll;
    contacts_drop(c);
    c.map.release(); c.touching.release();
    c.d = EnvCollDev{};
}

// the per-robot arrays for the robots the world has NOW: counts and touched colliders of the robots so far keep their place
static int env_collisions_size(mgx_world *w) {
    mgx_world::EnvCollisions &c = w->envcoll;
    const size_t R = w->robots.size();
    if (R <= c.n_sized) return MGX_OK;
    Outgrown out{w->stream};
    const int rc = contacts_size(w, c, c.d, out);
    if (rc != MGX_OK) return rc;
    if (c.touching.cap < c.per_robot.cap * ENV_COLL_SLOTS)  // slots for every robot the counts have room for; -1: a new robot touches nothing
        HIP_TRY(out.grow(c.touching, c.per_robot.cap * ENV_COLL_SLOTS, c.n_sized * ENV_COLL_SLOTS, 0xff));
    HIP_TRY(out.retire());
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
    if (c.touching.p) HIP_TRY(hipMemsetAsync(c.touching.p, 0xff, sizeof(int32_t) * c.touching.cap, w->stream));
    return contacts_reset(c, w->stream);
}

// the map's colliders and the grid over them, built on the host (the map is static) and uploaded: what the robot-environment pass
// and the global planner both read.  Synchronises the stream (the tables go up from pageable memory)
static int env_map_upload(mgx_world *w, const mgx_env_desc *env, mgx_world::EnvMap &m) {
    uint32_t n = 0, nv = 0;
    int rc = mgx_env_colliders(env, nullptr, 0, &n, nullptr, 0, &nv);
    if (rc != MGX_OK) return rc;
    std::vector<mgx_env_collider> cols(n);
    std::vector<float> verts(2 * (size_t)nv);
    if (n && (rc = mgx_env_colliders(env, cols.data(), n, &n, verts.data(), nv, &nv)) != MGX_OK) return rc;
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
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
        e.cx0 = env_cell_of(a.mins[0], x0, inv, ncx); e.cx1 = env_cell_of(a.maxs[0], x0, inv, ncx);
        e.cz0 = env_cell_of(a.mins[1], z0, inv, ncz); e.cz1 = env_cell_of(a.maxs[1], z0, inv, ncz);
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
    hipStream_t s = w->stream;
    HIP_TRY(m.colliders.upload(dev, s));
    HIP_TRY(m.verts.upload(verts, s));
    HIP_TRY(m.cell_ptr.upload(ptr, s));
    HIP_TRY(m.cell_idx.upload(idx, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the tables go up from pageable memory)
    m.d.colliders = m.colliders.p; m.d.n_colliders = (int)n; m.d.verts = m.verts.p;
    m.d.cell_ptr = m.cell_ptr.p; m.d.cell_idx = m.cell_idx.p; m.d.n_cx = ncx; m.d.n_cz = ncz;
    m.d.x0 = x0; m.d.z0 = z0; m.d.inv_cell = inv; m.d.pad = ENV_COLL_PAD * ts;
    return MGX_OK;
}

// switched on: the map's colliders, the grid over them and the log go up (a failure leaves the caller to drop what went up)
static int env_collisions_open(mgx_world *w, const mgx_env_desc *env, uint64_t event_capacity) {
    mgx_world::EnvCollisions &c = w->envcoll;
    int rc = env_map_upload(w, env, c.map);
    if (rc != MGX_OK) return rc;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", COLL_UNSHARDED);
    c.d = EnvCollDev{};
    if ((rc = contacts_open(c, c.d, event_capacity)) != MGX_OK) return rc;
    const EnvMapDev &m = c.map.d;
    c.d.colliders = m.colliders; c.d.n_colliders = m.n_colliders; c.d.verts = m.verts;
    c.d.cell_ptr = m.cell_ptr; c.d.cell_idx = m.cell_idx; c.d.n_cx = m.n_cx; c.d.n_cz = m.n_cz;
    c.d.x0 = m.x0; c.d.z0 = m.z0; c.d.inv_cell = m.inv_cell; c.d.pad = m.pad;
    return env_collisions_reset(w);
}

extern "C" {

int mgx_collisions_enable(mgx_world *w, int32_t enabled, uint32_t method, uint64_t event_capacity) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    mgx_world::Collisions &c = w->coll;
    if (!enabled) {  // the state goes with it: enabling again starts from everybody Free
        if (c.enabled) HIP_TRY(hipStreamSynchronize(w->stream));
        contacts_drop(c);
        c.bits.release(); c.cnt.release(); c.list[0].release(); c.list[1].release(); c.head.release(); c.next.release();
        c.stride = 0;
        c.d = CollDev{};
        return MGX_OK;
    }
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", COLL_UNSHARDED);
    if (c.enabled) {  // the capacities were chosen when it was switched on
        if (event_capacity && event_capacity != c.log_cap) return fail(MGX_ERR_STATE, "collision bookkeeping is on with room for %llu events", (unsigned long long)c.log_cap);
        c.method = method;
        return MGX_OK;
    }
    c.d = CollDev{};
    int rc = contacts_open(c, c.d, event_capacity);
    if (rc != MGX_OK) return rc;
    HIP_TRY(c.list[0].reserve(COLL_LIST_CAP));
    HIP_TRY(c.list[1].reserve(COLL_LIST_CAP));
    HIP_TRY(c.cnt.reserve(3));
    c.method = method;
    c.stride = 0;
    c.d.list[0] = c.list[0].p; c.d.list[1] = c.list[1].p; c.d.cnt = c.cnt.p; c.d.list_cap = COLL_LIST_CAP;
    if ((rc = collisions_reset(w)) != MGX_OK) return rc;
    c.enabled = true;
    return MGX_OK;
}

int mgx_collisions_update(mgx_world *w, const float *positions_xyz) {
    return contacts_update(w, w ? &w->coll : nullptr, positions_xyz, COLL_OFF, collisions_pass);
}

int mgx_collisions_read(mgx_world *w, uint64_t first, mgx_collision_event *events, uint64_t capacity, uint64_t *n_total, uint64_t *dropped,
                        uint32_t *per_robot) {
    return contacts_read(w, w ? &w->coll : nullptr, first, events, capacity, n_total, dropped, per_robot, COLL_OFF,
                         "more than %u pairs overlapped at once: the overlap state overflowed, later passes may have missed contacts", COLL_LIST_CAP);
}

int mgx_collisions_clear(mgx_world *w) { return contacts_clear(w, w ? &w->coll : nullptr, COLL_OFF, collisions_reset); }

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
    const int rc = env_collisions_open(w, env, event_capacity);
    if (rc != MGX_OK) { env_collisions_drop(w); return rc; }
    c.enabled = true;
    return MGX_OK;
}

int mgx_env_collisions_update(mgx_world *w, const float *positions_xyz) {
    return contacts_update(w, w ? &w->envcoll : nullptr, positions_xyz, ENV_COLL_OFF, env_collisions_pass);
}

int mgx_env_collisions_read(mgx_world *w, uint64_t first, mgx_env_collision_event *events, uint64_t capacity, uint64_t *n_total, uint64_t *dropped,
                            uint32_t *per_robot) {
    return contacts_read(w, w ? &w->envcoll : nullptr, first, events, capacity, n_total, dropped, per_robot, ENV_COLL_OFF,
                         "a robot touched more than %u colliders at once: contacts beyond that may have been logged again", (unsigned)ENV_COLL_SLOTS);
}

int mgx_env_collisions_clear(mgx_world *w) { return contacts_clear(w, w ? &w->envcoll : nullptr, ENV_COLL_OFF, env_collisions_reset); }

}  // extern "C" (continued in the next part)
