// mgx_world_observers.inc — what the observers (the passes mgx_mission_tick_end enqueues beside the GBP schedule: the two contact
// books, the trackers with their run metrics, the goal areas — the three parts behind this one) share on the host: the robots' inputs
// (mgx_world::RobotInputs), the head-room and the growth of every array that follows the robots, the checks and staging of an _update.
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).

static bool collisions_sharded(const mgx_world *w) { return w->obs.n_ghosts != 0; }
// the robots an observer looks at: the staged flags, the mission chain's moving bytes and the passes' own walks all ask here
static inline bool observed(const Robot &rb) { return !rb.removed && !rb.ghost; }

// the robots an array gets room for once `R` robots have outgrown it.  observers_room: with the world's head-room, so that the
// appends of a reserved world move nothing (the pair bits, quadratic in their stride, leave that out)
static size_t robots_room(size_t R, size_t at_least = 0) { return (std::max(R + R / 4 + 64, at_least) + 63) & ~(size_t)63; }
static size_t observers_room(const mgx_world *w, size_t R) { return robots_room(R, std::max<size_t>(w->reserve_want, (size_t)std::max(w->R_cap, 0))); }

// The arrays one sizing has grown out of: passes enqueued earlier may still read them, so they are freed once the stream has been
// synchronised — once for all of them (retire; at the latest when the sizing is left), and not at all while nothing moved
struct Outgrown {
    hipStream_t s;
    std::vector<void *> gone;
    ~Outgrown() { (void)retire(); }
    // `rows` rows of `want` elements where the rows had `had`: the first `keep` of every row as they were, every byte behind them
    // `byte`.  Enqueued; a failure leaves `buf` as it was
    template <class T>
    hipError_t grow(DevBuf<T> &buf, size_t want, size_t keep, int byte, size_t rows = 1, size_t had = 0) {
        DevBuf<T> next;
        hipError_t e = hipMalloc((void **)&next.p, sizeof(T) * rows * want);
        if (e != hipSuccess) return e;
        next.n = next.cap = rows * want;
        e = hipMemsetAsync(next.p, byte, sizeof(T) * next.cap, s);
        for (size_t r = 0; r < rows && keep && buf.p && e == hipSuccess; r++)
            e = hipMemcpyAsync(next.p + r * want, buf.p + r * had, sizeof(T) * keep, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;  // (`next` goes: hipFree waits for the device)
        buf.swap(next);
        if (next.p) gone.push_back(next.p);
        next.p = nullptr;
        return hipSuccess;
    }
    hipError_t retire() {
        const hipError_t e = gone.empty() ? hipSuccess : hipStreamSynchronize(s);
        for (void *p : gone) (void)hipFree(p);
        gone.clear();
        return e;
    }
};

// the radii of the robots that joined since the last sizing, behind the ones that are up: from a pinned slot, behind the passes
// enqueued so far.  A failure leaves n_sized where it was: the next sizing tries again
static int observers_radii(mgx_world *w, Outgrown &out) {
    mgx_world::RobotInputs &o = w->obs;
    const size_t R = w->robots.size(), n0 = o.n_sized;
    if (R <= n0) return MGX_OK;
    if (R > o.radius.cap) HIP_TRY(out.grow(o.radius, observers_room(w, R), n0, 0));
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(sizeof(float) * (R - n0), &hp, &slot));
    for (size_t r = n0; r < R; r++) static_cast<float *>(hp)[r - n0] = (float)w->robots[r].radius;
    HIP_TRY(hipMemcpyAsync(o.radius.p + n0, hp, sizeof(float) * (R - n0), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    o.n_sized = R;
    return MGX_OK;
}

// the groups of a GROUPED world's robots (include/mgx.h, ROBOT GROUPS), for the robot-robot pass: the ones that joined since they
// were last brought up, behind the ones that are up — as the radii above.  An ungrouped world never comes here
static int observers_groups(mgx_world *w, Outgrown &out) {
    mgx_world::RobotInputs &o = w->obs;
    const size_t R = w->robots.size(), n0 = o.group_sized;
    if (R <= n0) return MGX_OK;
    if (R > o.group.cap) HIP_TRY(out.grow(o.group, observers_room(w, R), n0, 0));
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(sizeof(uint32_t) * (R - n0), &hp, &slot));
    for (size_t r = n0; r < R; r++) static_cast<uint32_t *>(hp)[r - n0] = w->sets.group[r];
    HIP_TRY(hipMemcpyAsync(o.group.p + n0, hp, sizeof(uint32_t) * (R - n0), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    o.group_sized = R;
    return MGX_OK;
}

// who is looked at — and has moved, where the caller says who did (moved, may be NULL) — and the caller's positions (NULL: none):
// up from a pinned slot, behind whatever the stream is busy with (a buffer that has to grow: RobotInputs says what frees it)
static int observers_stage(mgx_world *w, const float *positions_xyz, const uint8_t *moved, hipStream_t s) {
    mgx_world::RobotInputs &o = w->obs;
    const size_t R = w->robots.size(), pos_bytes = positions_xyz ? sizeof(float) * 3 * R : 0;
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(o.flags.reserve(R));
    if (positions_xyz) HIP_TRY(o.pos.reserve(3 * R));
    HIP_TRY(w->stage.acquire(pos_bytes + R, &hp, &slot));
    char *h = static_cast<char *>(hp);
    if (positions_xyz) memcpy(h, positions_xyz, pos_bytes);
    for (size_t r = 0; r < R; r++) h[pos_bytes + r] = (observed(w->robots[r]) && (!moved || moved[r])) ? 1 : 0;
    if (positions_xyz) HIP_TRY(hipMemcpyAsync(o.pos.p, h, pos_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(o.flags.p, h + pos_bytes, R, hipMemcpyHostToDevice, s));
    HIP_TRY(w->stage.release(slot, s));
    return MGX_OK;
}

// What mgx_*collisions_update, mgx_tracks_update and mgx_goal_areas_update do before their pass; the caller hands in what differs:
// whether its observer is on, the texts, what is wrong with an argument of its own (`invalid`; NULL: nothing).  Out: the device
// positions and flags the pass is to read.  flags NULL: a world without robots — nothing staged, and what that means is the caller's
struct ObserverInputs { const float *pos = nullptr; const uint8_t *flags = nullptr; };
static int observers_update_begin(mgx_world *w, bool enabled, const char *off, const char *unsharded, const char *invalid,
                                  const float *positions_xyz, const uint8_t *moved, ObserverInputs &in) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!enabled) return fail(MGX_ERR_STATE, "%s", off);
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", unsharded);
    if (invalid) return fail(MGX_ERR_INVALID, "%s", invalid);
    const size_t R = w->robots.size();
    if (R == 0) return MGX_OK;
    const mgx_world::Mission &ms = w->mission;
    if (!positions_xyz && (!ms.uploaded || ms.dirty || ms.has.size() != R))
        return fail(MGX_ERR_STATE, "the device holds no Transforms of these robots (mgx_mission_tick)");
    const int rc = observers_stage(w, positions_xyz, moved, w->stream);
    if (rc != MGX_OK) return rc;
    in.pos = positions_xyz ? w->obs.pos.p : ms.translation_d.p;
    in.flags = w->obs.flags.p;
    return MGX_OK;
}
