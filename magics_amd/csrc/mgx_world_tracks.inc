// mgx_world_tracks.inc — C ABI: the trackers on the device — PositionTracker / VelocityTracker samples and the distance every
// robot has travelled (the pass mgx_mission_tick_end enqueues beside the two collision passes).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a pass computes: mgx_tracks.hip; the specification: include/mgx.h.  The host's side here: the per-robot state follows the
// world's robots (ids never change, so commit / mgx_robot_remove and a relayout move nothing: robots that join make the array
// grow, zeroed), a pass is enqueued on the world's stream without a synchronisation or a read-back, and mgx_tracks_take is the
// call that waits.

static constexpr uint64_t TRACKS_DEFAULT_SAMPLES = 1ull << 18;  // 10 MB of 40-byte records
static const char *const TRACKS_OFF = "the trackers are off (mgx_tracks_enable)";

static const char *const METRICS_OFF = "the run metrics are off (mgx_track_metrics_enable)";
static constexpr uint32_t METRICS_DEFAULT_ROUTE_POINTS = 16, METRICS_MAX_ROUTE_POINTS = 1u << 16;

static void metrics_drop(mgx_world *w) {
    mgx_world::Tracks &t = w->tracks;
    t.metrics = false;
    t.mstate.release(); t.route_xy.release(); t.routes.release(); t.mout.release();
    t.m_sized = t.m_room = 0; t.max_route_points = 0;
}

static void tracks_drop(mgx_world *w) {  // switched off: the state goes with it
    mgx_world::Tracks &t = w->tracks;
    metrics_drop(w);
    t.logging = true;
    t.enabled = false;
    t.state.release(); t.log.release(); t.cursor.release(); t.pos.release(); t.moved.release();
    t.n_sized = 0; t.log_cap = 0; t.period_ns = 0; t.tick_ns = 0; t.clock = 0; t.dropped = 0;
}

// the state array for the robots the world has NOW: the robots so far keep theirs, the others start from zero
static int tracks_size(mgx_world *w) {
    mgx_world::Tracks &t = w->tracks;
    const size_t R = w->robots.size();
    if (R <= t.n_sized) return MGX_OK;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the trackers run on unsharded worlds");
    if (t.state.cap < R) {  // (every element behind the robots so far is zero already: nothing to do while they fit)
        hipStream_t s = w->stream;
        DevBuf<TrackState> old;
        HIP_TRY(grow_keep(t.state, R, t.n_sized, 0, old, s));
        HIP_TRY(hipStreamSynchronize(s));  // (passes enqueued earlier may still have used what was grown out of)
    }
    t.n_sized = R;
    return MGX_OK;
}

// the metrics' arrays for the robots the world has NOW, under the rule of tracks_size: the robots so far keep state and route, the
// others start from zero and without a route.  All three arrays have room for the same number of robots
static int metrics_size(mgx_world *w) {
    mgx_world::Tracks &t = w->tracks;
    const size_t R = w->robots.size(), P = t.max_route_points;
    if (R <= t.m_sized) return MGX_OK;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the trackers run on unsharded worlds");
    if (t.m_room < R) {
        hipStream_t s = w->stream;
        const size_t room = R + R / 4 + 64;
        DevBuf<TrackMetricsState> old_state;
        DevBuf<double> old_xy;
        DevBuf<TrackRoute> old_routes;
        HIP_TRY(grow_keep(t.mstate, room, t.m_sized, 0, old_state, s));
        HIP_TRY(grow_keep(t.route_xy, room * P * 2, t.m_sized * P * 2, 0, old_xy, s));
        HIP_TRY(grow_keep(t.routes, room, t.m_sized, 0, old_routes, s));
        HIP_TRY(hipStreamSynchronize(s));  // (passes enqueued earlier may still have used what was grown out of)
        t.m_room = room;
    }
    t.m_sized = R;
    return MGX_OK;
}

// one pass at `tick` over device-resident positions [R][3] and moved bytes [R], enqueued on `s`.  distance: the mission chain's
// pass — the increment is formed from the blob's means and the missions' time scales as k_mission_prepare has just done
static int tracks_pass(mgx_world *w, const float *pos_d, const uint8_t *moved_d, uint64_t tick, bool distance, hipStream_t s) {
    mgx_world::Tracks &t = w->tracks;
    const int rc = tracks_size(w);
    if (rc != MGX_OK) return rc;
    TrackDev d{};
    d.state = t.state.p; d.log = t.log.p; d.cap = t.log_cap; d.cursor = t.cursor.p;
    d.period_ns = t.period_ns; d.tick_ns = t.tick_ns; d.tick = tick;
    d.pos = pos_d; d.moved = moved_d;
    if (distance) { d.blob = w->d.blob; d.time_scale = w->mission.time_scale_d.p; d.BS = w->d.BS; d.K = w->d.K; }
    d.n = (int)w->robots.size();
    d.no_log = t.logging ? 0 : 1;
    if (t.metrics) {
        const int mrc = metrics_size(w);
        if (mrc != MGX_OK) return mrc;
        d.metrics = t.mstate.p; d.route_xy = t.route_xy.p; d.routes = t.routes.p; d.max_route_points = t.max_route_points;
    }
    HIP_TRY(launch_tracks_pass(d, s));
    return MGX_OK;
}

static int tracks_reset(mgx_world *w) {  // nothing logged, nothing travelled, every timer and previous sample forgotten
    mgx_world::Tracks &t = w->tracks;
    hipStream_t s = w->stream;
    if (t.state.p) HIP_TRY(hipMemsetAsync(t.state.p, 0, sizeof(TrackState) * t.state.cap, s));
    if (t.mstate.p) HIP_TRY(hipMemsetAsync(t.mstate.p, 0, sizeof(TrackMetricsState) * t.mstate.cap, s));  // (the routes stay)
    HIP_TRY(hipMemsetAsync(t.cursor.p, 0, sizeof(unsigned long long), s));
    t.dropped = 0;
    return MGX_OK;
}

extern "C" {

int mgx_tracks_enable(mgx_world *w, int32_t enabled, uint64_t period_ns, uint64_t tick_ns, uint64_t next_tick, uint64_t sample_capacity) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Tracks &t = w->tracks;
    if (!enabled) {
        if (t.enabled) HIP_TRY(hipStreamSynchronize(w->stream));
        tracks_drop(w);
        return MGX_OK;
    }
    if (!period_ns || !tick_ns) return fail(MGX_ERR_INVALID, "period_ns and tick_ns must be positive");
    if (period_ns > (1ull << 62) || tick_ns > (1ull << 62)) return fail(MGX_ERR_INVALID, "period_ns or tick_ns beyond 2^62");
    const uint64_t cap = sample_capacity ? sample_capacity : TRACKS_DEFAULT_SAMPLES;
    if (cap > (1ull << 31)) return fail(MGX_ERR_INVALID, "sample capacity beyond 2^31");
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the trackers run on unsharded worlds");
    if (t.enabled) {  // the timers and the capacity were chosen when they were switched on
        if (period_ns != t.period_ns || tick_ns != t.tick_ns || (sample_capacity && cap != t.log_cap))
            return fail(MGX_ERR_STATE, "the trackers are on with period %llu ns, tick %llu ns and room for %llu samples", (unsigned long long)t.period_ns,
                        (unsigned long long)t.tick_ns, (unsigned long long)t.log_cap);
        t.clock = next_tick;
        return MGX_OK;
    }
    HIP_TRY(t.log.reserve((size_t)cap));
    HIP_TRY(t.cursor.reserve(1));
    t.log_cap = cap; t.period_ns = period_ns; t.tick_ns = tick_ns; t.clock = next_tick; t.n_sized = 0;
    const int rc = tracks_reset(w);
    if (rc != MGX_OK) { tracks_drop(w); return rc; }
    t.enabled = true;
    return MGX_OK;
}

int mgx_tracks_set_clock(mgx_world *w, uint64_t next_tick) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->tracks.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    w->tracks.clock = next_tick;
    return MGX_OK;
}

int mgx_tracks_update(mgx_world *w, const float *positions_xyz, const uint8_t *moved, uint64_t tick) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Tracks &t = w->tracks;
    if (!t.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the trackers run on unsharded worlds");
    const size_t R = w->robots.size();
    if (R == 0) return MGX_OK;
    const mgx_world::Mission &ms = w->mission;
    if (!positions_xyz && (!ms.uploaded || ms.dirty || ms.has.size() != R))
        return fail(MGX_ERR_STATE, "the device holds no Transforms of these robots (mgx_mission_tick)");
    // the caller's positions and who moved (a robot that is gone never does): up from a pinned slot, behind whatever the stream is busy with
    hipStream_t s = w->stream;
    const size_t pos_bytes = positions_xyz ? sizeof(float) * 3 * R : 0;
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(t.moved.reserve(R));
    if (positions_xyz) HIP_TRY(t.pos.reserve(3 * R));
    HIP_TRY(w->stage.acquire(pos_bytes + R, &hp, &slot));
    char *h = static_cast<char *>(hp);
    if (positions_xyz) memcpy(h, positions_xyz, pos_bytes);
    for (size_t r = 0; r < R; r++) h[pos_bytes + r] = (!w->robots[r].removed && !w->robots[r].ghost && (!moved || moved[r])) ? 1 : 0;
    if (positions_xyz) HIP_TRY(hipMemcpyAsync(t.pos.p, h, pos_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(t.moved.p, h + pos_bytes, R, hipMemcpyHostToDevice, s));
    HIP_TRY(w->stage.release(slot, s));
    return tracks_pass(w, positions_xyz ? t.pos.p : ms.translation_d.p, t.moved.p, tick, false, s);
}

int mgx_tracks_take(mgx_world *w, mgx_track_sample *samples, uint64_t capacity, uint64_t *n_taken, uint64_t *n_in_log, uint64_t *dropped,
                    double *travelled) {
    MGX_ENTER(w);
    if (!w || (!samples && capacity)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Tracks &t = w->tracks;
    if (!t.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    MGX_CONFIRM(w);
    hipStream_t s = w->stream;
    unsigned long long cursor = 0ull;
    std::vector<TrackState> st;
    const size_t R = w->robots.size(), n_st = travelled ? std::min(R, t.n_sized) : 0;
    HIP_TRY(hipMemcpyAsync(&cursor, t.cursor.p, sizeof cursor, hipMemcpyDeviceToHost, s));
    if (n_st) {
        st.resize(n_st);
        HIP_TRY(hipMemcpyAsync(st.data(), t.state.p, sizeof(TrackState) * n_st, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t in_log = std::min<uint64_t>(cursor, t.log_cap), drop = t.dropped + (cursor - in_log);
    if (n_in_log) *n_in_log = in_log;
    if (dropped) *dropped = drop;
    if (n_taken) *n_taken = 0;
    if (travelled)  // (robots that joined since the last pass have not moved yet)
        for (size_t r = 0; r < R; r++) travelled[r] = r < n_st ? st[r].travelled : 0.0;
    if (capacity >= in_log) {  // the whole log, in (tick, robot) order — which lane won an atomic never shows — and the log is empty again
        if (in_log) {
            TrackSample *out = reinterpret_cast<TrackSample *>(samples);  // (the ABI's record is TrackSample's layout: mgx_tracks.hip asserts it)
            HIP_TRY(hipMemcpyAsync(out, t.log.p, sizeof(TrackSample) * (size_t)in_log, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            std::sort(out, out + in_log, [](const TrackSample &x, const TrackSample &y) { return x.tick != y.tick ? x.tick < y.tick : x.robot < y.robot; });
        }
        if (cursor) HIP_TRY(hipMemsetAsync(t.cursor.p, 0, sizeof(unsigned long long), s));
        t.dropped = drop;
        if (n_taken) *n_taken = in_log;
    }
    return check_device_error(w);
}

int mgx_tracks_clear(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->tracks.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    return tracks_reset(w);
}

int mgx_tracks_set_logging(mgx_world *w, int32_t on) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->tracks.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    w->tracks.logging = on != 0;  // (a kernel argument of the passes enqueued from now on)
    return MGX_OK;
}

int mgx_track_metrics_enable(mgx_world *w, int32_t enabled, uint32_t max_route_points) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Tracks &t = w->tracks;
    if (!t.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    if (!enabled) {
        if (t.metrics) HIP_TRY(hipStreamSynchronize(w->stream));
        metrics_drop(w);
        return MGX_OK;
    }
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "the trackers run on unsharded worlds");
    const uint32_t P = max_route_points ? max_route_points : METRICS_DEFAULT_ROUTE_POINTS;
    if (P < 2 || P > METRICS_MAX_ROUTE_POINTS) return fail(MGX_ERR_INVALID, "max_route_points must be in 2 .. %u, got %u", METRICS_MAX_ROUTE_POINTS, P);
    if (t.metrics) {
        if (max_route_points && P != t.max_route_points)
            return fail(MGX_ERR_STATE, "the run metrics are on with room for %u route points per robot", t.max_route_points);
        return MGX_OK;
    }
    t.max_route_points = P;
    t.m_sized = t.m_room = 0;
    t.metrics = true;
    const int rc = metrics_size(w);
    if (rc != MGX_OK) metrics_drop(w);
    return rc;
}

int mgx_track_metrics_set_route(mgx_world *w, int32_t robot, const double *xy, uint32_t n_points) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Tracks &t = w->tracks;
    if (!t.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    if (!t.metrics) return fail(MGX_ERR_STATE, "%s", METRICS_OFF);
    if (robot < 0 || (size_t)robot >= w->robots.size() || (!xy && n_points)) return fail(MGX_ERR_INVALID, "bad argument");
    if (n_points > t.max_route_points) return fail(MGX_ERR_INVALID, "a route of %u points, room for %u (mgx_track_metrics_enable)", n_points, t.max_route_points);
    const int rc = metrics_size(w);
    if (rc != MGX_OK) return rc;
    // the points and where they are: up from a pinned slot, behind the passes enqueued so far
    hipStream_t s = w->stream;
    const size_t P = t.max_route_points, xy_bytes = sizeof(double) * 2 * n_points;
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(xy_bytes + sizeof(TrackRoute), &hp, &slot));
    char *h = static_cast<char *>(hp);
    const TrackRoute rt{(uint32_t)((size_t)robot * P), n_points};
    if (xy_bytes) memcpy(h, xy, xy_bytes);
    memcpy(h + xy_bytes, &rt, sizeof rt);
    if (xy_bytes) HIP_TRY(hipMemcpyAsync(t.route_xy.p + 2 * (size_t)robot * P, h, xy_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(t.routes.p + robot, h + xy_bytes, sizeof rt, hipMemcpyHostToDevice, s));
    HIP_TRY(w->stage.release(slot, s));
    return MGX_OK;
}

int mgx_track_metrics_read(mgx_world *w, mgx_track_metrics *out, uint64_t capacity) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Tracks &t = w->tracks;
    if (!t.enabled) return fail(MGX_ERR_STATE, "%s", TRACKS_OFF);
    if (!t.metrics) return fail(MGX_ERR_STATE, "%s", METRICS_OFF);
    const size_t R = w->robots.size(), n = std::min(R, t.m_sized);
    if (capacity < R || (!out && R)) return fail(MGX_ERR_INVALID, "room for %llu records, %llu robots", (unsigned long long)capacity, (unsigned long long)R);
    MGX_CONFIRM(w);
    hipStream_t s = w->stream;
    TrackMetricsOut *o = reinterpret_cast<TrackMetricsOut *>(out);  // (the ABI's record is TrackMetricsOut's layout: mgx_tracks.hip asserts it)
    if (n) {
        HIP_TRY(t.mout.reserve(n));
        HIP_TRY(launch_track_metrics_read((int)n, t.mstate.p, t.mout.p, s));
        HIP_TRY(hipMemcpyAsync(o, t.mout.p, sizeof(TrackMetricsOut) * n, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t r = n; r < R; r++) {  // (robots that joined since the last pass: nothing sampled yet)
        o[r] = TrackMetricsOut{};
        o[r].dimensionless_jerk = __builtin_nan("");
    }
    return check_device_error(w);
}

}  // extern "C" (continued in the next part)
