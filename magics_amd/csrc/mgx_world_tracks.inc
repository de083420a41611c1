// mgx_world_tracks.inc — C ABI: the trackers on the device — PositionTracker / VelocityTracker samples and the distance every
// robot has travelled (the pass mgx_mission_tick_end enqueues beside the two collision passes).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// What a pass computes: mgx_tracks.hip; the specification: include/mgx.h.  The host's side here: the per-robot state follows the
// world's robots under the rule of mgx_world_observers.inc (robots that join make the arrays grow, zeroed), a pass is enqueued on
// the world's stream without a synchronisation or a read-back, and mgx_tracks_take is the call that waits.

static constexpr uint64_t TRACKS_DEFAULT_SAMPLES = 1ull << 18;  // 10 MB of 40-byte records
static const char *const TRACKS_OFF = "the trackers are off (mgx_tracks_enable)";
static const char *const TRACKS_UNSHARDED = "the trackers run on unsharded worlds";

static const char *const METRICS_OFF = "the run metrics are off (mgx_track_metrics_enable)";
static constexpr uint32_t METRICS_DEFAULT_ROUTE_POINTS = 16, METRICS_MAX_ROUTE_POINTS = 1u << 16;

static void metrics_drop(mgx_world *w) {
    mgx_world::Tracks &t = w->tracks;
    t.metrics = false;
    t.mstate.release(); t.route_xy.release(); t.routes.release(); t.mout.release();
    t.max_route_points = 0;
}

static void tracks_drop(mgx_world *w) {  // switched off: the state goes with it
    mgx_world::Tracks &t = w->tracks;
    metrics_drop(w);
    t.logging = true;
    t.enabled = false;
    t.state.release(); t.log.release(); t.cursor.release();
    t.n_sized = 0; t.log_cap = 0; t.period_ns = 0; t.tick_ns = 0; t.clock = 0; t.dropped = 0;
}

// the state array and, while the run metrics are on, their three arrays (`routes` grows last: where it has room, all three have) for
// the robots the world has NOW: the robots so far keep state and route, the others start from zero and without a route
static int tracks_size(mgx_world *w) {
    mgx_world::Tracks &t = w->tracks;
    const size_t R = w->robots.size(), P = t.max_route_points, room = observers_room(w, R);
    const bool metrics = t.metrics && R > t.routes.cap;
    if (R <= t.n_sized && !metrics) return MGX_OK;
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", TRACKS_UNSHARDED);
    Outgrown out{w->stream};
    if (R > t.state.cap) HIP_TRY(out.grow(t.state, room, t.n_sized, 0));
    if (metrics) {
        HIP_TRY(out.grow(t.mstate, room, t.n_sized, 0));
        HIP_TRY(out.grow(t.route_xy, room * P * 2, t.n_sized * P * 2, 0));
        HIP_TRY(out.grow(t.routes, room, t.n_sized, 0));
    }
    HIP_TRY(out.retire());
    t.n_sized = R;
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
    if (t.metrics) { d.metrics = t.mstate.p; d.route_xy = t.route_xy.p; d.routes = t.routes.p; d.max_route_points = t.max_route_points; }
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
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", TRACKS_UNSHARDED);
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
    ObserverInputs in;  // the caller's positions and who moved (a robot that is gone never does)
    const int rc = observers_update_begin(w, w && w->tracks.enabled, TRACKS_OFF, TRACKS_UNSHARDED, nullptr, positions_xyz, moved, in);
    if (rc != MGX_OK || !in.flags) return rc;
    return tracks_pass(w, in.pos, in.flags, tick, false, w->stream);
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
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "%s", TRACKS_UNSHARDED);
    const uint32_t P = max_route_points ? max_route_points : METRICS_DEFAULT_ROUTE_POINTS;
    if (P < 2 || P > METRICS_MAX_ROUTE_POINTS) return fail(MGX_ERR_INVALID, "max_route_points must be in 2 .. %u, got %u", METRICS_MAX_ROUTE_POINTS, P);
    if (t.metrics) {
        if (max_route_points && P != t.max_route_points)
            return fail(MGX_ERR_STATE, "the run metrics are on with room for %u route points per robot", t.max_route_points);
        return MGX_OK;
    }
    t.max_route_points = P;
    t.metrics = true;
    const int rc = tracks_size(w);
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
    const int rc = tracks_size(w);
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
    const size_t R = w->robots.size(), n = std::min(R, t.n_sized);
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
