// mgx_world_launch.inc — launches: confirm_resident, sweep, resident schedule launches, lingering launches (the host's side).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// ---- launches -----------------------------------------------------------------------------------------
static int direct_exchange(mgx_world *w);
static int rccl_exchange(mgx_world *w);
static int sweep(mgx_world *w, int32_t robot, uint32_t ext_mask, uint32_t int_mask, int n_int, uint32_t hints = 0);
static void log_launch(mgx_world *w, int robot, uint32_t ext_mask, uint32_t int_mask, int n_int);

static void log_plan(mgx_world *w, const std::vector<Launch> &plan, size_t from = 0, size_t n = ~(size_t)0) {
    for (size_t k = from; k < plan.size() && k - from < n; k++) log_launch(w, -1, plan[k].ext, int_phases(plan[k]), plan[k].n_int);
}
// A masked world whose schedules may run resident (mgx_set_group_enabled + mgx_set_group_resident): the form of its launches reads
// the robots' groups and the groups' kinds (SWEEP_F_GRP, mgx_dev.h)
static bool masked_resident(const mgx_world *w) { return w->gkinds.masked() && w->gkinds.resident; }
static int run_masked_plan(mgx_world *w, const std::vector<Launch> &plan);
// Prior updates that were to ride in a schedule, sent as the kernel of their own instead (no launch of a group plan carries
// them): mgx_tick's records — one per device robot, (waypoint, time scale, what) — become mgx_update_priors' lists; the
// mission's are in device memory, where launch_mission_prepare wrote the lists beside them.
static int send_riding_updates(mgx_world *w, const RidingUpdates &upd) {
    if (!upd.any()) return MGX_OK;
    if (!upd.host) {
        const mgx_world::Mission &ms = w->mission;
        if (upd.dev != ms.rec_d.p) return fail(MGX_ERR_STATE, "internal: riding prior updates in device memory that are not the mission's");
        HIP_TRY(launch_update_priors(w->d, (int)w->robots.size(), ms.robots_d.p, ms.waypoints_d.p, ms.ts_list_d.p, ms.what_d.p, upd.max_speed, upd.delta_t, w->stream));
        return MGX_OK;
    }
    // (copied out first: the records may sit in a ring slot already released, which the acquire below could hand out again)
    const size_t RL = (size_t)w->d.R_local;
    const std::vector<double> rec(upd.host, upd.host + 4 * RL);
    std::vector<int32_t> who;
    for (size_t dr = 0; dr < RL; dr++)
        if (rec[4 * dr + 3] != 0.0) who.push_back((int32_t)dr);
    const size_t n = who.size();
    if (n == 0) return MGX_OK;
    // packed arguments, f64 words: waypoints[2n] | time_scale[n] | device robot (int32)[n] | what (u8)[n]
    const size_t w_r = (n + 1) / 2, w_w = (n + 7) / 8, words = 3 * n + w_r + w_w;
    void *hp = nullptr, *dp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(words * sizeof(double), &hp, &slot));
    double *hw = (double *)hp;
    int32_t *hr = (int32_t *)(hw + 3 * n);
    uint8_t *hh = (uint8_t *)(hw + 3 * n + w_r);
    for (size_t i = 0; i < n; i++) {
        const double *q = &rec[4 * (size_t)who[i]];
        hw[2 * i] = q[0]; hw[2 * i + 1] = q[1]; hw[2 * n + i] = q[2];
        hr[i] = who[i];
        hh[i] = (uint8_t)q[3];
    }
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    const double *dw = (const double *)dp;
    HIP_TRY(launch_update_priors(w->d, (int)n, (const int32_t *)(dw + 3 * n), dw, dw + 2 * n, (const uint8_t *)(dw + 3 * n + w_r), upd.max_speed,
                                 upd.delta_t, w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    return MGX_OK;
}
// Runs `plan` from segment `from` on launch by launch.  Prior updates ride in the first of these launches only, and the pinned
// ring slot they sit in is released behind it (an event-record error is reported only if the sweep itself succeeded).
// A masked world comes here only with mgx_set_group_resident on, from a schedule that could not run (or go on) resident: the
// riding updates go out as the kernel of their own, then the segments left are ONE group plan (run_masked_plan).
static int run_segments(mgx_world *w, const std::vector<Launch> &plan, size_t from, const RidingUpdates &upd) {
    if (w->gkinds.masked()) {
        int rc = send_riding_updates(w, upd);
        if (upd.slot >= 0) {
            const hipError_t e = w->stage.release(upd.slot, w->stream);
            if (rc == MGX_OK && e != hipSuccess) rc = fail(MGX_ERR_HIP, "event record: %s", hipGetErrorString(e));
        }
        if (rc != MGX_OK) return rc;
        w->gkinds.res_fallbacks++;
        if (from == 0) return run_masked_plan(w, plan);
        return run_masked_plan(w, std::vector<Launch>(plan.begin() + (long)std::min(from, plan.size()), plan.end()));
    }
    for (size_t k = from; k < plan.size(); k++) {
        const bool rides = k == from && upd.dev;
        if (rides) { w->d.upd = upd.dev; w->d.upd_max_speed = upd.max_speed; w->d.upd_delta_t = upd.delta_t; }
        int rc = sweep(w, -1, plan[k].ext, int_phases(plan[k]), plan[k].n_int, plan[k].hints);
        w->d.upd = nullptr;
        if (rides && upd.slot >= 0) {
            const hipError_t e = w->stage.release(upd.slot, w->stream);
            if (rc == MGX_OK && e != hipSuccess) rc = fail(MGX_ERR_HIP, "event record: %s", hipGetErrorString(e));
        }
        if (rc != MGX_OK) return rc;
    }
    return MGX_OK;
}
// Looks (`done`: non-zero ends the looking and is returned) for 30 s at the most, the clock read every 2^20 looks: -1 then, and
// the caller says what never happened.  No runtime call in this loop: a stream query per look made the runtime put markers
// between the launches.
template <class F>
static int spin_until(F done) {
    const double t0 = StageTimer::now();
    for (unsigned spins = 0;; spins++) {
        const int r = done();
        if (r) return r;
        if ((spins & 0xfffffu) == 0xfffffu && StageTimer::now() - t0 > 30e6) return -1;
    }
}
static Standing standing(const mgx_world *w) { return {w->d.cur, w->res.flag_base}; }
static void stand_at(mgx_world *w, const Standing &s) { w->d.cur = s.cur; w->res.flag_base = s.flag_base; }
void Submitted::take_back(mgx_world *w) {
    stand_at(w, before);
    w->last_sweep_launches = 0;  // (how the schedule runs after all is what mgx_last_launch_count says of it)
}

// A resident schedule launch decides for itself, before it writes anything, whether all its workgroups are on the device
// together (SegPlan: residency census) — and if another tenant of the GPU holds the CUs its tail needs, it returns at once
// and leaves the world untouched.  The host must not put anything behind a launch whose decision it has not seen (what
// follows would run on the wrong state), so every entry point that enqueues work or reads state comes through here first:
// the decision falls within microseconds of the launch's START, so in a stream of ticks the host simply stays ONE launch
// ahead of the device instead of many.  An aborted launch is run again on the launch-per-segment path, and the next few
// schedules skip the resident form (doubling back-off while the GPU stays shared).  Nothing pending: returns at once.
static int confirm_resident(mgx_world *w, bool rerun, int32_t *outcome) {
    ResidentLaunches &rl = w->res;
    Submitted &pd = rl.pending;
    if (outcome) *outcome = MGX_RESIDENT_NONE;
    if (!pd.active) return MGX_OK;
    StageTimer clock("confirm");
    unsigned long long v = 0;
    const int decided = spin_until([&] { v = __atomic_load_n(rl.decision_host(), __ATOMIC_ACQUIRE); return (v >> 2) >= pd.number ? 1 : 0; });
    pd.active = false;
    // the launch never started (a stuck stream): nothing sensible is left to do
    if (decided < 0) return fail(MGX_ERR_STATE, "resident launch %llu was never decided (the stream does not advance)", pd.number);
    clock.lap((v & 3ull) == RESIDENT_ABORT ? "launch ABORTED" : "launch decided: go");
    if ((v >> 2) == pd.number && (v & 3ull) == RESIDENT_ABORT) {
        // nothing happened on the device: take the host's bookkeeping back and run the same schedule launch by launch
        rl.aborts++;
        if (rl.linger.open && rl.linger.seq0 == pd.number) rl.linger.open = false;  // (its decider left with the verdict: nobody lingers)
        rl.backoff.declined((int)pd.plan.size());
        pd.take_back(w);
        if (!rerun && !pd.upd.any() && !pd.partial) {  // mgx_resident_outcome: the caller issues the schedule again
            if (outcome) *outcome = MGX_RESIDENT_DECLINED;
            return MGX_OK;
        }
        if (outcome) *outcome = MGX_RESIDENT_RAN;  // (by the time the caller looks, it has: launch by launch)
        // (the ring slot of the prior updates was released behind the declined launch, which returned at once: the re-run guards it
        // again, or the ring would hand it out — or free it — while the kernel just enqueued has yet to read them)
        return run_segments(w, pd.plan, 0, pd.upd);
    }
    rl.backoff.went_ahead();
    if (outcome) *outcome = MGX_RESIDENT_RAN;
    log_plan(w, pd.plan);
    return MGX_OK;
}
// ... on the way to the next schedule or into the open launch: a declined launch is run again without ending a launch that
// lingers (commit would), and its launches are not the coming schedule's
static int confirm_held(mgx_world *w) {
    bool &hold = w->res.linger.hold;
    const bool held = hold;
    hold = true;
    const int rc = confirm_resident(w);
    hold = held;
    return rc;
}
static int commit_held(mgx_world *w) {  // mgx_tick: a lingering launch stays — the tick is posted into it if it qualifies
    w->res.linger.hold = true;
    const int rc = commit(w);
    w->res.linger.hold = false;
    return rc;
}
static int run_masked_launch(mgx_world *w, uint32_t ext_mask, uint32_t int_mask, int n_int, uint32_t hints);
static int sweep(mgx_world *w, int32_t robot, uint32_t ext_mask, uint32_t int_mask, int n_int, uint32_t hints) {
    // A masked world (mgx_set_group_enabled): a world-wide sweep is a group plan of one launch, every group the same segment
    if (robot < 0 && w->gkinds.masked()) return run_masked_launch(w, ext_mask, int_mask, n_int, hints);
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    if ((rc = check_device_error(w)) != MGX_OK) return rc;
    if (!w->robots.empty()) w->stale_kinds |= ~w->p.enable_mask & 15u;  // disabled factors miss what this sweep delivers
    const bool writes_snap = (int_mask & PH_INT_VARIABLE) && n_int > 0;
    if (robot < 0 && ext_mask && w->thaw_kinds && (int_mask & PH_INT_FACTOR) && n_int > 0) {
        // Factors that come back from being switched off take their first update in front of the sweep launch (k_thaw
        // writes their messages into the robots' images).  An external variable sweep at the head of the same launch
        // would sum those new messages where the reference still sums the stale ones — its beliefs are overwritten by
        // the internal sweep that follows, but the means it hands to the neighbours' factors are not.  So the external
        // iteration runs as a launch of its own first.
        rc = sweep(w, -1, ext_mask, 0, 0, 0);
        return rc != MGX_OK ? rc : sweep(w, -1, 0, int_mask, n_int, hints & ~HINT_IR_DEAD);
    }
    if (robot < 0) {
        if (ext_mask) w->res.backoff.external_iteration();
        if (w->direct.connected && (ext_mask & PH_EXT_FACTOR)) {  // the inter-robot factors read the ghosts' snapshots
            rc = direct_exchange(w);
            if (rc != MGX_OK) return rc;
        } else if (w->rccl.connected && (ext_mask & PH_EXT_FACTOR)) {
            rc = rccl_exchange(w);
            if (rc != MGX_OK) return rc;
        }
        const int out = writes_snap ? 1 - w->d.cur : -1;
        const bool thawing = w->thaw_kinds && (int_mask & PH_INT_FACTOR) && n_int > 0;
        if (thawing) HIP_TRY(launch_thaw(w->d, 0, w->d.R_local, ext_mask, w->stream));
        if (w->n_keyless > 0 && (ext_mask & PH_EXT_FACTOR) && (w->p.enable_mask & 2u)) {
            // factors created while their kind was switched off and not yet in possession of both inbox keys (KeylessRec):
            // the keys fill structurally, so the log says which ones are there now
            flush_counts(w);
            std::vector<KeylessRec> recs;
            for (size_t ci = 0; ci < w->conns.size(); ci++) {
                const IrConn &c = w->conns[ci];
                const int32_t dev_slot = dev_slot_of(w, ci);
                if (c.keys.empty() || dev_slot < 0) continue;
                const int tr = w->dev_of[(size_t)c.other];
                for (size_t j = 0; j < c.keys.size(); j++)
                    recs.push_back(KeylessRec{(int32_t)edge_index(w->dev_in_ptr, w->K, tr, (int)j, dev_slot), tr, (uint32_t)c.keys[j], 0u});
            }
            if (!recs.empty()) {
                void *hp = nullptr, *dp = nullptr;
                int slot = 0;
                HIP_TRY(w->stage.acquire(sizeof(KeylessRec) * recs.size(), &hp, &slot));
                memcpy(hp, recs.data(), sizeof(KeylessRec) * recs.size());
                HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
                HIP_TRY(launch_keyless_ir(w->d, w->ir_gate.p, (int)recs.size(), (const KeylessRec *)dp, w->stream));
                HIP_TRY(w->stage.release(slot, w->stream));
                w->flags_dirty = true;  // the gate bytes go back to 0 / 1 in front of the next launch
            }
        }
        if (w->ir_thaw_active && (ext_mask & PH_EXT_FACTOR) && w->d.NI > 0 && !w->conns.empty())
            HIP_TRY(launch_thaw_ir(w->d, w->ir_gate.p, w->stream));
        HIP_TRY(launch_robot_sweep(w->d, 0, w->d.R_local, ext_mask, int_mask, n_int, out, hints, w->stream, &w->last_sweep));
        w->last_sweep_form = MGX_SWEEP_FORM_SEGMENTS;
        w->last_sweep_launches++;
        if (w->ir_thaw_active && writes_snap) {  // once every robot has run an internal variable sweep, every owner has delivered
            bool all_take_part = true;  // ghosts count: their owners' flags are kept here too, and their records arrive by exchange
            for (const Robot &rb : w->robots) all_take_part = all_take_part && (rb.removed || !rb.idle);
            if (all_take_part) {
                w->ir_thaw_active = false;
                w->d.ir_frozen_snap = nullptr; w->d.ir_frozen_epoch = nullptr; w->d.ir_thaw_epoch = nullptr;
                for (Robot &rb : w->robots) rb.ir_thaw_epoch.clear();
                w->flags_dirty = true;  // gate bytes back to 0 / 1
            }
        }
        if (w->thaw_kinds && (thawing || writes_snap)) {
            HIP_TRY(launch_thaw_done(w->d, 0, w->d.R_local, writes_snap ? 1 : 0, w->stream));
            bool all_take_part = true;  // idle robots keep thawing until they iterate again
            for (const Robot &rb : w->robots) all_take_part = all_take_part && (rb.ghost || rb.removed || !rb.idle);
            if (writes_snap && all_take_part) { w->thaw_kinds = 0; w->d.skip0 = nullptr; }
        }
        if (writes_snap) w->d.cur ^= 1;
        log_launch(w, -1, ext_mask, int_mask, n_int);
    } else {
        if ((size_t)robot >= w->robots.size() || w->robots[(size_t)robot].ghost) return fail(MGX_ERR_INVALID, "bad robot id %d", robot);
        if (ext_mask) return fail(MGX_ERR_INVALID, "external sweeps are world-wide (robot must be -1)");
        // single workgroup: nobody else reads the snapshot buffer concurrently => update in place
        const bool thawing = w->thaw_kinds && (int_mask & PH_INT_FACTOR) && n_int > 0;
        if (thawing) HIP_TRY(launch_thaw(w->d, w->dev_of[(size_t)robot], 1, 0, w->stream));
        // (one robot, one group: its kinds are the launch's own scalar — mgx_set_group_enabled)
        // (... and so are its sigmas — mgx_set_group_sigmas: the launch's three 1 / sigma^2, formed as commit forms the world's)
        w->d.enable = w->kinds_of_robot((size_t)robot);
        const double world_s2[3] = {w->d.inv_s2_obs, w->d.inv_s2_ir, w->d.inv_s2_trk};
        if (w->gkinds.n_sigma) {
            const mgx_group_sigmas gsg = w->sigmas_of_group(w->sets.group[(size_t)robot]);
            w->d.inv_s2_obs = 1.0 / (gsg.obstacle * gsg.obstacle);
            w->d.inv_s2_ir = 1.0 / (gsg.interrobot * gsg.interrobot);
            w->d.inv_s2_trk = 1.0 / (gsg.tracking * gsg.tracking);
        }
        const hipError_t le = launch_robot_sweep(w->d, w->dev_of[(size_t)robot], 1, 0, int_mask, n_int, writes_snap ? w->d.cur : -1, 0, w->stream,
                                                 &w->last_sweep);
        w->d.enable = w->p.enable_mask;
        w->d.inv_s2_obs = world_s2[0]; w->d.inv_s2_ir = world_s2[1]; w->d.inv_s2_trk = world_s2[2];
        HIP_TRY(le);
        w->last_sweep_form = MGX_SWEEP_FORM_SEGMENTS;
        if (w->thaw_kinds && (thawing || writes_snap)) HIP_TRY(launch_thaw_done(w->d, w->dev_of[(size_t)robot], 1, writes_snap ? 1 : 0, w->stream));
        log_launch(w, robot, 0, int_mask, n_int);
    }
    return MGX_OK;
}

// ---- resident schedule launches: a whole mgx_iterate / mgx_tick schedule in ONE launch -----------------------

// The environment's knobs of resident launches, each read once per process when it is first asked for (MGX_LINGER and
// MGX_LINGER_US: per world, linger_ticks).  Times become ticks of the 100 MHz wall clock.
struct ResidentKnobs {
    static long long positive(const char *name, long long dflt) { const char *e = getenv(name); const long long v = e ? atoll(e) : dflt; return v > 0 ? v : dflt; }
    static bool persistent() { static const bool v = [] { const char *e = getenv("MGX_PERSISTENT"); return !(e && e[0] == '0'); }(); return v; }  // 0: every schedule launch by launch
    static long long timeout_ticks() { static const long long v = positive("MGX_RESIDENT_TIMEOUT_MS", 2000) * 100000ll; return v; }  // a wait inside a launch
    static bool census() { static const bool v = [] { const char *e = getenv("MGX_RESIDENT_CENSUS"); return !(e && e[0] == '0'); }(); return v; }  // 0: plain bound on every wait
    static long long census_ticks() { static const long long v = positive("MGX_RESIDENT_CENSUS_US", 200) * 100ll; return v; }
    static long long census_ticks_sharded() { static const long long v = positive("MGX_RESIDENT_CENSUS_SHARDED_US", 20000) * 100ll; return v; }  // the ranks' hosts do not launch at the same instant
    // 1: hipLaunchCooperativeKernel — the runtime checks the grid against the occupancy query at launch time (same residency as a
    // plain launch, +15..19 us of host time per launch: MI355X_MICROARCH.md); a grid it turns down takes the launch-per-segment
    // path from now on instead of waiting for workgroups that never become resident
    static bool cooperative() { static const bool v = [] { const char *e = getenv("MGX_COOPERATIVE"); return e && e[0] == '1'; }(); return v; }
    static int32_t post_merge() {  // 0: every schedule its own post; 1 (default): merged while the launch is behind; 2: whenever they fit
        const char *e = getenv("MGX_POST_MERGE");
        return e && e[0] >= '0' && e[0] <= '2' && !e[1] ? e[0] - '0' : POST_MERGE_AUTO;
    }
    static int32_t specialize() { const char *e = getenv("MGX_SPECIALIZE"); return !(e && e[0] == '0'); }  // 0: every resident launch in the full form
    static long long linger_ticks() {  // microseconds a workgroup waits for the next schedule before it ends the launch
        const char *off = getenv("MGX_LINGER"), *us = getenv("MGX_LINGER_US");
        const long long v = off && off[0] == '0' ? 0 : us ? atoll(us) : 300;
        return (v > 0 ? std::min<long long>(v, 1000000) : 0) * 100ll;
    }
};
static bool resident_enabled() { return ResidentKnobs::persistent(); }
// The launches' words and tables for the device arrays as they are now.  The peer table: the robots each local robot exchanges snapshot records with: owners of its incoming connections and targets of
// its outgoing ones (the latter matter when the reference's bookkeeping has left a connection one-sided)
static int ensure_resident_tables(mgx_world *w) {
    hipStream_t s = w->stream;
    const size_t R = (size_t)w->d.R_local;
    if (!w->res.sweep_abort_buf.p) {
        std::vector<unsigned long long> z(1, 0ull);
        HIP_TRY(w->res.sweep_abort_buf.upload(z, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (w->res.sweep_flag_buf.n != R) {
        HIP_TRY(w->res.sweep_flag_buf.reserve(R));
        HIP_TRY(hipMemsetAsync(w->res.sweep_flag_buf.p, 0, sizeof(unsigned long long) * R, s));
        w->res.flag_base = 0;
        // ... and with the segment count the exchange records start over: zeroed, so that no sequence word of an earlier life
        // of the device arrays validates (a valid word has its top bit set, mgx_dev.h)
        const size_t xb = R * (size_t)w->K * (size_t)XREC_BYTES;
        HIP_TRY(w->res.xrec_buf.reserve(2 * xb));
        HIP_TRY(hipMemsetAsync(w->res.xrec_buf.p, 0, 2 * xb, s));
    }
    {
        const size_t xb = R * (size_t)w->K * (size_t)XREC_BYTES;
        w->d.xrec[0] = w->res.xrec_buf.p;
        w->d.xrec[1] = w->res.xrec_buf.p ? w->res.xrec_buf.p + xb : nullptr;
    }
    if (w->res.census_buf.n < R + 1) {  // residency census: one word per workgroup of a launch (never reset: monotonic in the launch number)
        std::vector<unsigned long long> z(R + 1 + R / 4 + 64, 0ull);
        HIP_TRY(w->res.census_buf.upload(z, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (!w->res.decision_buf.p) {  // the decision word and its host-mapped copy
        std::vector<unsigned long long> z1(1, 0ull);
        HIP_TRY(w->res.decision_buf.upload(z1, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(w->res.decision_mem.alloc(sizeof(unsigned long long)));
    }
    {
        void *dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, w->res.decision_host(), 0));
        w->d.census = w->res.census_buf.p;
        w->d.decision = w->res.decision_buf.p;
        w->d.decision_host = (unsigned long long *)dp;
    }
    if (!w->res.peers_valid) {
        // (lists of the LOCAL robots; a ghost — device index >= R — appears in them as a peer, its word lives in the ghost area.)
        // A list is what its robot's polling lanes walk, nothing more: its order carries no meaning and a robot that is both the
        // owner of an incoming and the target of an outgoing connection — the rule — may stand in it twice (two lanes look at
        // the same word).  So the table is two passes over the connections, written straight into the pinned block it travels
        // in ([R + 1 row pointers | entries], ONE copy): a world that follows its topology builds it every tick.
        const size_t n_conns = w->conns.size();
        const IrConn *conns = w->conns.data();
        const int32_t *dev_of = w->dev_of.data();
        void *hp = nullptr;
        int slot = 0;
        const size_t words = R + 1 + std::max<size_t>(2 * n_conns, 1);
        HIP_TRY(w->stage.acquire(sizeof(int32_t) * words, &hp, &slot));
        int32_t *ptr = (int32_t *)hp, *idx = ptr + R + 1;
        std::fill(ptr, ptr + R + 1, 0);
        for (size_t ci = 0; ci < n_conns; ci++) {
            const size_t o = (size_t)dev_of[(size_t)conns[ci].owner], t = (size_t)dev_of[(size_t)conns[ci].other];
            if (o < R) ptr[o + 1]++;
            if (t < R) ptr[t + 1]++;
        }
        for (size_t r = 0; r < R; r++) ptr[r + 1] += ptr[r];
        std::vector<int32_t> &fill = w->res.peer_fill;
        fill.assign(ptr, ptr + R);
        for (size_t ci = 0; ci < n_conns; ci++) {
            const int o = dev_of[(size_t)conns[ci].owner], t = dev_of[(size_t)conns[ci].other];
            if ((size_t)o < R) idx[(size_t)fill[(size_t)o]++] = t;
            if ((size_t)t < R) idx[(size_t)fill[(size_t)t]++] = o;
        }
        if (ptr[R] == 0) idx[0] = 0;
        HIP_TRY(w->res.peer_ptr_dev.reserve(words));
        HIP_TRY(hipMemcpyAsync(w->res.peer_ptr_dev.p, hp, sizeof(int32_t) * (R + 1 + (size_t)std::max(ptr[R], 1)), hipMemcpyHostToDevice, s));
        HIP_TRY(w->stage.release(slot, s));
        w->res.peer_idx_off = R + 1;
        w->res.peers_valid = true;
    }
    w->d.sweep_flag = w->res.sweep_flag_buf.p;
    w->d.sweep_abort = w->res.sweep_abort_buf.p;
    w->d.peer_ptr = w->res.peer_ptr_dev.p;
    w->d.peer_idx = w->res.peer_ptr_dev.p + w->res.peer_idx_off;
    return MGX_OK;
}
// the conditions every rank of a sharded world decides alike on: same schedule, same world-wide switches, the same back-off
// (aborts are the ranks' common answer)
static bool resident_gate(const mgx_world *w, const std::vector<Launch> &plan) {
    if (!resident_enabled() || w->res.mode == ResidentLaunches::OFF || plan.size() < 2) return false;
    if (w->res.backoff.left > 0) return false;  // a recent launch found the GPU shared (residency census): launch by launch for a while
    // enabled kinds per group (mgx_set_group_enabled): the resident kernel reads the world's only — but for its masked form, which
    // the world has to ask for (mgx_set_group_resident)
    if (w->gkinds.masked() && (!w->gkinds.resident || w->xres.connected)) return false;
    const DevWorld &d = w->d;
    const bool sharded = w->xres.connected;  // the ranks have agreed (mgx_halo_resident_connect_peers) that ghost records travel inside the launches
    if ((d.R_total != d.R_local && !sharded) || !(w->p.enable_mask & 2u)) return false;
    if (((w->direct.connected || w->rccl.connected) && !sharded)) return false;
    for (const Launch &l : plan)
        if (l.n_int > 255) return false;
    if (sharded && plan[0].ext && !w->direct.connected) return false;  // the exchange in front of the launch is the direct one
    return true;
}
// What this world's OWN launch needs, beyond the gate: inter-robot factors staged in LDS, nothing thawing or without its inbox
// keys, not told to decline, the workgroup's LDS footprint, and every workgroup — with the residency census' decider, for which
// one slot is kept free — on the device at once.  The callers draw their own consequences.
enum ResidentFit { FITS, UNFIT_NOW, UNFIT_LDS, UNFIT_CAPACITY };
// The form of the world's next resident launch (SWEEP_F_*, mgx_dev.h): tracking code only where tracking factors are enabled,
// the prior-update path only where the launch's own schedule carries updates or the world has seen some (ResidentLaunches).
static uint32_t resident_features(mgx_world *w, bool carries_updates) {
    ResidentLaunches &rl = w->res;
    if (masked_resident(w)) return SWEEP_F_GRP | SWEEP_F_ALL;  // (the one masked form, whatever mgx_set_specialize says)
    if (rl.specialize < 0) rl.specialize = ResidentKnobs::specialize();
    if (!rl.specialize) return SWEEP_F_ALL;
    const uint32_t f = ((w->p.enable_mask & 8u) ? SWEEP_F_TRK : 0u) | ((carries_updates || rl.upd_seen) ? SWEEP_F_UPD : 0u);
    return sweep_resident_form(w->K, f);
}
// The resident kernels take "nothing thaws" for granted (mgx_sweep.h: skip0 is a constant 0 there): every door to them —
// resident_fits for a launch, linger_world_qualifies for a post — is shut while a kind thaws, and this says so once more where
// the launch is made.
static bool resident_launch_allowed(const mgx_world *w) { return !w->thaw_kinds && !w->ir_thaw_active && w->d.skip0 == nullptr; }
static ResidentFit resident_fits(mgx_world *w, bool sharded, uint32_t form) {
    const DevWorld &d = w->d;
    if (!(d.ir_max_edges > 0 && !w->conns.empty() && !w->thaw_kinds && !w->ir_thaw_active && w->n_keyless == 0 && w->res.mode != ResidentLaunches::DECLINE))
        return UNFIT_NOW;
    if (sweep_lds_bytes(w->K, d.ir_max_edges, true) > sweep_resident_lds_max()) return UNFIT_LDS;
    return d.R_local + 1 > w->res.capacity_for(d, sharded, form) ? UNFIT_CAPACITY : FITS;
}

// ---- lingering resident launches: the host's side (mgx_dev.h; the device's side is in mgx_sweep.h) --------------------------
static int run_resident(mgx_world *w, const std::vector<Launch> &plan);
static long long linger_ticks(mgx_world *w) {  // (per world: asked at its first use, and again after mgx_set_linger(w, -1))
    ResidentLaunches::Linger &lg = w->res.linger;
    if (lg.ticks < 0) lg.ticks = ResidentKnobs::linger_ticks();
    return lg.ticks;
}
static int32_t post_merge_mode(mgx_world *w) {  // (per world: asked at its first use, and again after mgx_set_post_merge(w, -1))
    ResidentLaunches::Linger &lg = w->res.linger;
    if (lg.merge_mode < 0) lg.merge_mode = ResidentKnobs::post_merge();
    return lg.merge_mode;
}
static double *linger_upd_slot(mgx_world *w, unsigned long long number) {
    ResidentLaunches::Linger &lg = w->res.linger;
    return reinterpret_cast<double *>(reinterpret_cast<char *>(lg.box()) + sizeof(LingerBox)) + (size_t)(number & 1ull) * lg.upd_stride;
}
// the box (host-mapped: header, two plan slots, two blocks of prior-update records) and the go word; never while a launch lingers
static int ensure_linger_box(mgx_world *w) {
    ResidentLaunches::Linger &lg = w->res.linger;
    const size_t stride = ((size_t)4 * (size_t)std::max(w->d.R_local, 1) + 7) & ~(size_t)7;
    if (!lg.go.p) {
        std::vector<unsigned long long> z(1, 0ull);
        HIP_TRY(lg.go.upload(z, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (lg.box() && lg.upd_stride >= stride) return MGX_OK;
    const size_t grown = (stride + stride / 2 + 7) & ~(size_t)7;
    HIP_TRY(lg.box_mem.alloc(sizeof(LingerBox) + 2 * grown * sizeof(double)));
    lg.upd_stride = grown;
    lg.dev_stride = LINGER_SLOT_HEAD + (size_t)LINGER_UPD_BYTES * (grown / 4);  // the plan's chunks, then three chunks per robot (mgx_dev.h)
    HIP_TRY(lg.dev.reserve(2 * lg.dev_stride));
    HIP_TRY(hipMemsetAsync(lg.dev.p, 0, 2 * lg.dev_stride, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return MGX_OK;
}
// Spins (bounded) until `pred` holds: 0; or until the launch has ended (its go word went odd and the postman said so): 1.
template <class F>
static int linger_wait(mgx_world *w, F pred, const char *what) {
    ResidentLaunches::Linger &lg = w->res.linger;
    const int r = spin_until([&] {
        if (pred()) return 1;
        const unsigned long long c = __atomic_load_n(&lg.box()->closed, __ATOMIC_ACQUIRE);
        return (c & 1ull) && (c >> 1) >= lg.seq0 ? 2 : 0;
    });
    if (r < 0) return fail(MGX_ERR_STATE, "lingering launch %llu: no answer from the device while waiting for %s (the stream does not advance)", lg.seq0, what);
    return r - 1;
}
// a post the launch has taken: it runs (or has run) behind everything before it — its launches enter the counters' log
static void linger_confirm(mgx_world *w) {
    ResidentLaunches::Linger &lg = w->res.linger;
    log_plan(w, lg.un.plan);
    lg.un.active = false;
    lg.posts += lg.un.schedules;
    lg.taken_in_launch++;
}
// Submits `plan` with `upd` riding in it: posted or as resident launches where the world qualifies, launch by launch where not.
// The one place where a schedule's prior updates are set on the world, and cleared.  lap: the caller's stage clock (mgx_tick).
static int run_schedule(mgx_world *w, const std::vector<Launch> &plan, const RidingUpdates &upd, StageTimer *lap = nullptr) {
    // (a masked world: never posted, never resident — its callers send the prior updates as the kernel of their own — unless it
    // asked for the masked form: mgx_set_group_resident.  Then it goes the way of every world, and run_segments is its fall-back.)
    if (w->gkinds.masked() && !w->gkinds.resident) {
        if (upd.any()) return fail(MGX_ERR_STATE, "internal: prior updates riding in a masked world's schedule");
        return run_masked_plan(w, plan);
    }
    const RidingUpdates outer = w->res.riding;  // (none — unless this is a post taken back on the way to the schedule that follows it)
    w->res.riding = upd;
    const int resident = run_resident(w, plan);
    w->res.riding = outer;
    if (lap) lap->lap("resident launch enqueued");
    if (resident == 0) return run_segments(w, plan, 0, upd);
    const hipError_t e = upd.slot >= 0 ? w->stage.release(upd.slot, w->stream) : hipSuccess;
    if (resident < 0) return resident;
    return e == hipSuccess ? MGX_OK : fail(MGX_ERR_HIP, "event record: %s", hipGetErrorString(e));
}
// The launch has ended (closed word c = 2 S + 1: behind plan S).  A post it never took is taken back and run as a launch of its
// own — from the same records, nothing lost and nothing twice.
static int linger_settle(mgx_world *w, bool nested = false) {  // nested: on the way to the NEXT schedule (whose launches are counted apart)
    ResidentLaunches::Linger &lg = w->res.linger;
    const uint32_t count_before = w->last_sweep_launches;
    const unsigned long long c = __atomic_load_n(&lg.box()->closed, __ATOMIC_ACQUIRE);
    lg.open = false;
    int rc = MGX_OK;
    if (lg.un.active && (c >> 1) >= lg.un.number) {
        linger_confirm(w);
    } else if (lg.un.active) {
        Submitted un = std::move(lg.un);
        lg.un = Submitted{};
        lg.reruns += un.schedules;
        if (lg.ran.features & SWEEP_F_GRP) w->gkinds.res_posts -= std::min<uint64_t>(w->gkinds.res_posts, un.schedules);  // (not posted after all)
        un.take_back(w);
        RidingUpdates upd;
        if (un.upd.any()) {  // (a copy in the pinned ring: the box's slot belongs to the posts of the launch that follows)
            const size_t bytes = 4 * (size_t)w->d.R_local * sizeof(double);
            void *hp = nullptr, *dp = nullptr;
            HIP_TRY(w->stage.acquire(bytes, &hp, &upd.slot));
            memcpy(hp, un.upd.host, bytes);
            HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
            upd.dev = (const double *)dp;
            upd.host = (const double *)hp;
            upd.max_speed = un.upd.max_speed;
            upd.delta_t = un.upd.delta_t;
        }
        // (where it runs launch by launch the ring slot is released behind the FIRST launch, the only one that reads the records)
        rc = run_schedule(w, un.plan, upd);
    }
    if (nested) w->last_sweep_launches = count_before;
    if (lg.taken_in_launch == 0) lg.useless++;
    else lg.useless = 0;
    return rc;
}
// Ends the lingering launch: the postman turns the go word odd behind everything posted, every workgroup writes back as at the
// end of any launch.  What follows in the stream finds the world as after a plain launch.
static int linger_close(mgx_world *w) {
    ResidentLaunches::Linger &lg = w->res.linger;
    if (!lg.open) return MGX_OK;
    const int rc = confirm_held(w);  // (the launch's census: an aborted launch does not linger)
    if (rc != MGX_OK || !lg.open) return rc;
    StageTimer clock("linger");
    if (lg.un.active) {
        // The post before is in the launch's hands first.  The postman reads `posted`, then `close_req` (mgx_sweep.h): a close asked
        // for within the same call as the post — what is recorded goes out, then a schedule that cannot be posted ends the
        // launch — could be seen with the post still unseen, and the launch would end in front of it (taken back and run as a
        // launch: right, but a launch for nothing).  The launch ends behind the post either way: nothing is waited for twice.
        const unsigned long long n = lg.un.number;
        const int r0 = linger_wait(w, [&] { return __atomic_load_n(&lg.box()->taken, __ATOMIC_ACQUIRE) >= n; }, "the last post to be taken");
        if (r0 < 0) return r0;
        if (r0 == 1) return linger_settle(w);  // (the launch ended meanwhile: its workgroups had waited out their bound)
    }
    __atomic_store_n(&lg.box()->close_req, lg.seq0, __ATOMIC_RELEASE);
    const int r = linger_wait(w, [] { return false; }, "the launch to end");
    if (r < 0) return r;
    clock.lap("closed");
    return linger_settle(w);
}
// On the way to post `plan` into the open launch: 1 = the slot of the next number may be written and posted; 0 = no launch
// lingers any more (it had ended, or the plan does not qualify and it was ended): the caller launches.
// (the plan's own conditions: linger_plan_fits, mgx_resident.h)  What the WORLD has to be like for a post: nothing that a commit
// would have to bring to the device first, nothing thawing, resident launches on and not backing off.
static bool linger_world_qualifies(const mgx_world *w) {
    const ResidentLaunches &rl = w->res;
    return !w->dirty && !w->conns_dirty && !w->flags_dirty && !w->thaw_kinds && !w->ir_thaw_active && w->n_keyless == 0 &&
           rl.mode == ResidentLaunches::ON && (w->p.enable_mask & 2u) && rl.backoff.left == 0;
}
// needs_upd: the post carries prior updates — a launch of a form without them (SWEEP_F_UPD) is ended like one the plan does not
// fit, and the schedule becomes a launch of the covering form; from then on the world's launches keep it (upd_seen).
static int linger_prepare_post(mgx_world *w, const std::vector<Launch> &plan, bool needs_upd) {
    ResidentLaunches &rl = w->res;
    ResidentLaunches::Linger &lg = rl.linger;
    if (!lg.open) return 0;
    // a wait inside the launch gave up: nothing more is posted into it (the host-mapped word: no runtime call; linger_post
    // follows a successful return of this function and nothing else, so the check here is the check of both)
    if (const int rce = check_device_error(w)) return rce;
    {   // the launch's own census first (one launch of run-ahead, as ever)
        const uint32_t count_before = w->last_sweep_launches;  // (a declined launch is run again here: not the coming schedule's launches)
        const int rc = confirm_held(w);
        w->last_sweep_launches = count_before;
        if (rc != MGX_OK) return rc;
        if (!lg.open) return 0;
    }
    // (... and a launch whose form reads the world's kinds takes no plan of a world that needs its groups', or the other way
    // round: whoever masks a world or moves the switch has ended the launch already — MGX_ENTER — so this only says it again)
    const bool covered = (!needs_upd || (lg.ran.features & SWEEP_F_UPD) != 0u) && ((lg.ran.features & SWEEP_F_GRP) != 0u) == masked_resident(w);
    if (needs_upd) rl.upd_seen = true;
    const bool fits = covered && linger_plan_fits(plan) && linger_world_qualifies(w);
    if (!fits) {
        const int rc = linger_close(w);
        return rc != MGX_OK ? rc : 0;
    }
    int r = 0;
    if (lg.un.active) {  // the post before: taken?
        const unsigned long long n = lg.un.number;
        r = linger_wait(w, [&] { return __atomic_load_n(&lg.box()->taken, __ATOMIC_ACQUIRE) >= n; }, "the last post to be taken");
        if (r == 0) linger_confirm(w);
    }
    // (the box's slot of the coming number held the post two before it, which the postman has copied to the device: `taken`)
    if (r < 0) return r;
    if (r == 1) {  // the launch ended meanwhile (its workgroups waited out their bound)
        lg.ended_by_device++;
        const int rc = linger_settle(w, true);
        return rc != MGX_OK ? rc : 0;
    }
    return 1;
}
// Posts `plan` (prepared: linger_prepare_post returned 1) with `upd` riding in it: the records go into the coming number's slot
// of the box, unless the caller has written them there already (mgx_tick).
static void linger_post(mgx_world *w, const std::vector<Launch> &plan, const RidingUpdates &upd) {
    ResidentLaunches &rl = w->res;
    ResidentLaunches::Linger &lg = rl.linger;
    const unsigned long long P = ++rl.launch_seq;
    LingerPlan &lp = lg.box()->plan[P & 1ull];
    lp.n = (uint32_t)plan.size();
    lp.has_upd = upd.any() ? 1u : 0u;
    uint8_t ext[MAX_SEGS], n_int[MAX_SEGS];  // (filled here and copied: the box is host-mapped memory, written in words, not byte by byte)
    fill_segments(plan, 0, ext, n_int);
    memcpy(lp.ext, ext, sizeof ext);
    memcpy(lp.n_int, n_int, sizeof n_int);
    lp.upd_max_speed = upd.max_speed;
    lp.upd_delta_t = upd.delta_t;
    lp.number = P;
    Submitted &un = lg.un;
    un.active = true;
    un.number = P;
    un.plan = plan;
    un.before = standing(w);
    un.schedules = std::max(lg.coming, 1u);
    lg.plans_posted++;
    lg.schedules_in_plans += un.schedules;
    lg.largest_plan = std::max<uint64_t>(lg.largest_plan, un.schedules);
    if (lg.ran.features & SWEEP_F_GRP) w->gkinds.res_posts += un.schedules;
    un.upd = RidingUpdates{};
    if (upd.any()) {
        double *slot = linger_upd_slot(w, P);
        if (upd.host != slot) memcpy(slot, upd.host, 4 * (size_t)w->d.R_local * sizeof(double));
        un.upd.host = slot;
        un.upd.max_speed = upd.max_speed;
        un.upd.delta_t = upd.delta_t;
    }
    __atomic_store_n(&lg.box()->posted, P, __ATOMIC_RELEASE);
    stand_at(w, un.before.after_post((int)plan.size()));
    w->stale_kinds |= ~w->p.enable_mask & 15u;  // disabled factors miss what these sweeps deliver
    w->last_sweep_launches++;  // (one submission: the schedule runs inside the launch that is there)
    w->last_sweep = lg.ran;
    w->last_sweep_form = MGX_SWEEP_FORM_POSTED;
}

static uint32_t groups_in_use(const mgx_world *w);
// The robots' groups by device index, as they are now: uploaded again only when the layout has changed them.
static int ensure_group_of(mgx_world *w) {
    mgx_world::GroupSchedules &gs = w->gsched;
    const size_t RL = (size_t)w->d.R_local;
    std::vector<uint32_t> now(RL);
    for (size_t dr = 0; dr < RL; dr++) now[dr] = w->sets.group[(size_t)w->robot_of[dr]];
    if (now != gs.group_of || !gs.group_of_d.p) {
        gs.group_of.swap(now);
        HIP_TRY(gs.group_of_d.upload(gs.group_of, w->stream, (size_t)std::max(w->R_cap, 0)));
        HIP_TRY(hipStreamSynchronize(w->stream));  // (pageable memory: the copy has left it)
    }
    return MGX_OK;
}
// The groups' {inv_s2_obs, inv_s2_ir, inv_s2_trk} by group id, `top` groups of them (mgx_set_group_sigmas; DevWorld::group_sigma):
// each 1.0 / (s * s) as commit forms the world's, so a group's value is the very double a world created with its sigmas holds.
// Under the rule of the kinds' table beside it: fixed once a group has robots, so it goes up again only when a group joined or
// was given values — and the callers come here with no launch lingering.  No group with sigmas of its own: no table at all.
static int ensure_group_sigmas(mgx_world *w, size_t top) {
    mgx_world::GroupKinds &gk = w->gkinds;
    if (gk.n_sigma == 0) return MGX_OK;
    std::vector<double> now(top * (size_t)GROUP_SIGMA_W);
    for (size_t g = 0; g < top; g++) {
        const mgx_group_sigmas s = w->sigmas_of_group((uint32_t)g);
        now[g * GROUP_SIGMA_W + 0] = 1.0 / (s.obstacle * s.obstacle);
        now[g * GROUP_SIGMA_W + 1] = 1.0 / (s.interrobot * s.interrobot);
        now[g * GROUP_SIGMA_W + 2] = 1.0 / (s.tracking * s.tracking);
    }
    if (now != gk.sig_table || !gk.sig_d.p) {
        if (now.size() > gk.sig_d.cap) HIP_TRY(hipStreamSynchronize(w->stream));  // (an array that has to grow is freed first: nothing may still read it)
        gk.sig_table.swap(now);
        HIP_TRY(gk.sig_d.upload(gk.sig_table, w->stream, (size_t)MGX_GROUPS_MAX * (size_t)GROUP_SIGMA_W));
        HIP_TRY(hipStreamSynchronize(w->stream));  // (pageable memory: the copy has left it)
    }
    return MGX_OK;
}
// (what a launch of a world whose groups differ carries in DevWorld::group_sigma: the table, or null where no group has sigmas)
static const double *group_sigma_table(const mgx_world *w) { return w->gkinds.n_sigma ? w->gkinds.sig_d.p : nullptr; }
// What a masked world's resident launch reads (SWEEP_F_GRP): the robots' groups and the groups' kinds by group id, under the
// rule of run_group_plan — the kinds are fixed once a group has robots, so the table goes up again only when a group joined or was
// given its kinds (a table that a mixed call left longer than the groups in use serves as it is).  Never while a launch lingers:
// run_resident comes here behind its commit, which has ended one.
static int ensure_group_kinds(mgx_world *w) {
    const int rc = ensure_group_of(w);
    if (rc != MGX_OK) return rc;
    mgx_world::GroupKinds &gk = w->gkinds;
    if (w->res.linger.open) return fail(MGX_ERR_STATE, "internal: the groups' kinds written while a launch lingers");
    const size_t top = std::max((size_t)groups_in_use(w), gk.table.size());
    std::vector<uint32_t> kinds(top);
    for (size_t g = 0; g < top; g++) kinds[g] = w->kinds_of_group((uint32_t)g);
    if (kinds != gk.table || !gk.table_d.p) {
        if (top > gk.table_d.cap) HIP_TRY(hipStreamSynchronize(w->stream));  // (an array that has to grow is freed first: nothing may still read it)
        gk.table.swap(kinds);
        HIP_TRY(gk.table_d.upload(gk.table, w->stream, (size_t)MGX_GROUPS_MAX));
        HIP_TRY(hipStreamSynchronize(w->stream));  // (pageable memory: the copy has left it)
    }
    for (const uint32_t g : w->gsched.group_of)
        if ((size_t)g >= gk.table.size()) return fail(MGX_ERR_STATE, "internal: robot group %u beyond the kinds table", g);
    return ensure_group_sigmas(w, gk.table.size());  // (the groups' sigmas, as many rows)
}

// ---- run_resident, step by step -------------------------------------------------------------------------------------------
// A launch lingers: the schedule is posted into it if it qualifies — 1; 0: no launch lingers (any more), the caller launches.
// (mgx_tick comes to run_resident prepared, its records in the box already, and posts itself — unless the launch it found had
// ended and the post taken back became THIS lingering launch: then the tick's prior updates sit in the pinned ring.  Records in
// device memory, mgx_mission_tick_end's, cannot ride in a post: the launch ends first.)
static int post_into_open_launch(mgx_world *w, const std::vector<Launch> &plan) {
    if (!w->res.linger.open) return 0;
    if (!w->res.riding.postable()) {
        const int rc = linger_close(w);
        return rc != MGX_OK ? rc : 0;
    }
    const int r = linger_prepare_post(w, plan, w->res.riding.any());
    if (r == 1) linger_post(w, plan, w->res.riding);
    return r;
}
// One part (at most MAX_SEGS segments from `i0`) of the schedule as the launch reads it.  census: residency census + clean abort;
// the ranks of a sharded world abort together, on the word they agree on (without one — mgx_halo_resident_connect_peers without a
// coordinator — they keep the plain bound on every wait).  lingers: the launch stays for the schedules that follow (mgx_dev.h).
static int part_plan(mgx_world *w, const std::vector<Launch> &plan, size_t i0, bool sharded, bool census, bool ranks_agree, bool lingers, SegPlan &sp) {
    ResidentLaunches &rl = w->res;
    sp = SegPlan{};
    sp.n = fill_segments(plan, i0, sp.ext, sp.n_int);
    sp.flag_base = rl.flag_base;
    sp.timeout_ticks = ResidentKnobs::timeout_ticks();
    if (census) {
        sp.launch_seq = ++rl.launch_seq;
        sp.census_ticks = sharded ? ResidentKnobs::census_ticks_sharded() : ResidentKnobs::census_ticks();
        if (ranks_agree) sp.agree_seq = ++w->xres.agree_seq;
    }
    if (lingers) {
        const int rc = ensure_linger_box(w);
        if (rc != MGX_OK) return rc;
        void *bd = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&bd, rl.linger.box(), 0));
        sp.linger_ticks = linger_ticks(w);
        sp.linger_box = (const LingerBox *)bd;
        sp.linger_upd = reinterpret_cast<const double *>(reinterpret_cast<const char *>(bd) + sizeof(LingerBox));
        sp.linger_upd_stride = (unsigned long long)rl.linger.upd_stride;
        sp.linger_dev = rl.linger.dev.p;
        sp.linger_dev_stride = (unsigned long long)rl.linger.dev_stride;
        sp.linger_go = rl.linger.go.p;
    }
    return MGX_OK;
}
// What a launched part leaves on the host: the counts, the open launch if it lingers, what confirm_resident needs to take it
// back and run it again launch by launch, and where the world stands behind it.
static void part_launched(mgx_world *w, const std::vector<Launch> &plan, size_t i0, const SegPlan &sp, const RidingUpdates &rode, bool can, bool sharded,
                          const SweepRan &ran) {
    ResidentLaunches &rl = w->res;
    w->last_sweep_launches++;
    rl.launches++;
    if (can && (ran.features & SWEEP_F_GRP)) w->gkinds.res_launches++;
    if (can) {  // (a rank that voted no launched no sweep)
        w->last_sweep = ran;
        w->last_sweep_form = sharded ? MGX_SWEEP_FORM_SHARDED : MGX_SWEEP_FORM_RESIDENT;
    }
    if (sp.linger_ticks > 0) {
        ResidentLaunches::Linger &lg = rl.linger;
        lg.open = true;
        lg.seq0 = sp.launch_seq;
        lg.ran = ran;
        lg.taken_in_launch = 0;
        lg.un.active = false;
        lg.launches++;
    }
    if (sp.launch_seq) {  // (a launch with a census)
        Submitted &pd = rl.pending;
        pd.active = true;
        pd.number = sp.launch_seq;
        pd.partial = i0 > 0;
        pd.plan.assign(plan.begin() + (long)i0, plan.begin() + (long)i0 + sp.n);
        pd.before = standing(w);
        pd.upd = rode;
    } else {
        log_plan(w, plan, i0, (size_t)sp.n);
    }
    stand_at(w, standing(w).after_launch(sp.n));
}
// Runs the schedule as resident launches if this world qualifies: 1 = done, 0 = not eligible (the caller takes the
// launch-per-segment path), negative = error.  Eligible: inter-robot factors enabled and staged in LDS, every robot
// local (no ghosts: their records arrive between launches) or the ranks wired for it, nothing thawing, and every workgroup
// co-resident.  The world's riding prior updates (run_schedule) travel in the first launch only.
static int run_resident(mgx_world *w, const std::vector<Launch> &plan) {
    ResidentLaunches &rl = w->res;
    int rc = post_into_open_launch(w, plan);
    if (rc != 0) return rc;
    if (!resident_enabled() || rl.mode == ResidentLaunches::OFF || plan.size() < 2) return 0;
    if ((rc = commit(w)) != MGX_OK) return rc;
    if (!resident_gate(w, plan)) return 0;
    StageTimer tr("resident");
    const DevWorld &d = w->d;
    const bool sharded = w->xres.connected;
    // What follows is this rank's own: where the ranks agree on every schedule (xres.agree) a rank
    // that cannot take part says so THERE — its launch is a single vote, and everybody takes the launch-by-launch path.
    const bool ranks_agree = sharded && w->xres.agree != nullptr;
    if (rl.riding.any()) rl.upd_seen = true;
    const uint32_t form = resident_features(w, rl.riding.any());
    const ResidentFit fit = resident_fits(w, sharded, form);
    if (fit != FITS && !ranks_agree) {
        if (fit == UNFIT_NOW || !sharded) return 0;
        if (fit == UNFIT_LDS) return fail(MGX_ERR_STATE, "resident launches were agreed on with the other ranks, but this rank's robots no longer fit LDS");
        if (d.R_local > rl.capacity_for(d, true, form))  // (no census without the ranks' agreement, so no decider workgroup either)
            return fail(MGX_ERR_STATE, "resident launches were agreed on with the other ranks, but only %d of this rank's %d workgroups "
                                       "are resident at once", rl.capacity_for(d, true, form), d.R_local);
    }
    const bool can = fit == FITS || !ranks_agree;
    tr.lap("gate + capacity");
    if ((rc = ensure_resident_tables(w)) != MGX_OK) return rc;
    tr.lap("peer tables");
    const bool by_groups = (form & SWEEP_F_GRP) != 0u;  // the masked form: the robots' groups and the groups' kinds, in front of the launch
    if (by_groups && (rc = ensure_group_kinds(w)) != MGX_OK) return rc;
    w->stale_kinds |= ~w->p.enable_mask & 15u;  // disabled factors miss what these sweeps deliver
    const bool census = sharded ? ranks_agree : ResidentKnobs::census();
    for (size_t i0 = 0; i0 < plan.size(); i0 += MAX_SEGS) {
        if (census && i0 > 0) {
            if ((rc = confirm_resident(w)) != MGX_OK) return rc;  // the previous part of this schedule
            if (rl.backoff.left > 0) {  // ... was sent back: the rest follows it launch by launch
                rc = run_segments(w, plan, i0, RidingUpdates{});
                return rc != MGX_OK ? rc : 1;
            }
        }
        // Lingering: the launch that runs the END of the schedule stays for the schedules that follow — when the caller's pattern
        // promises some (schedules back to back, or no evidence yet that they are not: two lingering launches in a row that ended
        // without a post switch it off until schedules come back to back again)
        const bool lingers = census && can && !sharded && i0 + (size_t)MAX_SEGS >= plan.size() && linger_ticks(w) > 0 &&
                             (rl.linger.useless < 2 || rl.linger.streak >= 2);
        SegPlan sp;
        if ((rc = part_plan(w, plan, i0, sharded, census, ranks_agree, lingers, sp)) != MGX_OK) return rc;
        if (sharded && sp.ext[0]) {  // segment 0 reads the ghosts' plain copies: one direct exchange in front of the launch
            rc = direct_exchange(w);
            if (rc != MGX_OK) return rc;
        }
        const RidingUpdates rode = i0 == 0 ? rl.riding : RidingUpdates{};
        w->d.upd = rode.dev; w->d.upd_max_speed = rode.max_speed; w->d.upd_delta_t = rode.delta_t;
        if (by_groups) {  // (group_seg stays null)
            w->d.group_of = w->gsched.group_of_d.p; w->d.group_enable = w->gkinds.table_d.p; w->d.group_sigma = group_sigma_table(w);
        }
        SweepRan ran;
        const bool cooperative = ResidentKnobs::cooperative();
        if (can && !resident_launch_allowed(w)) return fail(MGX_ERR_STATE, "internal: a resident launch while factors thaw");
        const hipError_t le = can ? launch_robot_schedule(w->d, w->d.R_local, sp, sharded, form, cooperative, w->stream, &ran)
                                  : launch_agree_abort(w->d, sp, w->stream);
        w->d.upd = nullptr;
        w->d.group_of = nullptr;
        w->d.group_enable = nullptr;
        w->d.group_sigma = nullptr;
        if (le != hipSuccess) {
            (void)hipGetLastError();
            if (cooperative && le == hipErrorCooperativeLaunchTooLarge && i0 == 0 && !sharded) {
                for (int &c : rl.cap[0]) c = 0;  // until the topology (hence the workgroup's LDS) changes
                return 0;
            }
            return fail(MGX_ERR_HIP, "resident schedule launch: %s", hipGetErrorString(le));
        }
        part_launched(w, plan, i0, sp, rode, can, sharded, ran);
    }
    return 1;
}

// ---- one schedule per robot group (include/mgx.h, ROBOT GROUPS: mgx_iterate_groups, mgx_mission_tick_end_groups) ------------------
// What the per-group schedule calls check before anything happens: the arrays alone first (no device needed, no world either), the
// world last, then its live robots' groups.
static int group_schedule_arguments(mgx_world *w, uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first) {
    if (!step_first) return fail(MGX_ERR_INVALID, "null argument (step_first)");
    if (n_groups == 0 || n_groups > MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "n_groups %u is not in 1 .. MGX_GROUPS_MAX (%u)", n_groups, MGX_GROUPS_MAX);
    const long long bad = group_steps_check(n_groups, steps, step_first);
    if (bad == -1) return fail(MGX_ERR_INVALID, "step_first does not ascend from 0");
    if (bad == -2) return fail(MGX_ERR_INVALID, "null argument (steps)");
    if (bad > 0) return fail(MGX_ERR_INVALID, "bad step %lld", bad - 1);
    if (!w) return fail(MGX_ERR_INVALID, "null argument");
    for (size_t r = 0; r < w->robots.size(); r++)
        if (!w->robots[r].removed && !w->robots[r].ghost && w->sets.group[r] >= n_groups)
            return fail(MGX_ERR_INVALID, "robot %zu is in group %u: not below n_groups %u", r, w->sets.group[r], n_groups);
    return MGX_OK;
}
// Equal schedules — every group that holds live robots has byte-equal steps — ARE the plain call with those steps (*eq_steps,
// *eq_n): true.  Otherwise the call is MIXED, and a world that cannot run one is refused here, before anything changes (*rc).
static bool group_schedule_is_plain(mgx_world *w, uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first, const uint8_t **eq_steps,
                                    uint32_t *eq_n, int *rc) {
    std::vector<uint8_t> live((size_t)n_groups, 0);
    for (size_t r = 0; r < w->robots.size(); r++)
        if (!w->robots[r].removed && !w->robots[r].ghost) live[w->sets.group[r]] = 1;
    uint32_t first = n_groups;
    *rc = MGX_OK;
    const bool sharded = std::find(w->sets.ghost.begin(), w->sets.ghost.end(), (uint8_t)1) != w->sets.ghost.end() || w->xres.connected ||
                         w->direct.connected || w->rccl.connected;
    if (sharded) {  // (every robot is in group 0 there: only a call whose groups ALL have the same steps says what the world runs)
        const std::vector<uint8_t> all((size_t)n_groups, 1);
        if (!group_steps_equal(n_groups, steps, step_first, all.data(), &first)) {
            *rc = fail(MGX_ERR_STATE, "groups with different schedules on a sharded world: ghosts have no group");
            return false;
        }
    }
    if (group_steps_equal(n_groups, steps, step_first, live.data(), &first)) {
        *eq_steps = first < n_groups && steps ? steps + step_first[first] : nullptr;
        *eq_n = first < n_groups ? step_first[first + 1] - step_first[first] : 0u;
        return true;
    }
    if (w->frozen_live || w->ir_frozen_live || w->thaw_kinds || w->ir_thaw_active || w->n_keyless > 0)
        *rc = fail(MGX_ERR_STATE, "groups with different schedules on a world that has switched a factor kind (mgx_set_enabled): the thaw kernels are world-wide");
    return false;
}
// The launches of a MIXED call: launch k carries segment k of every group (GroupPlan, mgx_resident.h), launch by launch in the
// segments form — never recorded, posted or resident.  The caller has ended a lingering launch and submitted what was recorded
// (MGX_ENTER).  The robots' groups by device index go up only when the layout has changed them; the call's segment records travel
// through the pinned ring into device memory, ONE copy for all its launches.
// by_masks: the plan is ONE schedule (or one sweep) for every group, run this way because the world is masked
// (mgx_set_group_enabled) — counted apart (mgx_group_enabled_stats), and none of its workgroups sits out.
static int run_group_plan(mgx_world *w, const GroupPlan &gp, bool by_masks = false) {
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    if ((rc = check_device_error(w)) != MGX_OK) return rc;
    mgx_world::GroupSchedules &gs = w->gsched;
    mgx_world::GroupKinds &gk = w->gkinds;
    if (by_masks) gk.masked_plans++;
    else gs.mixed_calls++;
    const size_t RL = (size_t)w->d.R_local;
    if (gp.n_launches == 0 || RL == 0) return MGX_OK;
    // (a robot that has left keeps its group: every group on the device has a record, all-zero — sits out — beyond n_groups)
    if ((rc = ensure_group_of(w)) != MGX_OK) return rc;
    size_t top = gp.n_groups;
    for (const uint32_t g : gs.group_of) top = std::max(top, (size_t)g + 1);
    std::vector<uint32_t> members(top, 0u);
    for (size_t dr = 0; dr < RL; dr++) members[gs.group_of[dr]]++;
    const size_t n_rec = gp.n_launches * top;
    {
        void *hp = nullptr;
        int slot = 0;
        HIP_TRY(w->stage.acquire(sizeof(GroupSeg) * n_rec, &hp, &slot));
        GroupSeg *rec = (GroupSeg *)hp;
        std::fill(rec, rec + n_rec, GroupSeg{0u, 0u, 0, 0u});
        for (size_t k = 0; k < gp.n_launches; k++) std::copy(gp.launch(k), gp.launch(k) + gp.n_groups, rec + k * top);
        if (n_rec > gs.seg_d.cap) HIP_TRY(hipStreamSynchronize(w->stream));  // (an array that has to grow is freed first: nothing may still read it)
        HIP_TRY(gs.seg_d.reserve(n_rec));
        HIP_TRY(hipMemcpyAsync(gs.seg_d.p, hp, sizeof(GroupSeg) * n_rec, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(w->stage.release(slot, w->stream));
    }
    // A masked world: the groups' enabled kinds by group id, beside the records.  They are fixed once a group has robots, so the
    // table goes up again only when a group joined or was given its kinds (an unmasked world has none: the kernel's scalar serves)
    if (gk.masked()) {
        std::vector<uint32_t> kinds(top);
        for (size_t g = 0; g < top; g++) kinds[g] = w->kinds_of_group((uint32_t)g);
        if (kinds != gk.table || !gk.table_d.p) {
            if (top > gk.table_d.cap) HIP_TRY(hipStreamSynchronize(w->stream));  // (an array that has to grow is freed first: nothing may still read it)
            gk.table.swap(kinds);
            HIP_TRY(gk.table_d.upload(gk.table, w->stream, (size_t)MGX_GROUPS_MAX));
            HIP_TRY(hipStreamSynchronize(w->stream));  // (pageable memory: the copy has left it)
        }
        if ((rc = ensure_group_sigmas(w, top)) != MGX_OK) return rc;  // (... and their sigmas, where some group has its own)
    }
    w->stale_kinds |= ~w->p.enable_mask & 15u;  // disabled factors miss what these sweeps deliver
    for (size_t k = 0; k < gp.n_launches; k++) {
        const bool writes_snap = gp.writes_snap[k] != 0;
        if (gp.any_ext[k]) w->res.backoff.external_iteration();
        w->d.group_of = gs.group_of_d.p;
        w->d.group_seg = gs.seg_d.p + k * top;
        w->d.group_enable = gk.masked() ? gk.table_d.p : nullptr;
        w->d.group_sigma = group_sigma_table(w);
        const hipError_t e = launch_robot_sweep(w->d, 0, w->d.R_local, 0u, 0u, 0, writes_snap ? 1 - w->d.cur : -1, 0u, w->stream, &w->last_sweep);
        w->d.group_of = nullptr;
        w->d.group_seg = nullptr;
        w->d.group_enable = nullptr;
        w->d.group_sigma = nullptr;
        HIP_TRY(e);
        w->last_sweep_form = MGX_SWEEP_FORM_SEGMENTS;
        w->last_sweep_launches++;
        if (by_masks) gk.masked_launches++;
        else gs.mixed_launches++;
        if (writes_snap) w->d.cur ^= 1;
        for (size_t g = 0; g < top; g++) {  // the counters' log, scoped by group; the workgroups that sat the launch out, from the plan
            const GroupSeg none{0u, 0u, 0, 0u};
            const GroupSeg &sg = g < gp.n_groups ? gp.launch(k)[g] : none;
            if (sits_out(sg)) gs.sat_out += by_masks ? 0u : members[g];
            else if (members[g]) log_launch(w, -2 - (int)g, sg.ext_mask, sg.int_mask, sg.n_int);
        }
    }
    return MGX_OK;
}
static uint32_t groups_in_use(const mgx_world *w) {  // 1 + the highest group id a robot of the world has (had)
    uint32_t top = 1;
    for (const uint32_t g : w->sets.group) top = std::max(top, g + 1);
    return top;
}
// A masked world's schedules (mgx_set_group_enabled): the plan every group shares as a group plan in which every group has the
// same segments — the launches of run_segments, each reading its robots' kinds beside the segment record.
static int run_masked_plan(mgx_world *w, const std::vector<Launch> &plan) {
    GroupPlan gp;
    const uint32_t top = groups_in_use(w);
    gp.n_groups = top;
    gp.n_launches = plan.size();
    gp.n_segments.assign(top, (uint32_t)plan.size());
    gp.recs.reserve(plan.size() * (size_t)top);
    for (const Launch &l : plan) {
        gp.recs.insert(gp.recs.end(), (size_t)top, GroupSeg{l.ext, int_phases(l), l.n_int, l.hints});
        gp.writes_snap.push_back(l.n_int > 0 ? 1 : 0);
        gp.any_ext.push_back(l.ext ? 1 : 0);
    }
    return run_group_plan(w, gp, true);
}
// ... and its world-wide fine-grained sweeps (mgx_sweep, mgx_*_iteration with robot = -1): one launch of that form
static int run_masked_launch(mgx_world *w, uint32_t ext_mask, uint32_t int_mask, int n_int, uint32_t hints) {
    GroupPlan gp;
    const uint32_t top = groups_in_use(w);
    gp.n_groups = top;
    gp.n_launches = 1;
    gp.n_segments.assign(top, 1u);
    gp.recs.assign((size_t)top, GroupSeg{ext_mask, int_mask, n_int, hints});
    gp.writes_snap.assign(1, (int_mask & PH_INT_VARIABLE) && n_int > 0 ? 1 : 0);
    gp.any_ext.assign(1, ext_mask ? 1 : 0);
    return run_group_plan(w, gp, true);
}
