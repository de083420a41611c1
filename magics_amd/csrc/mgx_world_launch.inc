// mgx_world_launch.inc — launches: confirm_resident, sweep, resident schedule launches, lingering launches (the host's side).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// ---- launches -----------------------------------------------------------------------------------------
static int direct_exchange(mgx_world *w);
static int rccl_exchange(mgx_world *w);
static int sweep(mgx_world *w, int32_t robot, uint32_t ext_mask, uint32_t int_mask, int n_int, uint32_t hints = 0);
static void log_launch(mgx_world *w, int robot, uint32_t ext_mask, uint32_t int_mask, int n_int);

// A resident schedule launch decides for itself, before it writes anything, whether all its workgroups are on the device
// together (SegPlan: residency census) — and if another tenant of the GPU holds the CUs its tail needs, it returns at once
// and leaves the world untouched.  The host must not put anything behind a launch whose decision it has not seen (what
// follows would run on the wrong state), so every entry point that enqueues work or reads state comes through here first:
// the decision falls within microseconds of the launch's START, so in a stream of ticks the host simply stays ONE launch
// ahead of the device instead of many.  An aborted launch is run again on the launch-per-segment path, and the next few
// schedules skip the resident form (doubling back-off while the GPU stays shared).
static int confirm_resident(mgx_world *w, bool rerun, int32_t *outcome) {
    mgx_world::PendingResident &pd = w->pending;
    if (outcome) *outcome = MGX_RESIDENT_NONE;
    if (!pd.active) return MGX_OK;
    StageTimer clock("confirm");
    const double t0 = StageTimer::now();
    unsigned long long v = 0;
    for (unsigned spins = 0;; spins++) {
        v = __atomic_load_n(w->decision_host, __ATOMIC_ACQUIRE);
        if ((v >> 2) >= pd.seq) break;
        if ((spins & 0xfffffu) == 0xfffffu && StageTimer::now() - t0 > 30e6) {
            // 30 s: the launch never started (a stuck stream): nothing sensible is left to do.  (No runtime call in this loop:
            // a stream query per look made the runtime put markers between the launches.)
            pd.active = false;
            return fail(MGX_ERR_STATE, "resident launch %llu was never decided (the stream does not advance)", pd.seq);
        }
    }
    pd.active = false;
    clock.lap((v & 3ull) == RESIDENT_ABORT ? "launch ABORTED" : "launch decided: go");
    if ((v >> 2) == pd.seq && (v & 3ull) == RESIDENT_ABORT) {
        // nothing happened on the device: take the host's bookkeeping back and run the same schedule launch by launch
        w->resident_aborts++;
        if (w->linger.open && w->linger.seq0 == pd.seq) w->linger.open = false;  // (its decider left with the verdict: nobody lingers)
        w->resident_backoff_len = std::min(std::max(2 * w->resident_backoff_len, 64), 32768);
        w->resident_backoff = w->resident_backoff_len + (int)pd.segs.size();  // (+ this schedule's own re-run)
        w->d.cur = pd.cur_before;
        w->flag_base = pd.flag_base_before;
        w->last_sweep_launches = 0;
        if (!rerun && !pd.upd && !pd.partial) {  // mgx_resident_outcome: the caller issues the schedule again
            if (outcome) *outcome = MGX_RESIDENT_DECLINED;
            return MGX_OK;
        }
        if (outcome) *outcome = MGX_RESIDENT_RAN;  // (by the time the caller looks, it has: launch by launch)
        bool first = true;
        for (size_t k = 0; k < pd.segs.size(); k++) {
            if (first && pd.upd) { w->d.upd = pd.upd; w->d.upd_max_speed = pd.upd_max_speed; w->d.upd_delta_t = pd.upd_delta_t; }
            const int rc = sweep(w, -1, pd.segs[k].first, pd.segs[k].second ? (PH_INT_FACTOR | PH_INT_VARIABLE) : 0, pd.segs[k].second, pd.hints[k]);
            w->d.upd = nullptr;
            if (first && pd.upd && pd.upd_slot >= 0) {
                // the slot was released behind the declined launch, which returned at once: without this the ring would hand it
                // out again (or free it) while the kernel just enqueued has yet to read the prior updates
                const hipError_t e = w->stage.release(pd.upd_slot, w->stream);
                if (rc == MGX_OK && e != hipSuccess) return fail(MGX_ERR_HIP, "event record: %s", hipGetErrorString(e));
            }
            first = false;
            if (rc != MGX_OK) return rc;
        }
        return MGX_OK;
    }
    w->resident_backoff_len = 0;
    if (outcome) *outcome = MGX_RESIDENT_RAN;
    for (const auto &sg : pd.segs) log_launch(w, -1, sg.first, sg.second ? (PH_INT_FACTOR | PH_INT_VARIABLE) : 0, sg.second);
    return MGX_OK;
}
static int sweep(mgx_world *w, int32_t robot, uint32_t ext_mask, uint32_t int_mask, int n_int, uint32_t hints) {
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
        if (ext_mask && w->resident_backoff > 0) w->resident_backoff--;
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
        HIP_TRY(launch_robot_sweep(w->d, w->dev_of[(size_t)robot], 1, 0, int_mask, n_int, writes_snap ? w->d.cur : -1, 0, w->stream,
                                   &w->last_sweep));
        w->last_sweep_form = MGX_SWEEP_FORM_SEGMENTS;
        if (w->thaw_kinds && (thawing || writes_snap)) HIP_TRY(launch_thaw_done(w->d, w->dev_of[(size_t)robot], 1, writes_snap ? 1 : 0, w->stream));
        log_launch(w, robot, 0, int_mask, n_int);
    }
    return MGX_OK;
}

// ---- resident schedule launches: a whole mgx_iterate / mgx_tick schedule in ONE launch -----------------------

static bool resident_enabled() {  // MGX_PERSISTENT=0 keeps every schedule on the launch-per-segment path
    static int v = -1;
    if (v < 0) { const char *e = getenv("MGX_PERSISTENT"); v = (e && e[0] == '0') ? 0 : 1; }
    return v == 1;
}
// a wait inside a resident launch gave up (a neighbour's workgroup never published): the beliefs are not to be trusted
// the robots each local robot exchanges snapshot records with: owners of its incoming connections and targets of
// its outgoing ones (the latter matter when the reference's bookkeeping has left a connection one-sided)
static int ensure_resident_tables(mgx_world *w) {
    hipStream_t s = w->stream;
    const size_t R = (size_t)w->d.R_local;
    if (!w->sweep_abort_buf.p) {
        std::vector<unsigned long long> z(1, 0ull);
        HIP_TRY(w->sweep_abort_buf.upload(z, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (w->sweep_flag_buf.n != R) {
        HIP_TRY(w->sweep_flag_buf.reserve(R));
        HIP_TRY(hipMemsetAsync(w->sweep_flag_buf.p, 0, sizeof(unsigned long long) * R, s));
        w->flag_base = 0;
        // ... and with the segment count the exchange records start over: zeroed, so that no sequence word of an earlier life
        // of the device arrays validates (a valid word has its top bit set, mgx_dev.h)
        const size_t xb = R * (size_t)w->K * (size_t)XREC_BYTES;
        HIP_TRY(w->xrec_buf.reserve(2 * xb));
        HIP_TRY(hipMemsetAsync(w->xrec_buf.p, 0, 2 * xb, s));
    }
    {
        const size_t xb = R * (size_t)w->K * (size_t)XREC_BYTES;
        w->d.xrec[0] = w->xrec_buf.p;
        w->d.xrec[1] = w->xrec_buf.p ? w->xrec_buf.p + xb : nullptr;
    }
    if (w->census_buf.n < R + 1) {  // residency census: one word per workgroup of a launch (never reset: monotonic in the launch number)
        std::vector<unsigned long long> z(R + 1 + R / 4 + 64, 0ull);
        HIP_TRY(w->census_buf.upload(z, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (!w->decision_buf.p) {  // the decision word and its host-mapped copy
        std::vector<unsigned long long> z1(1, 0ull);
        HIP_TRY(w->decision_buf.upload(z1, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipHostMalloc((void **)&w->decision_host, sizeof(unsigned long long), hipHostMallocMapped));
        *w->decision_host = 0ull;
    }
    {
        void *dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, w->decision_host, 0));
        w->d.census = w->census_buf.p;
        w->d.decision = w->decision_buf.p;
        w->d.decision_host = (unsigned long long *)dp;
    }
    if (!w->peers_valid) {
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
        std::vector<int32_t> &fill = w->peer_fill;
        fill.assign(ptr, ptr + R);
        for (size_t ci = 0; ci < n_conns; ci++) {
            const int o = dev_of[(size_t)conns[ci].owner], t = dev_of[(size_t)conns[ci].other];
            if ((size_t)o < R) idx[(size_t)fill[(size_t)o]++] = t;
            if ((size_t)t < R) idx[(size_t)fill[(size_t)t]++] = o;
        }
        if (ptr[R] == 0) idx[0] = 0;
        HIP_TRY(w->peer_ptr_dev.reserve(words));
        HIP_TRY(hipMemcpyAsync(w->peer_ptr_dev.p, hp, sizeof(int32_t) * (R + 1 + (size_t)std::max(ptr[R], 1)), hipMemcpyHostToDevice, s));
        HIP_TRY(w->stage.release(slot, s));
        w->peer_idx_off = R + 1;
        w->peers_valid = true;
    }
    w->d.sweep_flag = w->sweep_flag_buf.p;
    w->d.sweep_abort = w->sweep_abort_buf.p;
    w->d.peer_ptr = w->peer_ptr_dev.p;
    w->d.peer_idx = w->peer_ptr_dev.p + w->peer_idx_off;
    return MGX_OK;
}
// Runs the schedule as resident launches if this world qualifies: 1 = done, 0 = not eligible (the caller takes the
// launch-per-segment path), negative = error.  Eligible: inter-robot factors enabled and staged in LDS, every robot
// local (no ghosts: their records arrive between launches), nothing thawing, and every workgroup co-resident.
// the conditions every rank of a sharded world decides alike on: same schedule, same world-wide switches, the same back-off
// (aborts are the ranks' common answer)
static bool resident_gate(const mgx_world *w, const std::vector<Launch> &plan) {
    if (!resident_enabled() || w->resident_off || plan.size() < 2) return false;
    if (w->resident_backoff > 0) return false;  // a recent launch found the GPU shared (residency census): launch by launch for a while
    const DevWorld &d = w->d;
    const bool sharded = w->xres.connected;  // the ranks have agreed (mgx_halo_resident_connect_peers) that ghost records travel inside the launches
    if ((d.R_total != d.R_local && !sharded) || !(w->p.enable_mask & 2u)) return false;
    if (((w->direct.connected || w->rccl.connected) && !sharded)) return false;
    for (const Launch &l : plan)
        if (l.n_int > 255) return false;
    if (sharded && plan[0].ext && !w->direct.connected) return false;  // the exchange in front of the launch is the direct one
    return true;
}

// ---- lingering resident launches: the host's side (mgx_dev.h; the device's side is in mgx_sweep.h) --------------------------
static int run_resident(mgx_world *w, const std::vector<Launch> &plan);
static long long linger_ticks(mgx_world *w) {
    mgx_world::Linger &lg = w->linger;
    if (lg.ticks < 0) {
        const char *off = getenv("MGX_LINGER"), *us = getenv("MGX_LINGER_US");
        long long v = us ? atoll(us) : 300;  // microseconds a workgroup waits for the next schedule before it ends the launch
        if (off && off[0] == '0') v = 0;
        lg.ticks = (v > 0 ? std::min<long long>(v, 1000000) : 0) * 100ll;  // 100 MHz wall clock
    }
    return lg.ticks;
}
static double *linger_upd_slot(mgx_world *w, unsigned long long number) {
    mgx_world::Linger &lg = w->linger;
    return reinterpret_cast<double *>(reinterpret_cast<char *>(lg.box) + sizeof(LingerBox)) + (size_t)(number & 1ull) * lg.upd_stride;
}
// the box (host-mapped: header, two plan slots, two blocks of prior-update records) and the go word; never while a launch lingers
static int ensure_linger_box(mgx_world *w) {
    mgx_world::Linger &lg = w->linger;
    const size_t stride = ((size_t)4 * (size_t)std::max(w->d.R_local, 1) + 7) & ~(size_t)7;
    if (!lg.go.p) {
        std::vector<unsigned long long> z(1, 0ull);
        HIP_TRY(lg.go.upload(z, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (lg.box && lg.upd_stride >= stride) return MGX_OK;
    if (lg.box) { (void)hipHostFree(lg.box); lg.box = nullptr; }
    const size_t grown = (stride + stride / 2 + 7) & ~(size_t)7, bytes = sizeof(LingerBox) + 2 * grown * sizeof(double);
    HIP_TRY(hipHostMalloc((void **)&lg.box, bytes, hipHostMallocMapped));
    memset(lg.box, 0, bytes);
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
    mgx_world::Linger &lg = w->linger;
    const double t0 = StageTimer::now();
    for (unsigned spins = 0;; spins++) {
        if (pred()) return 0;
        const unsigned long long c = __atomic_load_n(&lg.box->closed, __ATOMIC_ACQUIRE);
        if ((c & 1ull) && (c >> 1) >= lg.seq0) return 1;
        if ((spins & 0xfffffu) == 0xfffffu && StageTimer::now() - t0 > 30e6)
            return fail(MGX_ERR_STATE, "lingering launch %llu: no answer from the device while waiting for %s (the stream does not advance)", lg.seq0, what);
    }
}
// a post the launch has taken: it runs (or has run) behind everything before it — its launches enter the counters' log
static void linger_confirm(mgx_world *w) {
    mgx_world::Linger &lg = w->linger;
    for (const Launch &l : lg.un.plan) log_launch(w, -1, l.ext, l.n_int ? (PH_INT_FACTOR | PH_INT_VARIABLE) : 0, l.n_int);
    lg.un.active = false;
    lg.posts++;
    lg.taken_in_launch++;
}
// The launch has ended (closed word c = 2 S + 1: behind plan S).  A post it never took is taken back and run as a launch of its
// own — from the same records, nothing lost and nothing twice.
static int linger_settle(mgx_world *w, bool nested = false) {  // nested: on the way to the NEXT schedule (whose launches are counted apart)
    mgx_world::Linger &lg = w->linger;
    const uint32_t count_before = w->last_sweep_launches;
    const unsigned long long c = __atomic_load_n(&lg.box->closed, __ATOMIC_ACQUIRE);
    lg.open = false;
    int rc = MGX_OK;
    if (lg.un.active) {
        if ((c >> 1) >= lg.un.number) {
            linger_confirm(w);
        } else {
            mgx_world::Linger::Post un = std::move(lg.un);
            lg.un = mgx_world::Linger::Post{};
            lg.reruns++;
            w->d.cur = un.cur_before;
            w->flag_base = un.flag_base_before;
            w->last_sweep_launches = 0;  // (how the schedule that was posted ran after all: what mgx_last_launch_count says of it)
            void *hp = nullptr, *dp = nullptr;
            int slot = -1;
            if (un.has_upd) {  // (a copy in the pinned ring: the box's slot belongs to the posts of the launch that follows)
                const size_t bytes = 4 * (size_t)w->d.R_local * sizeof(double);
                HIP_TRY(w->stage.acquire(bytes, &hp, &slot));
                memcpy(hp, linger_upd_slot(w, un.number), bytes);
                HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
            }
            bool first = true;
            auto with_upd = [&]() { if (first && un.has_upd) { w->d.upd = (const double *)dp; w->d.upd_max_speed = un.max_speed; w->d.upd_delta_t = un.delta_t; w->upd_ring_slot = slot; } };
            with_upd();
            w->upd_host = (const double *)hp;
            const int resident = run_resident(w, un.plan);
            w->upd_host = nullptr;
            w->upd_ring_slot = -1;
            w->d.upd = nullptr;
            if (resident < 0) rc = resident;
            if (resident == 0)
                for (const Launch &l : un.plan) {
                    with_upd();
                    rc = sweep(w, -1, l.ext, l.n_int ? (PH_INT_FACTOR | PH_INT_VARIABLE) : 0, l.n_int, l.hints);
                    w->d.upd = nullptr;
                    first = false;
                    if (rc != MGX_OK) break;
                }
            if (slot >= 0) {
                const hipError_t e = w->stage.release(slot, w->stream);
                if (rc == MGX_OK && e != hipSuccess) rc = fail(MGX_ERR_HIP, "event record: %s", hipGetErrorString(e));
            }
        }
    }
    if (nested) w->last_sweep_launches = count_before;
    if (lg.taken_in_launch == 0) lg.useless++;
    else lg.useless = 0;
    return rc;
}
// Ends the lingering launch: the postman turns the go word odd behind everything posted, every workgroup writes back as at the
// end of any launch.  What follows in the stream finds the world as after a plain launch.
static int linger_close(mgx_world *w) {
    mgx_world::Linger &lg = w->linger;
    if (!lg.open) return MGX_OK;
    if (w->pending.active) {  // (the launch's census: an aborted launch does not linger)
        const bool hold = lg.hold;
        lg.hold = true;
        const int rc = confirm_resident(w);
        lg.hold = hold;
        if (rc != MGX_OK) return rc;
        if (!lg.open) return MGX_OK;
    }
    StageTimer clock("linger");
    __atomic_store_n(&lg.box->close_req, lg.seq0, __ATOMIC_RELEASE);
    const int r = linger_wait(w, [] { return false; }, "the launch to end");
    if (r < 0) return r;
    clock.lap("closed");
    return linger_settle(w);
}
// On the way to post `plan` into the open launch: 1 = the slot of the next number may be written and posted; 0 = no launch
// lingers any more (it had ended, or the plan does not qualify and it was ended): the caller launches.
static bool linger_plan_fits(const std::vector<Launch> &plan) {
    if (plan.empty() || plan.size() > (size_t)MAX_SEGS || plan[0].ext) return false;  // a post CONTINUES the last segment of the plan before
    for (const Launch &l : plan)
        if (l.n_int > 255) return false;
    return true;
}
static int linger_prepare_post(mgx_world *w, const std::vector<Launch> &plan) {
    mgx_world::Linger &lg = w->linger;
    if (!lg.open) return 0;
    if (w->pending.active) {  // the launch's own census first (one launch of run-ahead, as ever)
        const uint32_t count_before = w->last_sweep_launches;  // (a declined launch is run again here: not the coming schedule's launches)
        lg.hold = true;
        const int rc = confirm_resident(w);
        lg.hold = false;
        w->last_sweep_launches = count_before;
        if (rc != MGX_OK) return rc;
        if (!lg.open) return 0;
    }
    const bool fits = linger_plan_fits(plan) && !w->dirty && !w->conns_dirty && !w->flags_dirty && !w->thaw_kinds && !w->ir_thaw_active &&
                      w->n_keyless == 0 && !w->resident_decline && !w->resident_off && (w->p.enable_mask & 2u) && w->resident_backoff == 0;
    if (!fits) {
        const int rc = linger_close(w);
        return rc != MGX_OK ? rc : 0;
    }
    int r = 0;
    if (lg.un.active) {  // the post before: taken?
        const unsigned long long n = lg.un.number;
        r = linger_wait(w, [&] { return __atomic_load_n(&lg.box->taken, __ATOMIC_ACQUIRE) >= n; }, "the last post to be taken");
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
// Posts `plan` (prepared: linger_prepare_post returned 1; the prior-update records, if any, are in the coming number's slot).
static int linger_post(mgx_world *w, const std::vector<Launch> &plan, bool has_upd, double max_speed, double delta_t) {
    mgx_world::Linger &lg = w->linger;
    const unsigned long long P = ++w->launch_seq;
    LingerPlan &lp = lg.box->plan[P & 1ull];
    lp.n = (uint32_t)plan.size();
    lp.has_upd = has_upd ? 1u : 0u;
    uint8_t ext[MAX_SEGS] = {}, n_int[MAX_SEGS] = {};
    for (size_t k = 0; k < plan.size(); k++) { ext[k] = plan[k].ext ? 1 : 0; n_int[k] = (uint8_t)plan[k].n_int; }
    memcpy(lp.ext, ext, sizeof ext);
    memcpy(lp.n_int, n_int, sizeof n_int);
    lp.upd_max_speed = max_speed;
    lp.upd_delta_t = delta_t;
    lp.number = P;
    lg.un.active = true;
    lg.un.number = P;
    lg.un.plan = plan;
    lg.un.has_upd = has_upd; lg.un.max_speed = max_speed; lg.un.delta_t = delta_t;
    lg.un.cur_before = w->d.cur;
    lg.un.flag_base_before = w->flag_base;
    __atomic_store_n(&lg.box->posted, P, __ATOMIC_RELEASE);
    // (segment 0 of the post continues the last segment of the plan before: one launch-wide index less than a launch of its own)
    w->d.cur = (w->d.cur + (int)plan.size() - 1) & 1;
    w->flag_base += (unsigned long long)plan.size() - 1ull;
    w->stale_kinds |= ~w->p.enable_mask & 15u;  // disabled factors miss what these sweeps deliver
    w->last_sweep_launches++;  // (one submission: the schedule runs inside the launch that is there)
    w->last_sweep = lg.ran;
    w->last_sweep_form = MGX_SWEEP_FORM_POSTED;
    return MGX_OK;
}
static int run_resident(mgx_world *w, const std::vector<Launch> &plan) {
    if (w->linger.open) {
        // A launch lingers: the schedule is posted into it if it qualifies.  (mgx_tick comes here prepared, its records in the box
        // already — unless the launch it found had ended and the post taken back became THIS lingering launch: then the tick's
        // prior updates sit in the pinned ring, and are copied over; records in device memory, mgx_mission_tick_end's, cannot ride
        // in a post: the launch ends first.)
        if (w->d.upd && !w->upd_host) {
            const int rc = linger_close(w);
            if (rc != MGX_OK) return rc;
        } else {
            const int r = linger_prepare_post(w, plan);
            if (r < 0) return r;
            if (r == 1) {
                const bool has_upd = w->d.upd != nullptr;
                if (has_upd) memcpy(linger_upd_slot(w, w->launch_seq + 1ull), w->upd_host, 4 * (size_t)w->d.R_local * sizeof(double));
                (void)linger_post(w, plan, has_upd, w->d.upd_max_speed, w->d.upd_delta_t);
                return 1;
            }
        }
    }
    if (!resident_enabled() || w->resident_off || plan.size() < 2) return 0;
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    if (!resident_gate(w, plan)) return 0;
    StageTimer tr("resident");
    const DevWorld &d = w->d;
    const bool sharded = w->xres.connected;
    // What follows is this rank's own: where the ranks agree on every schedule (xres.agree) a rank
    // that cannot take part says so THERE — its launch is a single vote, and everybody takes the launch-by-launch path.
    const bool ranks_agree = sharded && w->xres.agree != nullptr;
    bool can = d.ir_max_edges > 0 && !w->conns.empty() && !w->thaw_kinds && !w->ir_thaw_active && w->n_keyless == 0 && !w->resident_decline;
    if (!can && !ranks_agree) return 0;
    if (can && sweep_lds_bytes(w->K, d.ir_max_edges, true) > sweep_resident_lds_max()) {
        if (!sharded) return 0;
        if (!ranks_agree) return fail(MGX_ERR_STATE, "resident launches were agreed on with the other ranks, but this rank's robots no longer fit LDS");
        can = false;
    }
    int &cap = sharded ? w->resident_cap_sharded : w->resident_cap;
    if (can) {
        if (cap < 0) cap = sweep_resident_capacity(d, sharded);
        if (d.R_local + 1 > cap) {  // (+ the residency census' decider workgroup: one slot kept free for it)
            if (!sharded) return 0;
            if (!ranks_agree && d.R_local > cap)
                return fail(MGX_ERR_STATE, "resident launches were agreed on with the other ranks, but only %d of this rank's %d workgroups "
                                           "are resident at once", cap, d.R_local);
            if (ranks_agree) can = false;
        }
    }
    tr.lap("gate + capacity");
    rc = ensure_resident_tables(w);
    if (rc != MGX_OK) return rc;
    tr.lap("peer tables");
    static const long long timeout_ticks = [] {
        const char *e = getenv("MGX_RESIDENT_TIMEOUT_MS");
        const long long ms = e ? atoll(e) : 2000;
        return (ms > 0 ? ms : 2000) * 100000ll;  // 100 MHz wall clock
    }();
    w->stale_kinds |= ~w->p.enable_mask & 15u;  // disabled factors miss what these sweeps deliver
    for (size_t i0 = 0; i0 < plan.size(); i0 += MAX_SEGS) {
        SegPlan sp{};
        sp.n = (int32_t)std::min<size_t>(MAX_SEGS, plan.size() - i0);
        for (int k = 0; k < sp.n; k++) {
            const Launch &l = plan[i0 + (size_t)k];
            sp.ext[k] = l.ext ? 1 : 0;
            sp.n_int[k] = (uint8_t)l.n_int;
        }
        sp.flag_base = w->flag_base;
        sp.timeout_ticks = timeout_ticks;
        // residency census + clean abort (SegPlan); the ranks of a sharded world abort together, on the word they agree on
        // (without one — mgx_halo_resident_connect_peers without a coordinator — they keep the plain bound on every wait)
        static const long long census_ticks = [] {
            const char *e = getenv("MGX_RESIDENT_CENSUS_US");
            const long long us = e ? atoll(e) : 200;
            return (us > 0 ? us : 200) * 100ll;  // 100 MHz wall clock
        }();
        static const long long census_ticks_sharded = [] {  // the ranks' hosts do not launch at the same instant
            const char *e = getenv("MGX_RESIDENT_CENSUS_SHARDED_US");
            const long long us = e ? atoll(e) : 20000;
            return (us > 0 ? us : 20000) * 100ll;
        }();
        static const bool census_on = [] { const char *e = getenv("MGX_RESIDENT_CENSUS"); return !(e && e[0] == '0'); }();
        const bool census = sharded ? ranks_agree : census_on;  // MGX_RESIDENT_CENSUS=0: plain bound on every wait
        if (census) {
            if (i0 > 0 && (rc = confirm_resident(w)) != MGX_OK) return rc;  // the previous part of this schedule
            if (i0 > 0 && w->resident_backoff > 0) {  // ... was sent back: the rest follows it launch by launch
                for (size_t i = i0; i < plan.size(); i++)
                    if ((rc = sweep(w, -1, plan[i].ext, plan[i].n_int ? (PH_INT_FACTOR | PH_INT_VARIABLE) : 0, plan[i].n_int, plan[i].hints)) != MGX_OK) return rc;
                return 1;
            }
            sp.launch_seq = ++w->launch_seq;
            sp.census_ticks = sharded ? census_ticks_sharded : census_ticks;
            if (ranks_agree) sp.agree_seq = ++w->xres.agree_seq;
        }
        // Lingering (mgx_dev.h): the launch that runs the END of the schedule stays for the schedules that follow — when the caller's
        // pattern promises some (schedules back to back, or no evidence yet that they are not: two lingering launches in a row that
        // ended without a post switch it off until schedules come back to back again)
        if (census && can && !sharded && i0 + (size_t)MAX_SEGS >= plan.size() && linger_ticks(w) > 0 &&
            (w->linger.useless < 2 || w->linger.streak >= 2)) {
            if ((rc = ensure_linger_box(w)) != MGX_OK) return rc;
            void *bd = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&bd, w->linger.box, 0));
            sp.linger_ticks = linger_ticks(w);
            sp.linger_box = (const LingerBox *)bd;
            sp.linger_upd = reinterpret_cast<const double *>(reinterpret_cast<const char *>(bd) + sizeof(LingerBox));
            sp.linger_upd_stride = (unsigned long long)w->linger.upd_stride;
            sp.linger_dev = w->linger.dev.p;
            sp.linger_dev_stride = (unsigned long long)w->linger.dev_stride;
            sp.linger_go = w->linger.go.p;
        }
        if (sharded && sp.ext[0]) {  // segment 0 reads the ghosts' plain copies: one direct exchange in front of the launch
            rc = direct_exchange(w);
            if (rc != MGX_OK) return rc;
        }
        // MGX_COOPERATIVE=1: hipLaunchCooperativeKernel — the runtime checks the grid against the occupancy query at launch
        // time (same residency as a plain launch, +15..19 us of host time per launch: MI355X_MICROARCH.md); a grid it turns
        // down takes the launch-per-segment path from now on instead of waiting for workgroups that never become resident
        static const bool cooperative = [] { const char *e = getenv("MGX_COOPERATIVE"); return e && e[0] == '1'; }();
        SweepRan ran;
        const hipError_t le = can ? launch_robot_schedule(w->d, w->d.R_local, sp, sharded, cooperative, w->stream, &ran)
                                  : launch_agree_abort(w->d, sp, w->stream);
        if (le != hipSuccess) {
            (void)hipGetLastError();
            if (cooperative && le == hipErrorCooperativeLaunchTooLarge && i0 == 0 && !sharded) {
                cap = 0;  // until the topology (hence the workgroup's LDS) changes
                return 0;
            }
            return fail(MGX_ERR_HIP, "resident schedule launch: %s", hipGetErrorString(le));
        }
        w->last_sweep_launches++;
        w->resident_launches++;
        if (can) {  // (a rank that voted no launched no sweep)
            w->last_sweep = ran;
            w->last_sweep_form = sharded ? MGX_SWEEP_FORM_SHARDED : MGX_SWEEP_FORM_RESIDENT;
        }
        if (sp.linger_ticks > 0) {
            mgx_world::Linger &lg = w->linger;
            lg.open = true;
            lg.seq0 = sp.launch_seq;
            lg.ran = ran;
            lg.taken_in_launch = 0;
            lg.un.active = false;
            lg.launches++;
        }
        if (census) {  // what confirm_resident needs to take the launch back and run it again launch by launch
            mgx_world::PendingResident &pd = w->pending;
            pd.active = true;
            pd.seq = sp.launch_seq;
            pd.partial = i0 > 0;
            pd.segs.clear();
            pd.hints.clear();
            for (int k = 0; k < sp.n; k++) {
                const Launch &l = plan[i0 + (size_t)k];
                pd.segs.emplace_back(l.ext, l.n_int);
                pd.hints.push_back(l.hints);
            }
            pd.cur_before = w->d.cur;
            pd.flag_base_before = w->flag_base;
            pd.upd = w->d.upd; pd.upd_max_speed = w->d.upd_max_speed; pd.upd_delta_t = w->d.upd_delta_t;
            pd.upd_slot = w->d.upd ? w->upd_ring_slot : -1;
        }
        w->d.upd = nullptr;  // mgx_tick's prior updates ride in the first launch only
        w->d.cur = (w->d.cur + sp.n) & 1;
        w->flag_base += (unsigned long long)sp.n;
        if (!census)
            for (int k = 0; k < sp.n; k++) {
                const Launch &l = plan[i0 + (size_t)k];
                log_launch(w, -1, l.ext, l.n_int ? (PH_INT_FACTOR | PH_INT_VARIABLE) : 0, l.n_int);
            }
    }
    return 1;
}
