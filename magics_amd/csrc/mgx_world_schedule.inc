// mgx_world_schedule.inc — C ABI: batches, mgx_iterate, prior changes, mgx_tick, resets, diagnostics, read-back.
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
extern "C" {
// ---- batches: several schedules, one submission ---------------------------------------------------------------------------
// A resident schedule launch pays for itself once: the robots' graphs go HBM -> LDS when it starts and back when it ends, some
// 12 us of a 94 us launch at 1000 x 16 (stamps: staging 17.6 k + write-back 14.7 k of 242 k clocks).  A caller that issues
// schedule after schedule with nothing in between (a planner that runs ahead, a benchmark loop) can bracket the loop: the
// schedules are recorded and submitted together, merged into as few launches as their segments fit (MAX_SEGS per launch) —
// the engine's form of capturing a launch-bound loop in a graph.  Nothing is reordered and nothing is skipped:
// iterate(a); iterate(b) computes exactly what iterate(a ++ b) computes (the phases are flattened either way), and every other
// call on the world first submits what was recorded (MGX_ENTER), so it finds the world as if each schedule had run when it was
// issued.
static int submit_batch(mgx_world *w) {
    std::vector<uint8_t> st;
    st.swap(w->batch.steps);  // (first: whatever runs below may pass MGX_ENTER again)
    const uint32_t merged = w->batch.implicit;  // (schedules mgx_iterate recorded by itself: they count as schedules where posted)
    w->batch.implicit = 0;
    if (st.empty()) return MGX_OK;
    ResidentLaunches::Linger &lg = w->res.linger;
    if (merged > 1) lg.streak += merged - 1;  // (iterate_now counts the submission as one schedule issued)
    lg.coming = std::max(merged, 1u);
    const int rc = iterate_now(w, st.data(), (uint32_t)st.size());
    lg.coming = 1;
    w->batch.submissions++;
    w->batch.launches += w->last_sweep_launches;
    return rc;
}

// ---- post merging: mgx_iterate records by itself while the launch that lingers is behind ----------------------------------
// Schedules issued back to back into a launch that lingers are posted one plan each, and the host stays at most two plans ahead:
// post P is taken only when every workgroup has picked up plan P - 2, and until then the host spins in linger_prepare_post.  In
// that time it already holds the next schedules — which could ride in ONE plan and spare the launch the boundaries between them
// (what the explicit batch above buys, without the caller asking).  So mgx_iterate outside a batch looks — once, without
// waiting — whether the post before is still untaken, and if so records its schedule in the batch's buffer instead of spinning
// (post_merge_decide, mgx_resident.h, has the rule).  MGX_ENTER_SCHEDULE / MGX_ENTER submit the buffer in front of every other
// entry point, so mgx_tick, every query, read, mgx_flush and mgx_synchronize find the world as ever; the one difference is that
// a recorded schedule reaches the device only with the caller's next call on the world (include/mgx.h, mgx_iterate).
// A launch lingers, its census is confirmed (waited for, as iterate_now would: it falls within microseconds of the launch's
// start) and it has not ended — the box's `closed` word, read once.
static int iterate_plan(mgx_world *w, const std::vector<Launch> &plan);
static bool linger_open_now(mgx_world *w, int *rc) {
    ResidentLaunches::Linger &lg = w->res.linger;
    *rc = MGX_OK;
    if (!lg.open) return false;
    const uint32_t count_before = w->last_sweep_launches;  // (a declined launch is run again here: not the coming schedule's launches)
    *rc = confirm_held(w);
    w->last_sweep_launches = count_before;
    if (*rc != MGX_OK || !lg.open) return false;
    const unsigned long long c = __atomic_load_n(&lg.box()->closed, __ATOMIC_ACQUIRE);
    return !((c & 1ull) && (c >> 1) >= lg.seq0);
}
static int iterate_merging(mgx_world *w, const uint8_t *steps, uint32_t n) {
    mgx_world::Batch &b = w->batch;
    ResidentLaunches::Linger &lg = w->res.linger;
    const int32_t mode = post_merge_mode(w);
    if (mode == POST_MERGE_OFF && b.steps.empty()) return iterate_now(w, steps, n);
    // (the checks of the explicit batch: a call that would fail when it runs fails when it is issued)
    if (w->robots.empty()) return fail(MGX_ERR_STATE, "world has no robots");
    int rc = check_device_error(w);
    if (rc != MGX_OK) return rc;
    const std::vector<Launch> fresh = plan_launches(steps, n);
    for (int round = 0; round < 2; round++) {  // (the second: behind SUBMIT_RECORDED, with nothing recorded)
        const bool held = !b.steps.empty();
        std::vector<Launch> merged_plan;
        if (held) {
            std::vector<uint8_t> both(b.steps);
            both.insert(both.end(), steps, steps + n);
            merged_plan = plan_launches(both.data(), (uint32_t)both.size());
        }
        const std::vector<Launch> &merged = held ? merged_plan : fresh;
        const bool open = linger_open_now(w, &rc);
        if (rc != MGX_OK) return rc;
        const unsigned outstanding = open && lg.un.active ? (unsigned)std::min<unsigned long long>(lg.un.number - lg.seq0, 1000ull) : 0u;
        const bool taken = outstanding && __atomic_load_n(&lg.box()->taken, __ATOMIC_ACQUIRE) >= lg.un.number;
        const PostMerge what = post_merge_decide(mode, open, outstanding, taken, linger_world_qualifies(w), held, fresh, merged);
        if (what == PostMerge::SUBMIT_RECORDED) {
            if ((rc = submit_batch(w)) != MGX_OK) return rc;
            continue;
        }
        if (what == PostMerge::SUBMIT && !held) return iterate_plan(w, fresh);  // (a post — or launches — of its own, as ever)
        b.steps.insert(b.steps.end(), steps, steps + n);
        b.implicit++;
        return what == PostMerge::DEFER ? MGX_OK : submit_batch(w);
    }
    return fail(MGX_ERR_STATE, "internal: a schedule was neither recorded nor submitted");
}

int mgx_batch_begin(mgx_world *w) {
    MGX_ENTER_SCHEDULE(w);  // (schedules mgx_iterate recorded by itself go out first: the batch's counters start clean)
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (w->batch.open) return fail(MGX_ERR_STATE, "a batch is open already");
    w->batch.open = true;
    w->batch.schedules = w->batch.submissions = w->batch.launches = 0;
    return MGX_OK;
}
int mgx_batch_end(mgx_world *w, uint32_t *n_schedules, uint32_t *n_launches) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->batch.open) return fail(MGX_ERR_STATE, "no batch is open");
    w->batch.open = false;
    const int rc = submit_batch(w);
    if (n_schedules) *n_schedules = w->batch.schedules;
    if (n_launches) *n_launches = w->batch.launches;
    return rc;
}

int mgx_iterate(mgx_world *w, const uint8_t *steps, uint32_t n) {
    if (!w || (!steps && n)) return fail(MGX_ERR_INVALID, "null argument");
    // (the same checks inside and outside a batch: a call that would fail when it runs fails when it is issued)
    for (uint32_t i = 0; i < n; i++)
        if (steps[i] & ~(MGX_STEP_INTERNAL | MGX_STEP_EXTERNAL)) return fail(MGX_ERR_INVALID, "bad step %u", i);
    if (!w->batch.open) {
        // (no launch lingers and nothing is recorded — every world that does not post, sharded ones among them: as ever)
        if (!w->res.linger.open && w->batch.steps.empty()) return iterate_now(w, steps, n);
        return iterate_merging(w, steps, n);
    }
    if (w->robots.empty()) return fail(MGX_ERR_STATE, "world has no robots");
    int rc0 = check_device_error(w);
    if (rc0 != MGX_OK) return rc0;
    mgx_world::Batch &b = w->batch;
    if (!b.steps.empty()) {  // does it still fit the launch the recorded ones make?
        std::vector<uint8_t> both(b.steps);
        both.insert(both.end(), steps, steps + n);
        if (plan_launches(both.data(), (uint32_t)both.size()).size() > (size_t)MAX_SEGS) {
            const int rc = submit_batch(w);
            if (rc != MGX_OK) return rc;
        }
    }
    b.steps.insert(b.steps.end(), steps, steps + n);
    b.schedules++;  // (recorded: a schedule whose predecessors' submission failed above is not counted)
    return MGX_OK;
}

// One schedule per robot group (include/mgx.h, ROBOT GROUPS).  Equal schedules are mgx_iterate itself — the same door, so resident
// launches, lingering, post merging and batches are as ever; a mixed call runs launch by launch (run_group_plan).
int mgx_iterate_groups(mgx_world *w, uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first) {
    int rc = group_schedule_arguments(w, n_groups, steps, step_first);
    if (rc != MGX_OK) return rc;
    const uint8_t *eq_steps = nullptr;
    uint32_t eq_n = 0;
    if (group_schedule_is_plain(w, n_groups, steps, step_first, &eq_steps, &eq_n, &rc)) return mgx_iterate(w, eq_steps, eq_n);
    if (rc != MGX_OK) return rc;
    MGX_ENTER(w);  // (ends a lingering launch and submits what was recorded, an open batch's schedules included)
    if ((rc = check_device_error(w)) != MGX_OK) return rc;
    MGX_CONFIRM(w);  // (a declined launch is run again here: not this call's launches)
    w->last_sweep_launches = 0;
    w->last_sweep = SweepRan{};
    w->last_sweep_form = -1;
    return run_group_plan(w, plan_group_launches(n_groups, steps, step_first));
}
int mgx_group_schedule_stats(mgx_world *w, uint64_t *mixed_calls, uint64_t *mixed_launches, uint64_t *sat_out) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (mixed_calls) *mixed_calls = w->gsched.mixed_calls;
    if (mixed_launches) *mixed_launches = w->gsched.mixed_launches;
    if (sat_out) *sat_out = w->gsched.sat_out;
    return MGX_OK;
}

static int iterate_now(mgx_world *w, const uint8_t *steps, uint32_t n) { return iterate_plan(w, plan_launches(steps, n)); }
static int iterate_plan(mgx_world *w, const std::vector<Launch> &plan) {
    const int rcc = confirm_held(w);  // (a declined launch is run again here: not this call's launches)
    if (rcc != MGX_OK) return rcc;
    w->last_sweep_launches = 0;
    w->last_sweep = SweepRan{};
    w->last_sweep_form = -1;
    w->res.schedule_issued();  // (every other entry point resets the streak: MGX_ENTER)
    return run_schedule(w, plan, RidingUpdates{});
}

int mgx_internal_factor_iteration(mgx_world *w, int32_t robot) {
    MGX_ENTER(w);
    return w ? sweep(w, robot, 0, PH_INT_FACTOR, 1) : fail(MGX_ERR_INVALID, "null world");
}
int mgx_internal_variable_iteration(mgx_world *w, int32_t robot) {
    MGX_ENTER(w);
    return w ? sweep(w, robot, 0, PH_INT_VARIABLE, 1) : fail(MGX_ERR_INVALID, "null world");
}
int mgx_external_factor_iteration(mgx_world *w, int32_t robot) {
    MGX_ENTER(w);
    return w ? sweep(w, robot, PH_EXT_FACTOR, 0, 0) : fail(MGX_ERR_INVALID, "null world");
}
int mgx_external_variable_iteration(mgx_world *w, int32_t robot) {
    MGX_ENTER(w);
    return w ? sweep(w, robot, PH_EXT_VARIABLE, 0, 0) : fail(MGX_ERR_INVALID, "null world");
}

int mgx_change_priors(mgx_world *w, uint32_t n, const int32_t *robots, const uint32_t *var_ix, const double *means) {
    MGX_ENTER(w);
    if (!w || !robots || !var_ix || !means) return fail(MGX_ERR_INVALID, "null argument");
    if (n == 0) return MGX_OK;
    for (uint32_t i = 0; i < n; i++) {
        if (robots[i] < 0 || (size_t)robots[i] >= w->robots.size() || w->robots[(size_t)robots[i]].ghost || w->robots[(size_t)robots[i]].removed || (int)var_ix[i] >= w->K)
            return fail(MGX_ERR_INVALID, "bad (robot, variable) at %u", i);
    }
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    // packed arguments, f64 words: means[4n] | device robot (int32)[n] | variable (uint32)[n]
    const size_t words = 4 * (size_t)n + (n + 1) / 2 + (n + 1) / 2;
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(words * sizeof(double), &hp, &slot));
    double *hm = (double *)hp;
    int32_t *hr = (int32_t *)(hm + 4 * (size_t)n);
    uint32_t *hv = (uint32_t *)(hm + 4 * (size_t)n + (n + 1) / 2);
    memcpy(hm, means, 4 * (size_t)n * sizeof(double));
    for (uint32_t i = 0; i < n; i++) { hr[i] = w->dev_of[(size_t)robots[i]]; hv[i] = var_ix[i]; log_change_prior(w, robots[i], (int)var_ix[i]); }
    void *dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    const double *dm = (const double *)dp;
    w->stale_kinds |= ~w->p.enable_mask & 15u;
    HIP_TRY(launch_change_prior(w->d, (int)n, (const int32_t *)(dm + 4 * (size_t)n), (const uint32_t *)(dm + 4 * (size_t)n + (n + 1) / 2), dm,
                                w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    return MGX_OK;
}
int mgx_update_priors(mgx_world *w, uint32_t n, const int32_t *robots, const double *waypoints_xy, const double *time_scale,
                      const uint8_t *what, double max_speed, double delta_t) {
    MGX_ENTER(w);
    if (!w || !robots || !waypoints_xy || !time_scale || !what) return fail(MGX_ERR_INVALID, "null argument");
    if (n == 0) return MGX_OK;
    if (w->K < 3) return fail(MGX_ERR_INVALID, "needs K >= 3");
    for (uint32_t i = 0; i < n; i++)
        if (robots[i] < 0 || (size_t)robots[i] >= w->robots.size() || w->robots[(size_t)robots[i]].ghost || w->robots[(size_t)robots[i]].removed || (what[i] & ~3u))
            return fail(MGX_ERR_INVALID, "bad entry %u", i);
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    // packed arguments, f64 words: waypoints[2n] | time_scale[n] | device robot (int32)[n] | what (u8)[n]
    const size_t w_r = (n + 1) / 2, w_w = (n + 7) / 8, words = 3 * (size_t)n + w_r + w_w;
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(words * sizeof(double), &hp, &slot));
    double *hw = (double *)hp;
    int32_t *hr = (int32_t *)(hw + 3 * (size_t)n);
    uint8_t *hh = (uint8_t *)(hw + 3 * (size_t)n + w_r);
    memcpy(hw, waypoints_xy, 2 * (size_t)n * sizeof(double));
    memcpy(hw + 2 * (size_t)n, time_scale, (size_t)n * sizeof(double));
    for (uint32_t i = 0; i < n; i++) {
        hr[i] = w->dev_of[(size_t)robots[i]];
        if (what[i] & 1u) log_change_prior(w, robots[i], w->K - 1);
        if (what[i] & 2u) log_change_prior(w, robots[i], 0);
    }
    memcpy(hh, what, n);
    void *dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    const double *dw = (const double *)dp;
    w->stale_kinds |= ~w->p.enable_mask & 15u;
    HIP_TRY(launch_update_priors(w->d, (int)n, (const int32_t *)(dw + 3 * (size_t)n), dw, dw + 2 * (size_t)n,
                                 (const uint8_t *)(dw + 3 * (size_t)n + w_r), max_speed, delta_t, w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    return MGX_OK;
}

// One driver tick in one call: update_prior_of_horizon_state + update_prior_of_current_state_v3 for the listed
// robots, then iterate_gbp_v2 (robot.rs:86-103).  When the schedule opens with an internal iteration — every
// schedule of the reference does — the two prior updates ride in the launch that runs it: each robot's
// workgroup applies them to the image it has just staged, which saves the separate kernel and its trip
// through HBM.  Otherwise (or while factors are thawing) this is mgx_update_priors followed by mgx_iterate.
int mgx_tick(mgx_world *w, uint32_t n, const int32_t *robots, const double *waypoints_xy, const double *time_scale,
             const uint8_t *what, double max_speed, double delta_t, const uint8_t *steps, uint32_t n_steps) {
    MGX_ENTER_SCHEDULE(w);
    if (!w || (!steps && n_steps) || (n && (!robots || !waypoints_xy || !time_scale || !what))) return fail(MGX_ERR_INVALID, "null argument");
    const std::vector<Launch> plan = plan_launches(steps, n_steps);
    const int rcc = confirm_held(w);  // (a declined launch is run again here: not this call's launches)
    if (rcc != MGX_OK) return rcc;
    w->last_sweep_launches = 0;
    w->last_sweep = SweepRan{};
    w->last_sweep_form = -1;
    // (a masked world — mgx_set_group_enabled — sends its prior updates as mixed calls do: no launch of a group plan carries them;
    // with mgx_set_group_resident they ride, and every fall-back to a group plan sends them first: run_segments)
    const bool fuse = n > 0 && !plan.empty() && plan[0].ext == 0 && plan[0].n_int > 0 && w->thaw_kinds == 0 && w->K >= 3 &&
                      (!w->gkinds.masked() || w->gkinds.resident);
    if (!fuse) {
        const int rc = n ? mgx_update_priors(w, n, robots, waypoints_xy, time_scale, what, max_speed, delta_t) : MGX_OK;
        return rc != MGX_OK ? rc : iterate_now(w, steps, n_steps);
    }
    for (uint32_t i = 0; i < n; i++)  // (the robots' ghost / removed flags from their compact copies)
        if (robots[i] < 0 || (size_t)robots[i] >= w->robots.size() || w->sets.ghost[(size_t)robots[i]] || w->sets.removed[(size_t)robots[i]] || (what[i] & ~3u))
            return fail(MGX_ERR_INVALID, "bad entry %u", i);
    StageTimer tmk("tick");
    const int rc = commit_held(w);  // (a lingering launch stays: this tick is posted into it if it qualifies)
    tmk.lap("commit (confirm + table rebuild)");
    if (rc != MGX_OK) return rc;
    const size_t RL = (size_t)w->d.R_local;
    void *hp = nullptr, *dp = nullptr;
    int slot = 0;
    // a launch lingers and takes this tick: the records go straight into the coming number's slot of its box (the pinned ring's
    // slots are guarded by events, and an event behind a launch that lingers does not complete)
    int posting = 0;
    if (w->res.linger.open && (posting = linger_prepare_post(w, plan, true)) < 0) return posting;
    double *rec = nullptr;
    if (posting) {
        rec = linger_upd_slot(w, w->res.launch_seq + 1ull);
    } else {
        HIP_TRY(w->stage.acquire(4 * RL * sizeof(double), &hp, &slot));
        rec = (double *)hp;
    }
    std::fill(rec, rec + 4 * RL, 0.0);
    for (uint32_t i = 0; i < n; i++) {
        double *q = rec + 4 * (size_t)w->dev_of[(size_t)robots[i]];
        q[0] = waypoints_xy[2 * i]; q[1] = waypoints_xy[2 * i + 1]; q[2] = time_scale[i]; q[3] = (double)what[i];
        if (what[i] & 1u) log_change_prior(w, robots[i], w->K - 1);
        if (what[i] & 2u) log_change_prior(w, robots[i], 0);
    }
    w->res.schedule_issued();  // (every other entry point resets the streak: MGX_ENTER)
    RidingUpdates upd;
    upd.host = rec;
    upd.max_speed = max_speed;
    upd.delta_t = delta_t;
    if (posting) {
        linger_post(w, plan, upd);
        tmk.lap("update records + counter log + post");
        return MGX_OK;
    }
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    w->stale_kinds |= ~w->p.enable_mask & 15u;
    tmk.lap("update records + counter log");
    // the whole tick as one resident launch when the world qualifies: the prior updates ride in it all the same
    upd.dev = (const double *)dp;
    upd.slot = slot;
    return run_schedule(w, plan, upd, &tmk);
}

// FactorGraph::reset_variables (factorgraph.rs:1541-1564: VariableNode::reset, variable.rs:350-360, for every variable, then
// FactorNode::empty_inbox, factor/mod.rs:480-483, for every factor of the graph).  In the engine's terms (DESIGN.md §3):
//   belief mean / precision  <- the given mean / diag(sigma) (the reference uses the sigma AS the precision's diagonal, +inf
//                               included); information vector, covariance, validity and the prior stay;
//   variable inboxes emptied <- own factor -> variable messages and the messages of foreign inter-robot factors attached to
//                               these variables become the empty (= zero) message;
//   own factors' inboxes emptied <- the variables' delivery counts restart at zero (an own factor's inbox entry is "present"
//                               once its variable has delivered; a tracking factor reads the record's mean even before, so
//                               that becomes zero as well), and for the inter-robot factors this graph owns the entry from
//                               the other robot's variable (its last response mean) is emptied and their creation epoch
//                               restarts with the count.
// A rare call (the reference makes it when a global path has been found, robot.rs:700-790): the device state is pulled,
// edited on the host mirror and laid out again by the next launch.
int mgx_reset_variables(mgx_world *w, int32_t robot, const double *means, uint32_t n_means, double first_last_sigma, double inbetween_sigma) {
    MGX_ENTER(w);
    if (!w || !means || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    if (w->robots[(size_t)robot].ghost || w->robots[(size_t)robot].removed) return fail(MGX_ERR_INVALID, "robot %d is not a live local robot", robot);
    if ((int)n_means != w->robots[(size_t)robot].K)  // factorgraph.rs:1548 asserts variable_indices.len() == means.len()
        return fail(MGX_ERR_INVALID, "%u means for a graph of %d variables", n_means, w->robots[(size_t)robot].K);
    int rc = pull(w);
    if (rc != MGX_OK) return rc;
    flush_counts(w);
    Robot &rb = w->robots[(size_t)robot];
    const int K = rb.K, E = 4 * K - 6;
    // connections made since the last commit whose TARGET is this robot took its variables' means when they were made
    // (robot.rs:1549-1585): they are settled now, as the commit would settle them, before the means are replaced
    for (IrConn &c : w->conns) {
        if (c.other != robot) continue;
        for (size_t j = 0; j < c.edges.size(); j++) {
            IrEdge &ed = c.edges[j];
            if (!ed.fresh) continue;
            ed.created = w->robots[(size_t)c.owner].epoch[j + 1];
            for (int q = 0; q < 4; q++) ed.bmu[q] = (w->p.enable_mask & 2u) ? rb.bel_mu[4 * (j + 1) + q] : 0.0;
            ed.fresh = false;
        }
    }
    for (int i = 0; i < K; i++) {
        const double sigma = (i == 0 || i == K - 1) ? first_last_sigma : inbetween_sigma;
        for (int c = 0; c < 4; c++) rb.bel_mu[4 * i + c] = means[4 * i + c];
        for (int c = 0; c < 16; c++) rb.bel_lam[16 * i + c] = (c % 5 == 0) ? sigma : 0.0;
        rb.epoch[(size_t)i] = 0;
        for (int c = 0; c < 4; c++) rb.snap[24 * i + 20 + c] = 0.0;
    }
    std::fill(rb.fv_eta.begin(), rb.fv_eta.begin() + 4 * E, 0.0);
    std::fill(rb.fv_lam.begin(), rb.fv_lam.begin() + 16 * E, 0.0);
    // ... the inboxes of switched-off and thawing factors too (empty_inbox asks no factor whether it is enabled): the entries they
    // froze with become empty; a factor without inbox keys stays without
    std::fill(rb.frozen.begin(), rb.frozen.end(), 0.0);
    for (uint8_t &fl : rb.frozen_flag) fl = fl == 2 ? 2 : 0;
    for (IrConn &c : w->conns) {
        if (c.other == robot)  // foreign factors attached to these variables: their message to us is emptied
            for (IrEdge &ed : c.edges) { std::fill(ed.fv_eta, ed.fv_eta + 4, 0.0); std::fill(ed.fv_lam, ed.fv_lam + 16, 0.0); }
        if (c.owner == robot)  // own inter-robot factors: both inbox entries emptied
            for (IrEdge &ed : c.edges) { std::fill(ed.bmu, ed.bmu + 4, 0.0); ed.created = 0; ed.fresh = false; }
    }
    w->dirty = w->relayout = true;
    w->dev_valid = false;  // the host mirror is the truth now: the next launch lays it out again (and must not pull over it)
    return MGX_OK;
}
// FactorGraph::reset_tracking_factors (factorgraph.rs:1566-1590): set_timeout(10) on every tracking factor of the graph —
// its next ten updates are skipped (tracking.rs:362-371) and send the empty message.
int mgx_reset_tracking_factors(mgx_world *w, int32_t robot) {
    MGX_ENTER(w);
    if (!w || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    if (w->robots[(size_t)robot].ghost || w->robots[(size_t)robot].removed) return fail(MGX_ERR_INVALID, "robot %d is not a live local robot", robot);
    int rc = pull(w);
    if (rc != MGX_OK) return rc;
    Robot &rb = w->robots[(size_t)robot];
    for (int32_t &rec : rb.trk_record) rec = (rec & 0xffff) | (11 << 16);  // Some(10), gbp_math.h tracking_timeout_skips
    w->dirty = w->relayout = true;
    w->dev_valid = false;
    return MGX_OK;
}
// FactorGraph::modify_tracking_factors(|t| t.set_tracking_path(path)) (factorgraph.rs:1467, tracking.rs:134-136; the
// completion handler's first call, robot.rs:674-682): the graph's tracking factors share the robot's polyline (Robot::path), so
// replacing it IS the call — records, last measurements and timeouts stay where they are (on the device: nothing is pulled).
// The packed path arrays are rebuilt from the host's per-robot paths in the device order of the layout there now and uploaded;
// a world about to be laid out again (dirty, or never laid out) takes the new path with that layout.
int mgx_set_tracking_path(mgx_world *w, int32_t robot, const float *path_xy, uint32_t n_path) {
    MGX_ENTER(w);
    if (n_path < 2) return fail(MGX_ERR_INVALID, "n_path must be >= 2 (TwoOrMore), got %u", n_path);
    if (!path_xy) return fail(MGX_ERR_INVALID, "null path");
    if (!w || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id");
    if (w->robots[(size_t)robot].ghost || w->robots[(size_t)robot].removed) return fail(MGX_ERR_INVALID, "robot %d is not a live local robot", robot);
    if (n_path > 0xffffu) return fail(MGX_ERR_INVALID, "n_path %u: a factor's record is kept in 16 bits", n_path);
    // (a resident launch the census declined is run again first: its schedule was issued under the old path)
    MGX_CONFIRM(w);
    w->robots[(size_t)robot].path.assign(path_xy, path_xy + 2 * (size_t)n_path);
    // (about to be laid out in full; robots that only wait to be appended bring their paths along, the ones on the device are packed here)
    if (w->relayout || !w->dev_valid) return MGX_OK;
    const size_t RL = (size_t)w->d.R_local;
    std::vector<int32_t> pptr(RL + 1, 0);
    std::vector<float> pxy;
    size_t longest = 0;
    for (size_t dr = 0; dr < RL; dr++) {  // (as commit packs them — every robot's again: one packed array, a rare call)
        const Robot &rb = w->robots[(size_t)w->robot_of[dr]];
        pptr[dr] = (int32_t)(pxy.size() / 2);
        pxy.insert(pxy.end(), rb.path.begin(), rb.path.end());
        pptr[dr + 1] = (int32_t)(pxy.size() / 2);
        longest = std::max(longest, rb.path.size());
    }
    if (pptr.size() > w->path_ptr.cap || pxy.size() > w->path_xy.cap)
        HIP_TRY(hipStreamSynchronize(w->stream));  // (an array that has to grow is freed first: nothing may still read it)
    HIP_TRY(w->path_ptr.upload(pptr, w->stream, (size_t)w->R_cap + 1));
    HIP_TRY(w->path_xy.upload(pxy, w->stream, pxy.size() > w->path_xy.cap ? path_room_for(w, pxy.size(), longest) : 0));
    w->d.path_ptr = w->path_ptr.p;
    w->d.path_xy = w->path_xy.p;
    HIP_TRY(hipStreamSynchronize(w->stream));  // the staging vectors die here
    return check_device_error(w);
}

// The whole path-finding completion handler (robot.rs:643-799) for a batch of robots: set_tracking_path, reset_variables,
// reset_tracking_factors, mission.state = Active, and — under device missions — Route::update_waypoints.  On a world that is
// laid out, unsharded and in none of the switching states the reset is applied IN PLACE (k_global_paths_robots /
// k_global_paths_owned, which restate the host edit of mgx_reset_variables above on the arrays pull() reads back): nothing is
// pulled, nothing is laid out again, the device stays the truth.  Any other world runs the per-robot calls above.
static int apply_global_route(mgx_world *w, int32_t robot, const float *xy, uint32_t n_path, bool on_device);
int mgx_apply_global_paths(mgx_world *w, uint32_t n, const int32_t *robots, const uint32_t *path_ptr, const float *path_xy, const double *means,
                           double first_last_sigma, double inbetween_sigma, uint32_t flags) {
    MGX_ENTER(w);
    if (!w || !robots || !path_ptr || !path_xy || !means) return fail(MGX_ERR_INVALID, "null argument");
    if (flags & ~(MGX_GLOBAL_PATH_RESET_TRACKING | MGX_GLOBAL_PATH_ROUTE | MGX_GLOBAL_PATH_ACTIVATE)) return fail(MGX_ERR_INVALID, "bad flags");
    if (n == 0) return MGX_OK;
    const mgx_world::Mission &msc = w->mission;
    std::vector<uint8_t> listed(w->robots.size(), 0);
    for (uint32_t i = 0; i < n; i++) {
        const int32_t r = robots[i];
        if (r < 0 || (size_t)r >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id at %u", i);
        if (w->robots[(size_t)r].ghost || w->robots[(size_t)r].removed) return fail(MGX_ERR_INVALID, "robot %d is not a live local robot", r);
        if (listed[(size_t)r]) return fail(MGX_ERR_INVALID, "robot %d is listed twice", r);
        listed[(size_t)r] = 1;
        if (path_ptr[i + 1] < path_ptr[i]) return fail(MGX_ERR_INVALID, "path_ptr decreases at %u", i);
        const uint32_t np = path_ptr[i + 1] - path_ptr[i];
        if (np < 2) return fail(MGX_ERR_INVALID, "path %u: n_path must be >= 2 (TwoOrMore), got %u", i, np);
        if (np > 0xffffu) return fail(MGX_ERR_INVALID, "path %u: n_path %u: a factor's record is kept in 16 bits", i, np);
        if (flags & MGX_GLOBAL_PATH_ROUTE) {
            if (!msc.any || (size_t)r >= msc.has.size() || !msc.has[(size_t)r]) return fail(MGX_ERR_STATE, "robot %d has no mission (mgx_mission_set)", r);
            if (msc.finished_tick[(size_t)r] >= 0) return fail(MGX_ERR_STATE, "robot %d has completed its mission", r);
        }
    }
    const int K = w->K;
    const bool sharded = std::find(w->sets.ghost.begin(), w->sets.ghost.end(), (uint8_t)1) != w->sets.ghost.end() || w->xres.connected;
    const bool in_place = w->dev_valid && !w->dirty && !sharded && !w->frozen_live && !w->ir_frozen_live && w->thaw_kinds == 0 && w->n_keyless == 0;
    if (!in_place) {  // the per-robot calls, in the handler's order (every one of them validated above)
        for (uint32_t i = 0; i < n; i++) {
            const int32_t r = robots[i];
            const float *xy = path_xy + 2 * (size_t)path_ptr[i];
            const uint32_t np = path_ptr[i + 1] - path_ptr[i];
            int rc = mgx_set_tracking_path(w, r, xy, np);
            if (rc == MGX_OK) rc = mgx_reset_variables(w, r, means + 4 * (size_t)K * i, (uint32_t)K, first_last_sigma, inbetween_sigma);
            if (rc == MGX_OK && (flags & MGX_GLOBAL_PATH_RESET_TRACKING)) rc = mgx_reset_tracking_factors(w, r);
            if (rc == MGX_OK && (flags & MGX_GLOBAL_PATH_ROUTE)) rc = apply_global_route(w, r, xy, np, false);
            if (rc == MGX_OK && (flags & MGX_GLOBAL_PATH_ACTIVATE)) rc = mgx_set_idle(w, r, 0);
            if (rc != MGX_OK) return rc;
        }
        return MGX_OK;
    }
    // pending topology and flag differences reach the device in place: no connection of a listed robot exists only on the host
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    flush_counts(w);
    const size_t RL = (size_t)w->d.R_local, RT = (size_t)w->d.R_total;
    for (uint32_t i = 0; i < n; i++) {
        const float *xy = path_xy + 2 * (size_t)path_ptr[i];
        w->robots[(size_t)robots[i]].path.assign(xy, xy + 2 * (size_t)(path_ptr[i + 1] - path_ptr[i]));
    }
    {  // the packed path arrays, as mgx_set_tracking_path rebuilds them
        std::vector<int32_t> pptr(RL + 1, 0);
        std::vector<float> pxy;
        size_t longest = 0;
        for (size_t dr = 0; dr < RL; dr++) {
            const Robot &rb = w->robots[(size_t)w->robot_of[dr]];
            pptr[dr] = (int32_t)(pxy.size() / 2);
            pxy.insert(pxy.end(), rb.path.begin(), rb.path.end());
            pptr[dr + 1] = (int32_t)(pxy.size() / 2);
            longest = std::max(longest, rb.path.size());
        }
        if (pptr.size() > w->path_ptr.cap || pxy.size() > w->path_xy.cap)
            HIP_TRY(hipStreamSynchronize(w->stream));  // (an array that has to grow is freed first: nothing may still read it)
        HIP_TRY(w->path_ptr.upload(pptr, w->stream, (size_t)w->R_cap + 1));
        HIP_TRY(w->path_xy.upload(pxy, w->stream, pxy.size() > w->path_xy.cap ? path_room_for(w, pxy.size(), longest) : 0));
        w->d.path_ptr = w->path_ptr.p;
        w->d.path_xy = w->path_xy.p;
        HIP_TRY(hipStreamSynchronize(w->stream));  // the staging vectors die here
    }
    mgx_world::Mission &ms = w->mission;
    const bool route = (flags & MGX_GLOBAL_PATH_ROUTE) != 0;
    const bool route_on_device = route && ms.uploaded && !ms.dirty && ms.has.size() == w->robots.size();
    if (route)
        for (uint32_t i = 0; i < n; i++)
            if ((rc = apply_global_route(w, robots[i], path_xy + 2 * (size_t)path_ptr[i], path_ptr[i + 1] - path_ptr[i], route_on_device)) != MGX_OK) return rc;
    if (route_on_device) {  // the packed waypoints, as mission_upload packs them; what the device advances is not laid out again
        const size_t R = w->robots.size();
        std::vector<int32_t> ptr(R + 1, 0);
        std::vector<double> xy;
        for (size_t r = 0; r < R; r++) {
            xy.insert(xy.end(), ms.wp[r].begin(), ms.wp[r].end());
            ptr[r + 1] = (int32_t)(xy.size() / 2);
        }
        if (xy.size() > ms.wp_xy_d.cap) HIP_TRY(hipStreamSynchronize(w->stream));
        HIP_TRY(ms.wp_ptr_d.upload(ptr, w->stream));
        HIP_TRY(ms.wp_xy_d.upload(xy, w->stream));
        ms.d.wp_ptr = ms.wp_ptr_d.p;
        ms.d.wp_xy = ms.wp_xy_d.p;
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    // ONE pinned block, f64 words: means [n][4][K] (component-major, as the blob keeps them) | device robots (int32)[n] | selected (u8)[R_total]
    const size_t w_m = 4 * (size_t)K * n, w_r = (n + 1) / 2, w_s = (RT + 7) / 8;
    void *hp = nullptr, *dp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire((w_m + w_r + w_s) * sizeof(double), &hp, &slot));
    double *hm = (double *)hp;
    int32_t *hr = (int32_t *)(hm + w_m);
    uint8_t *hs = (uint8_t *)(hm + w_m + w_r);
    memset(hs, 0, w_s * sizeof(double));
    for (uint32_t i = 0; i < n; i++) {
        const double *src = means + 4 * (size_t)K * i;
        double *dst = hm + 4 * (size_t)K * i;
        for (int v = 0; v < K; v++)
            for (int c = 0; c < 4; c++) dst[c * K + v] = src[4 * v + c];
        hr[i] = w->dev_of[(size_t)robots[i]];
        hs[(size_t)hr[i]] = 1;
    }
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    const double *dm = (const double *)dp;
    const int n_edges = w->dev_in_ptr.empty() ? 0 : w->dev_in_ptr.back() * (K - 1);
    if ((size_t)n_edges > w->ir_rec.n) return fail(MGX_ERR_STATE, "internal: %d edges on the device, %zu records", n_edges, w->ir_rec.n);
    HIP_TRY(launch_global_paths(w->d, (int)n, (const int32_t *)(dm + w_m), dm, first_last_sigma, inbetween_sigma,
                                (flags & MGX_GLOBAL_PATH_RESET_TRACKING) != 0, route_on_device ? ms.target_d.p : nullptr, n_edges, w->ir_rec.p,
                                (const uint8_t *)(dm + w_m + w_r), w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    if (flags & MGX_GLOBAL_PATH_ACTIVATE) {  // mission.state = Active (robot.rs:786): the flags travel with the next commit
        for (uint32_t i = 0; i < n; i++) {
            Robot &rb = w->robots[(size_t)robots[i]];
            if (rb.idle) { rb.idle = 0; w->flags_dirty = true; }
        }
    }
    return check_device_error(w);
}
// Route::update_waypoints (robot.rs:389-392, called at :778): the route becomes path[1:] — target_index = 1 skips the first point,
// the robot's own position — widened to f64, and the next waypoint is its first.  Reach rules, Transform and time scale stay.
// on_device: the device's mission arrays stay as they are (the caller uploads the packed waypoints and k_global_paths_robots
// rewinds the target); otherwise what the device has advanced is fetched first and the missions are laid out again.
static int apply_global_route(mgx_world *w, int32_t robot, const float *xy, uint32_t n_path, bool on_device) {
    mgx_world::Mission &ms = w->mission;
    if (!on_device && ms.uploaded && !ms.dirty) {
        const int rc = mission_download(w);
        if (rc != MGX_OK) return rc;
    }
    std::vector<double> &wp = ms.wp[(size_t)robot];
    wp.resize(2 * (size_t)(n_path - 1));
    for (size_t q = 0; q < wp.size(); q++) wp[q] = (double)xy[2 + q];
    ms.target[(size_t)robot] = 0;
    if (!on_device) ms.dirty = true;
    return MGX_OK;
}
// The world expects to hold up to `robots` robots: the next full layout sizes the per-robot arrays for that many, and commit()
// brings the robots that join afterwards onto the device in place (append_robots).  Before the first layout only the wish is
// recorded; a laid-out world is marked for ONE full layout with the head-room.
int mgx_world_reserve(mgx_world *w, uint32_t robots) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (robots > 0x3fffffffu) return fail(MGX_ERR_INVALID, "%u robots: more than a world can hold", robots);
    if ((size_t)robots <= w->robots.size() || robots <= w->reserve_want) return MGX_OK;  // (the head-room already there stays)
    w->reserve_want = robots;
    if (w->dev_valid && (int)robots > w->R_cap) w->dirty = w->relayout = true;
    return MGX_OK;
}
int mgx_append_stats(mgx_world *w, uint64_t *appends, uint64_t *robots_appended, uint64_t *fallbacks) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (appends) *appends = w->n_appends;
    if (robots_appended) *robots_appended = w->n_robots_appended;
    if (fallbacks) *fallbacks = w->n_append_fallbacks;
    return MGX_OK;
}
int mgx_layout_stats(mgx_world *w, uint64_t *n_layouts, uint64_t *n_pulls) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (n_layouts) *n_layouts = w->n_layouts;
    if (n_pulls) *n_pulls = w->n_pulls;
    return MGX_OK;
}

// Sharded worlds: a prior change applied on ANOTHER rank (to a robot that is a ghost here) still delivers a message to the
// inter-robot factors local robots own on that variable (variable.rs:210-221): the counters are told, nothing else happens.
int mgx_note_change_priors(mgx_world *w, uint32_t n, const int32_t *robots, const uint32_t *var_ix) {
    MGX_ENTER(w);
    if (!w || (n && (!robots || !var_ix))) return fail(MGX_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (robots[i] < 0 || (size_t)robots[i] >= w->robots.size() || (int)var_ix[i] >= w->K) return fail(MGX_ERR_INVALID, "bad (robot, variable) at %u", i);
    for (uint32_t i = 0; i < n; i++)
        if (!w->robots[(size_t)robots[i]].removed) log_change_prior(w, robots[i], (int)var_ix[i]);
    return MGX_OK;
}

int mgx_change_prior(mgx_world *w, int32_t robot, uint32_t var_ix, const double mean[4]) {
    MGX_ENTER(w);
    return mgx_change_priors(w, 1, &robot, &var_ix, mean);
}

int mgx_set_resident_launches(mgx_world *w, int32_t enabled) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    w->res.set_mode(enabled);
    return MGX_OK;
}
int mgx_is_thawing(mgx_world *w, int32_t *thawing) {
    MGX_ENTER(w);
    if (!w || !thawing) return fail(MGX_ERR_INVALID, "null argument");
    *thawing = (w->thaw_kinds || w->ir_thaw_active || w->n_keyless > 0) ? 1 : 0;
    return MGX_OK;
}
int mgx_last_launch_count(mgx_world *w, uint32_t *n_launches) {
    MGX_ENTER_SCHEDULE(w);
    if (!w || !n_launches) return fail(MGX_ERR_INVALID, "null argument");
    MGX_CONFIRM(w);
    *n_launches = w->last_sweep_launches;
    return MGX_OK;
}
int mgx_last_sweep(mgx_world *w, int32_t *variant, int32_t *ir_mode, int32_t *form, int32_t *resident_capacity) {
    MGX_ENTER_SCHEDULE(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    // (a resident launch the census declined has been run again launch by launch by the time it is decided: that is what ran)
    MGX_CONFIRM(w);
    if (variant) *variant = w->last_sweep.variant;
    if (ir_mode) *ir_mode = w->last_sweep.ir_mode;
    if (form) *form = w->last_sweep_form;
    if (resident_capacity) {
        const bool sharded = w->xres.connected;
        // (of the form that ran last, or that the next launch would take; not asked by a launch yet: asked here, for the topology on
        // the device — no commit, which would end a lingering launch)
        const uint32_t form = w->last_sweep.ir_mode >= 0 && w->last_sweep_form != MGX_SWEEP_FORM_SEGMENTS ? w->last_sweep.features : resident_features(w, false);
        int cap = w->res.cap[sharded ? 1 : 0][form & 7u];
        if (cap < 0) cap = device_ok() ? sweep_resident_capacity(w->d, sharded, form) : 0;
        *resident_capacity = cap;
    }
    return MGX_OK;
}
int mgx_last_sweep_features(mgx_world *w, uint32_t *features) {
    MGX_ENTER_SCHEDULE(w);
    if (!w || !features) return fail(MGX_ERR_INVALID, "null argument");
    MGX_CONFIRM(w);
    *features = w->last_sweep.ir_mode >= 0 ? w->last_sweep.features : 0u;
    return MGX_OK;
}
int mgx_last_search(mgx_world *w, int32_t *kernel, int32_t *row_cap, int32_t *n_launches, int32_t *n_changed, uint8_t *changed,
                    uint32_t capacity) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    const NeighbourSearch &S = w->search;
    if (kernel) *kernel = S.last_kernel;
    if (row_cap) *row_cap = S.last_cap;
    if (n_launches) *n_launches = S.last_launches;
    if (n_changed) *n_changed = S.last_changed;
    // (flags reach a pass only for a world without removed robots: one byte per robot of the world)
    if (changed && S.last_changed >= 0 && (size_t)capacity >= w->robots.size() && S.chg.size() >= w->robots.size())
        memcpy(changed, S.chg.data(), w->robots.size());
    return MGX_OK;
}

int mgx_num_robots(mgx_world *w, uint32_t *n_robots, uint32_t *n_variables) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    uint32_t nr = 0;
    for (const Robot &r : w->robots) nr += r.ghost ? 0 : 1;
    if (n_robots) *n_robots = nr;
    if (n_variables) *n_variables = nr * (uint32_t)w->K;
    return MGX_OK;
}

// the mean of variable `var_ix` of every local robot, id order: what the driver reads every tick
// (nth_variable(0) / last_variable for reached_waypoint, robot.rs:2125-2136; variables 0 and 1 for the
// Transform increment, robot.rs:2309-2330) — gathered on the device straight into pinned memory
int mgx_read_variable_means(mgx_world *w, uint32_t var_ix, double *means) {
    MGX_ENTER(w);
    if (!w || !means) return fail(MGX_ERR_INVALID, "null argument");
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    if ((int)var_ix >= w->K) return fail(MGX_ERR_INVALID, "variable index out of range");
    const size_t bytes = (size_t)w->d.R_local * 4 * sizeof(double);
    void *hp = nullptr, *dp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(bytes, &hp, &slot));
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    HIP_TRY(launch_gather_variable_means(w->d, (int)var_ix, (double *)dp, w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    memcpy(means, hp, bytes);
    return check_device_error(w);
}

// FactorGraph::messages_sent / messages_received (factorgraph.rs:876-890) of one robot's graph
int mgx_message_counts(mgx_world *w, int32_t robot, uint64_t counts[4]) {
    MGX_ENTER(w);
    if (!w || !counts || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    MGX_CONFIRM(w);
    if (w->robots[(size_t)robot].ghost) return fail(MGX_ERR_INVALID, "robot %d is a ghost here: its graph is counted on the rank that owns it", robot);
    flush_counts(w);
    const Robot &rb = w->robots[(size_t)robot];
    for (int c = 0; c < 4; c++) counts[c] = rb.cnt[c];
    for (const IrConn &cn : w->conns) {
        if (cn.owner != robot) continue;
        for (int c = 0; c < 4; c++) counts[c] += cn.cnt[c];
    }
    return MGX_OK;
}

// bulk read of the belief means only (what reached_waypoint and the visualisers read, robot.rs:2125-2136)
int mgx_read_means(mgx_world *w, double *means) {
    MGX_ENTER(w);
    if (!w || !means) return fail(MGX_ERR_INVALID, "null argument");
    return mgx_read_beliefs(w, nullptr, nullptr, means);
}


int mgx_read_beliefs(mgx_world *w, double *eta, double *lam, double *means) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    const int K = w->K;
    const BlobLayout L(K);
    const size_t BS = (size_t)w->d.BS, R = (size_t)w->d.R_local;
    // strided device -> host copies of the belief (eta, lam) and mean rows of every local blob
    std::vector<double> bel(R * 20 * K), mu(R * 4 * K);
    if (eta || lam)
        HIP_TRY(hipMemcpy2DAsync(bel.data(), 20 * K * sizeof(double), w->blob.p + L.bel(), BS * sizeof(double),
                                 20 * K * sizeof(double), R, hipMemcpyDeviceToHost, w->stream));
    if (means)
        HIP_TRY(hipMemcpy2DAsync(mu.data(), 4 * K * sizeof(double), w->blob.p + L.mu(), BS * sizeof(double),
                                 4 * K * sizeof(double), R, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    if ((rc = check_device_error(w)) != MGX_OK) return rc;
    // device local order == id order of non-ghost robots
    for (size_t r = 0; r < R; r++)
        for (int i = 0; i < K; i++) {
            const size_t v = r * K + i;
            if (eta)
                for (int c = 0; c < 4; c++) eta[4 * v + c] = bel[r * 20 * K + c * K + i];
            if (lam)
                for (int c = 0; c < 16; c++) lam[16 * v + c] = bel[r * 20 * K + (4 + c) * K + i];
            if (means)
                for (int c = 0; c < 4; c++) means[4 * v + c] = mu[r * 4 * K + c * K + i];
        }
    return MGX_OK;
}

int mgx_get_belief(mgx_world *w, int32_t robot, uint32_t var_ix, double eta[4], double lam[16], double mean[4], double cov[16],
                   int32_t *valid) {
    MGX_ENTER(w);
    if (!w || robot < 0 || (size_t)robot >= w->robots.size() || (int)var_ix >= w->K) return fail(MGX_ERR_INVALID, "bad (robot, variable)");
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    const int K = w->K, i = (int)var_ix;
    const BlobLayout L(K);
    std::vector<double> b((size_t)w->d.BS);
    HIP_TRY(hipMemcpyAsync(b.data(), w->blob.p + (size_t)w->dev_of[(size_t)robot] * w->d.BS, sizeof(double) * b.size(),
                           hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    if ((rc = check_device_error(w)) != MGX_OK) return rc;
    if (eta)
        for (int c = 0; c < 4; c++) eta[c] = b[L.bel() + c * K + i];
    if (lam)
        for (int c = 0; c < 16; c++) lam[c] = b[L.bel() + (4 + c) * K + i];
    if (mean)
        for (int c = 0; c < 4; c++) mean[c] = b[L.mu() + c * K + i];
    if (cov)
        for (int c = 0; c < 16; c++) cov[c] = b[L.cov() + c * K + i];
    if (valid) *valid = reinterpret_cast<const int32_t *>(b.data() + L.valid())[i];
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
