// mgx_world_missions.inc — C ABI: missions on the device, many ticks per call, fine-grained sweeps, schedules -> launches.
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
extern "C" {
// ---- missions on the device (SURVEY §8 f1) ---------------------------------------------------------------------------
static int mission_download(mgx_world *w) {  // device -> host copies of what the device advances (before the arrays are laid out again)
    mgx_world::Mission &ms = w->mission;
    if (!ms.uploaded) return MGX_OK;
    std::vector<int32_t> tg, lg;
    std::vector<float> tr;
    std::vector<long long> fin;
    HIP_TRY(ms.target_d.download(tg, w->stream));
    HIP_TRY(ms.translation_d.download(tr, w->stream));
    HIP_TRY(ms.finished_d.download(fin, w->stream));
    HIP_TRY(ms.legs_d.download(lg, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    for (size_t r = 0; r < tg.size() && r < ms.target.size(); r++) {
        ms.target[r] = tg[r];
        ms.finished_tick[r] = fin[r];
        ms.legs_left[r] = lg[r];
        for (int c = 0; c < 3; c++) ms.translation[3 * r + c] = tr[3 * r + c];
    }
    return MGX_OK;
}
static int mission_upload(mgx_world *w) {
    mgx_world::Mission &ms = w->mission;
    const size_t R = w->robots.size();
    ms.wp.resize(R);
    ms.target.resize(R, 0); ms.vars.resize(2 * R, 0); ms.dist2.resize(2 * R, 0.f); ms.translation.resize(3 * R, 0.f);
    ms.time_scale.resize(R, 0.0); ms.has.resize(R, 0); ms.finished_tick.resize(R, -1); ms.legs_left.resize(R, 0);
    std::vector<int32_t> ptr(R + 1, 0);
    std::vector<double> xy;
    for (size_t r = 0; r < R; r++) {
        xy.insert(xy.end(), ms.wp[r].begin(), ms.wp[r].end());
        ptr[r + 1] = (int32_t)(xy.size() / 2);
    }
    if (xy.empty()) xy.assign(2, 0.0);
    hipStream_t s = w->stream;
    HIP_TRY(ms.wp_ptr_d.upload(ptr, s));
    HIP_TRY(ms.wp_xy_d.upload(xy, s));
    HIP_TRY(ms.target_d.upload(ms.target, s));
    HIP_TRY(ms.vars_d.upload(ms.vars, s));
    HIP_TRY(ms.dist2_d.upload(ms.dist2, s));
    HIP_TRY(ms.translation_d.upload(ms.translation, s));
    HIP_TRY(ms.time_scale_d.upload(ms.time_scale, s));
    HIP_TRY(ms.has_d.upload(ms.has, s));
    HIP_TRY(ms.finished_d.upload(ms.finished_tick, s));
    HIP_TRY(ms.legs_d.upload(ms.legs_left, s));
    HIP_TRY(ms.rec_d.reserve(4 * R));
    HIP_TRY(ms.robots_d.reserve(R));
    HIP_TRY(ms.waypoints_d.reserve(2 * R));
    HIP_TRY(ms.ts_list_d.reserve(R));
    HIP_TRY(ms.what_d.reserve(R));
    HIP_TRY(ms.moving_d.reserve(R));
    HIP_TRY(hipStreamSynchronize(s));
    if (ms.ev_cap < R + 1) {
        if (ms.ev_host) (void)hipHostFree(ms.ev_host);
        ms.ev_host = nullptr;
        HIP_TRY(hipHostMalloc((void **)&ms.ev_host, sizeof(unsigned int) * (R + 64), hipHostMallocMapped));
        ms.ev_cap = R + 64;
        ms.ev_host[0] = 0;
    }
    DevMission &d = ms.d;
    d.wp_ptr = ms.wp_ptr_d.p; d.wp_xy = ms.wp_xy_d.p; d.target = ms.target_d.p; d.vars = ms.vars_d.p; d.dist2 = ms.dist2_d.p;
    d.time_scale = ms.time_scale_d.p; d.has = ms.has_d.p; d.translation = ms.translation_d.p; d.finished_tick = ms.finished_d.p; d.legs_left = ms.legs_d.p;
    ms.uploaded = true;
    ms.dirty = false;
    ms.alive_dirty = true;
    return MGX_OK;
}

int mgx_mission_set(mgx_world *w, int32_t robot, const mgx_mission_desc *desc) {
    MGX_ENTER(w);
    if (!w || !desc || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    const Robot &rb = w->robots[(size_t)robot];
    if (rb.ghost || rb.removed) return fail(MGX_ERR_INVALID, "robot %d is not a live local robot", robot);
    if (desc->n_waypoints == 0 || !desc->waypoints_xy) return fail(MGX_ERR_INVALID, "a mission needs at least one waypoint");
    if ((int)desc->reach_var >= rb.K || (int)desc->finish_var >= rb.K) return fail(MGX_ERR_INVALID, "rule names a variable beyond the horizon");
    if (desc->legs_after > 0x7fffffffu) return fail(MGX_ERR_INVALID, "legs_after %u: more legs than a mission can count", desc->legs_after);
    if (collisions_sharded(w)) return fail(MGX_ERR_STATE, "missions run on unsharded worlds");
    mgx_world::Mission &ms = w->mission;
    if (ms.uploaded && !ms.dirty) {  // the device has advanced the missions it holds: fetch before the arrays are laid out again
        int rc = mission_download(w);
        if (rc != MGX_OK) return rc;
    }
    const size_t R = w->robots.size(), r = (size_t)robot;
    ms.wp.resize(R);
    ms.target.resize(R, 0); ms.vars.resize(2 * R, 0); ms.dist2.resize(2 * R, 0.f); ms.translation.resize(3 * R, 0.f);
    ms.time_scale.resize(R, 0.0); ms.has.resize(R, 0); ms.finished_tick.resize(R, -1); ms.legs_left.resize(R, 0);
    ms.wp[r].assign(desc->waypoints_xy, desc->waypoints_xy + 2 * (size_t)desc->n_waypoints);
    ms.target[r] = 0;
    ms.vars[2 * r] = desc->reach_var; ms.vars[2 * r + 1] = desc->finish_var;
    ms.dist2[2 * r] = desc->reach_dist2; ms.dist2[2 * r + 1] = desc->finish_dist2;
    for (int c = 0; c < 3; c++) ms.translation[3 * r + c] = desc->translation[c];
    ms.time_scale[r] = desc->time_scale;
    ms.has[r] = 1;
    ms.finished_tick[r] = -1;
    ms.legs_left[r] = (int32_t)desc->legs_after;
    ms.any = true;
    ms.dirty = true;
    return MGX_OK;
}

int mgx_mission_tick(mgx_world *w, float comms_radius, uint32_t method, uint64_t *robot_number_next, int32_t despawn_finished,
                     const uint8_t *antennas, double max_speed, double delta_t, const uint8_t *steps, uint32_t n_steps, uint32_t *stats) {
    MGX_ENTER(w);
    int rc = mgx_mission_tick_begin(w, comms_radius, method, robot_number_next, despawn_finished, stats);
    return rc != MGX_OK ? rc : mgx_mission_tick_end(w, antennas, max_speed, delta_t, steps, n_steps);
}

static int mission_tick_begin(mgx_world *w, float comms_radius, uint32_t method, uint64_t *robot_number_next, int32_t despawn_finished,
                              uint32_t *stats, uint32_t n_groups, const float *radii = nullptr);
int mgx_mission_tick_begin(mgx_world *w, float comms_radius, uint32_t method, uint64_t *robot_number_next, int32_t despawn_finished,
                           uint32_t *stats) {
    MGX_ENTER(w);
    if (!w || !robot_number_next) return fail(MGX_ERR_INVALID, "null argument");
    if (*robot_number_next == 0) return fail(MGX_ERR_INVALID, "robot_number is NonZeroUsize");
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    return mission_tick_begin(w, comms_radius, method, robot_number_next, despawn_finished, stats, 0);
}
int mgx_mission_tick_begin_groups(mgx_world *w, float comms_radius, uint32_t method, uint32_t n_groups, uint64_t *number_next,
                                  int32_t despawn_finished, uint32_t *stats) {
    MGX_ENTER(w);
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    const int rc = groups_arguments(w, n_groups, number_next);
    if (rc != MGX_OK) return rc;
    const std::vector<float> radii((size_t)n_groups, comms_radius);  // (the radii call with all radii equal)
    return mission_tick_begin(w, comms_radius, method, number_next, despawn_finished, stats, n_groups, radii.data());
}
int mgx_mission_tick_begin_groups_radii(mgx_world *w, const float *comms_radii, uint32_t method, uint32_t n_groups, uint64_t *number_next,
                                        int32_t despawn_finished, uint32_t *stats) {
    MGX_ENTER(w);
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    if (!comms_radii) return fail(MGX_ERR_INVALID, "null argument (radii)");
    const int rc = groups_arguments(w, n_groups, number_next);
    if (rc != MGX_OK) return rc;
    return mission_tick_begin(w, comms_radii[0], method, number_next, despawn_finished, stats, n_groups, comms_radii);
}
// n_groups: 0 — one generator, stats {created, deleted, completed}; otherwise one generator and one stats triple per group.
// radii (may be null): [n_groups], one comms radius per group (an ungrouped world: radii[0], which comms_radius is)
static int mission_tick_begin(mgx_world *w, float comms_radius, uint32_t method, uint64_t *robot_number_next, int32_t despawn_finished,
                              uint32_t *stats, uint32_t n_groups, const float *radii) {
    int rc = MGX_OK;
    mgx_world::Mission &ms = w->mission;
    if (!ms.any) return fail(MGX_ERR_STATE, "no robot has a mission (mgx_mission_set)");
    if (w->K < 3) return fail(MGX_ERR_INVALID, "needs K >= 3");
    if (w->sets.n_grouped == 0) radii = nullptr;  // (the scalar search)
    const std::vector<float> now = radii ? std::vector<float>(radii, radii + n_groups) : std::vector<float>();
    rc = commit(w);
    if (rc != MGX_OK) return rc;
    if (w->d.R_total != w->d.R_local) return fail(MGX_ERR_STATE, "missions run on unsharded worlds");
    if (ms.dirty || ms.has.size() != w->robots.size()) {
        if (ms.uploaded && !ms.dirty && (rc = mission_download(w)) != MGX_OK) return rc;
        if ((rc = mission_upload(w)) != MGX_OK) return rc;
        w->search.mission.valid = false;  // the host has touched the missions: Transforms may have moved
    }
    const int R = (int)w->robots.size();
    hipStream_t s = w->stream;
    StageTimer tm("mission_tick");
    // reached_waypoint (robot.rs:2080-2176), then update_robot_neighbours on the Transforms as they are (robot.rs:1362-1384);
    // both results come back at the tick's ONE synchronisation (inside neighbours())
    ms.ev_host[0] = 0;
    void *evd = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&evd, ms.ev_host, 0));
    HIP_TRY(launch_mission_reached(w->d, ms.d, R, ms.tick_no, (unsigned int *)evd, s));
    std::vector<int32_t> ptr, idx;
    // the search itself was enqueued by the last tick's end, in front of its GBP schedule, if nothing has changed since: the same
    // radius — every group's, where they have one each — and method, the same robots alive (this tick's despawns are taken out of
    // the rows below either way)
    NeighbourSearch::PendingSearch &pf = w->search.mission;
    bool prefetched = pf.valid && pf.radius == comms_radius && pf.radii == now && pf.method == method && pf.n_all == R;
    if (prefetched) {
        size_t a = 0;
        for (int r = 0; r < R && prefetched; r++)
            if (!w->robots[(size_t)r].removed) {
                if (a >= pf.alive.size() || pf.alive[a] != r) prefetched = false;
                a++;
            }
        if (a != pf.alive.size()) prefetched = false;
    }
    rc = prefetched ? neighbours_collect(w, pf, ptr, idx) : neighbours(w, nullptr, comms_radius, method, ptr, idx, radii, radii ? n_groups : 0);
    if (rc != MGX_OK) return rc;
    ms.search_radius = comms_radius;
    ms.search_radii = now;
    ms.search_method = method;
    ms.search_known = true;
    tm.lap(prefetched ? "reached + rows of the search enqueued last tick" : "reached + search");
    // robots that reached their last waypoint this tick: despawned before the topology systems see them (robot.rs:2172) —
    // the search still looked at them, so they are taken out of its rows here
    // ... and the robots that ended a leg with legs left (the ids with MISSION_EVENT_LEG): MissionState::Idle from here on
    // (Mission::next_route, robot.rs:987, inside reached_waypoint: ahead of the chain) — the flags and the edge gates travel with
    // mission_tick_end's commit, ahead of the tick's sweeps and of its counter log.  They stay in the world and in the search's rows
    const unsigned n_ev = ms.ev_host[0];
    std::vector<uint8_t> gone;
    ms.last_finished.clear();
    ms.last_leg_ended.clear();
    std::vector<int> fin;
    for (unsigned e = 0; e < n_ev; e++) {
        const unsigned int id = ms.ev_host[1 + e];
        if (id & MISSION_EVENT_LEG) ms.last_leg_ended.push_back((int32_t)(id & ~MISSION_EVENT_LEG));
        else fin.push_back((int)id);
    }
    if (!ms.last_leg_ended.empty()) {
        std::sort(ms.last_leg_ended.begin(), ms.last_leg_ended.end());
        flush_counts(w);
        for (int32_t r : ms.last_leg_ended) w->robots[(size_t)r].idle = 1;
        w->flags_dirty = true;
    }
    const unsigned n_fin = (unsigned)fin.size();
    if (n_fin) {
        std::sort(fin.begin(), fin.end());
        ms.last_finished.assign(fin.begin(), fin.end());
        for (int r : fin) ms.finished_tick[(size_t)r] = ms.tick_no;
        if (despawn_finished) {
            gone.assign((size_t)R, 0);
            for (int r : fin) {
                gone[(size_t)r] = 1;
                if ((rc = mgx_robot_remove(w, r)) != MGX_OK) return rc;
            }
            std::vector<int32_t> nptr((size_t)R + 1, 0), nidx;
            nidx.reserve(idx.size());
            for (int r = 0; r < R; r++) {
                if (!gone[(size_t)r])
                    for (int32_t q = ptr[(size_t)r]; q < ptr[(size_t)r + 1]; q++)
                        if (!gone[(size_t)idx[(size_t)q]]) nidx.push_back(idx[(size_t)q]);
                nptr[(size_t)r + 1] = (int32_t)nidx.size();
            }
            ptr.swap(nptr);
            idx.swap(nidx);
        }
    }
    if (n_groups) {
        rc = topology_bookkeeping(w, ptr, idx, robot_number_next, stats, tm, nullptr, n_groups, 3);
        if (rc != MGX_OK) return rc;
        if (stats) {
            for (uint32_t g = 0; g < n_groups; g++) stats[3 * (size_t)g + 2] = 0;
            for (int32_t r : ms.last_finished) stats[3 * (size_t)w->sets.group[(size_t)r] + 2] += 1;
        }
    } else {
        uint32_t st[2] = {0, 0};
        rc = topology_bookkeeping(w, ptr, idx, robot_number_next, st, tm);
        if (rc != MGX_OK) return rc;
        if (stats) { stats[0] = st[0]; stats[1] = st[1]; stats[2] = n_fin; }
    }
    ms.in_tick = true;
    return MGX_OK;
}

// The observers' part of a tick's second half (mgx_world_observers.inc): over the Transforms after this tick's move (pos_d), the
// robots alive after its despawns (alive_d) and the ones k_mission_prepare has just moved (what_d), enqueued on `s`
static int observers_tick_end(mgx_world *w, const float *pos_d, const uint8_t *alive_d, const uint8_t *what_d, hipStream_t s) {
    int rc = MGX_OK;
    // update_robot_robot_collisions (collisions.rs:72-140) on the Transforms after this tick's move and the robots alive after its
    // despawns: enqueued here, in front of the schedule's launches — no synchronisation, nothing read back (mgx_collisions_read)
    if (w->coll.enabled && (rc = collisions_pass(w, pos_d, alive_d, s)) != MGX_OK) return rc;
    // update_robot_environment_collisions (collisions.rs:368-438), beside it on the same stream (mgx_env_collisions_read)
    if (w->envcoll.enabled && (rc = env_collisions_pass(w, pos_d, alive_d, s)) != MGX_OK) return rc;
    // goal_area::detect_collisions (goal_area.rs:67-103), beside them on the same Transforms and alive bytes (mgx_goal_areas_read);
    // the goal areas' own clock then names the coming tick
    if (w->goals.enabled) {
        if ((rc = goal_areas_pass(w, pos_d, alive_d, w->goals.clock, s)) != MGX_OK) return rc;
        w->goals.clock += 1;
    }
    // track_positions / track_velocities (tracking.rs:117-136, 210-240) and the distance travelled, for the robots k_mission_prepare
    // has just moved (its `what` flags): in front of the prior updates, which change the means the increment is formed from
    // again — no synchronisation, nothing read back (mgx_tracks_take).  The world's clock then names the coming tick
    if (w->tracks.enabled) {
        if ((rc = tracks_pass(w, pos_d, what_d, w->tracks.clock, true, s)) != MGX_OK) return rc;
        w->tracks.clock += 1;
    }
    return MGX_OK;
}

static int mission_tick_end(mgx_world *w, const uint8_t *antennas, double max_speed, double delta_t, const uint8_t *steps, uint32_t n_steps, const GroupPlan *mixed);
int mgx_mission_tick_end(mgx_world *w, const uint8_t *antennas, double max_speed, double delta_t, const uint8_t *steps, uint32_t n_steps) {
    MGX_ENTER(w);
    if (!w || (!steps && n_steps)) return fail(MGX_ERR_INVALID, "null argument");
    return mission_tick_end(w, antennas, max_speed, delta_t, steps, n_steps, nullptr);
}
// ... with one schedule per robot group (include/mgx.h, ROBOT GROUPS): equal schedules are the call above; a mixed one runs the
// prior updates as the kernel of their own and then the groups' segments launch by launch (run_group_plan)
int mgx_mission_tick_end_groups(mgx_world *w, const uint8_t *antennas, double max_speed, double delta_t, uint32_t n_groups, const uint8_t *steps,
                                const uint32_t *step_first) {
    int rc = group_schedule_arguments(w, n_groups, steps, step_first);
    if (rc != MGX_OK) return rc;
    const uint8_t *eq_steps = nullptr;
    uint32_t eq_n = 0;
    if (group_schedule_is_plain(w, n_groups, steps, step_first, &eq_steps, &eq_n, &rc)) return mgx_mission_tick_end(w, antennas, max_speed, delta_t, eq_steps, eq_n);
    if (rc != MGX_OK) return rc;
    MGX_ENTER(w);
    const GroupPlan gp = plan_group_launches(n_groups, steps, step_first);
    return mission_tick_end(w, antennas, max_speed, delta_t, nullptr, 0, &gp);
}
// mixed (may be null): the groups' own segments in place of the one schedule `steps`
static int mission_tick_end(mgx_world *w, const uint8_t *antennas, double max_speed, double delta_t, const uint8_t *steps, uint32_t n_steps, const GroupPlan *mixed) {
    mgx_world::Mission &ms = w->mission;
    if (!ms.in_tick) return fail(MGX_ERR_STATE, "mgx_mission_tick_end without mgx_mission_tick_begin");
    ms.in_tick = false;
    int rc = MGX_OK;
    const int R = (int)w->robots.size();
    hipStream_t s = w->stream;
    StageTimer tm("mission_tick_end");
    if (ms.dirty || ms.has.size() != w->robots.size()) {  // robots joined between the two halves: lay the missions out again
        if (ms.uploaded && !ms.dirty && (rc = mission_download(w)) != MGX_OK) return rc;
        if ((rc = commit(w)) != MGX_OK) return rc;
        if ((rc = mission_upload(w)) != MGX_OK) return rc;
    }
    // update_failed_comms (robot.rs:1593-1601): the caller's draws for the robots still alive
    if (antennas) {
        bool changed = false;
        for (int r = 0; r < R; r++) {
            Robot &rb = w->robots[(size_t)r];
            if (rb.removed || rb.ghost) continue;
            const uint8_t a = antennas[r] ? 1 : 0;
            if (rb.antenna != a) { if (!changed) flush_counts(w); changed = true; rb.antenna = a; }
        }
        if (changed) w->flags_dirty = true;
    }
    if ((rc = commit(w)) != MGX_OK) return rc;  // edge tables / flags of what the pass changed
    tm.lap("antennas + commit");
    // the two prior updates + the Transform increment, from the device's own mission state; then iterate_gbp_v2
    {
        void *hp = nullptr, *dp = nullptr;
        int slot = 0;
        HIP_TRY(w->stage.acquire((size_t)R, &hp, &slot));
        uint8_t *mv = (uint8_t *)hp;
        for (int r = 0; r < R; r++) mv[r] = observed(w->robots[(size_t)r]) ? 1 : 0;
        HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
        HIP_TRY(launch_copy_bytes(ms.moving_d.p, (const uint8_t *)dp, (size_t)R, s));
        HIP_TRY(w->stage.release(slot, s));
    }
    HIP_TRY(launch_mission_prepare(w->d, ms.d, R, ms.moving_d.p, ms.rec_d.p, ms.robots_d.p, ms.waypoints_d.p, ms.ts_list_d.p, ms.what_d.p, s));
    // the collision passes, the goal areas and the trackers: the last of them in front of the prior updates
    if ((rc = observers_tick_end(w, ms.translation_d.p, ms.moving_d.p, ms.what_d.p, s)) != MGX_OK) return rc;
    // the Transforms after this tick's move travel to the host behind the launch: complete at the next synchronisation
    // (the next tick's own one), read without one by mgx_mission_translations
    if (ms.tr_cap < (size_t)R) {
        if (ms.tr_host) (void)hipHostFree(ms.tr_host);
        ms.tr_host = nullptr;
        HIP_TRY(hipHostMalloc((void **)&ms.tr_host, sizeof(float) * 3 * ((size_t)R + 64), hipHostMallocDefault));
        ms.tr_cap = (size_t)R + 64;
    }
    HIP_TRY(hipMemcpyAsync(ms.tr_host, ms.translation_d.p, sizeof(float) * 3 * (size_t)R, hipMemcpyDeviceToHost, s));
    ms.tr_n = (size_t)R;
    // update_robot_neighbours of the COMING tick (robot.rs:1362-1384): the Transforms it looks at are final now, so the search goes
    // in front of this tick's GBP schedule and its rows reach the host while that runs
    tm.lap("prepare");
    if (ms.search_known && (rc = neighbours_enqueue(w, nullptr, ms.search_radius, ms.search_method, w->search.mission, false,
                                                    ms.search_radii.empty() ? nullptr : ms.search_radii.data(), (uint32_t)ms.search_radii.size())) != MGX_OK)
        return rc;
    tm.lap("search of the coming tick enqueued");
    for (int r = 0; r < R; r++) {  // message counters: the prior changes of the robots that move (what the device decides too)
        const Robot &rb = w->robots[(size_t)r];
        if (rb.removed || rb.ghost || rb.idle || !ms.has[(size_t)r] || ms.finished_tick[(size_t)r] >= 0) continue;
        log_change_prior(w, r, w->K - 1);
        log_change_prior(w, r, 0);
    }
    w->stale_kinds |= ~w->p.enable_mask & 15u;
    tm.lap("counter log");
    const std::vector<Launch> plan = plan_launches(steps, n_steps);
    MGX_CONFIRM(w);  // (a declined launch is run again here: not this call's launches)
    w->last_sweep_launches = 0;
    w->last_sweep = SweepRan{};
    w->last_sweep_form = -1;
    // (a masked world — mgx_set_group_enabled — sends its prior updates as mixed calls do: no launch of a group plan carries them;
    // with mgx_set_group_resident they ride, and every fall-back to a group plan sends them first: run_segments)
    const bool fuse = !mixed && !plan.empty() && plan[0].ext == 0 && plan[0].n_int > 0 && w->thaw_kinds == 0 &&
                      (!w->gkinds.masked() || w->gkinds.resident);
    if (mixed) {
        HIP_TRY(launch_update_priors(w->d, R, ms.robots_d.p, ms.waypoints_d.p, ms.ts_list_d.p, ms.what_d.p, max_speed, delta_t, s));
        rc = run_group_plan(w, *mixed);
    } else if (!fuse) {
        HIP_TRY(launch_update_priors(w->d, R, ms.robots_d.p, ms.waypoints_d.p, ms.ts_list_d.p, ms.what_d.p, max_speed, delta_t, s));
        rc = iterate_now(w, steps, n_steps);
    } else {
        RidingUpdates upd;  // (in device memory: no host view, no ring slot)
        upd.dev = ms.rec_d.p;
        upd.max_speed = max_speed;
        upd.delta_t = delta_t;
        rc = run_schedule(w, plan, upd);
    }
    ms.tick_no += 1;
    tm.lap("prior updates + schedule");
    // plans that ride the ticks (mgx_planner_set_tick_budget): one slice for every pending request, behind this tick's launches on
    // the same stream — a planner workgroup beside them would take a CU's LDS from the resident launch's census
    if (rc == MGX_OK && w->planner.enabled && w->planner.tick_budget) rc = plan_pool_advance(w->planner.pool, w->planner, w->stream, w->planner.tick_budget);
    return rc;
}

// Many ticks in one call (include/mgx.h): the host loop of a headless run — tick, comms draws, tick — without the caller's
// interpreter in it.  Nothing new happens on the device: the two halves above, once per tick.
int mgx_mission_run(mgx_world *w, mgx_mission_run_desc *d) {
    MGX_ENTER(w);
    if (!w || !d || !d->robot_number_next || (!d->steps && d->n_steps) || !d->created || !d->deleted || !d->n_finished ||
        (d->finished_capacity && !d->finished))
        return fail(MGX_ERR_INVALID, "null argument");
    if (!(d->failure_rate >= 0.0 && d->failure_rate <= 1.0)) return fail(MGX_ERR_INVALID, "failure_rate is outside [0, 1]");
    if (w->gkinds.masked())
        return fail(MGX_ERR_STATE, "mgx_mission_run on a world whose groups have enabled kinds or sigmas of their own (mgx_set_group_enabled, mgx_set_group_sigmas): "
                                   "one generator and one schedule are one group's");
    mgx_world::Mission &ms = w->mission;
    const size_t R = w->robots.size();
    d->ticks_done = 0;
    d->finished_total = 0;
    // rand 0.8.5 Bernoulli over wyrand 0.2.0 (restated in magics_amd/prng.py, which is the checker of this copy): one u64 per
    // draw unless p == 1
    const bool always = d->failure_rate == 1.0;
    const unsigned long long p_int = always ? 0ull : (unsigned long long)(d->failure_rate * 18446744073709551616.0);
    auto next_u64 = [&]() {
        unsigned long long &st = *reinterpret_cast<unsigned long long *>(d->wyrand_state);
        st += 0xA0761D6478BD642Full;
        const unsigned __int128 t = (unsigned __int128)st * (unsigned __int128)(st ^ 0xE7037ED1A0B428DBull);
        return (unsigned long long)(t >> 64) ^ (unsigned long long)t;
    };
    std::vector<uint8_t> ant(R, 1);
    int rc = MGX_OK;
    for (uint32_t t = 0; t < d->n_ticks; t++) {
        uint32_t st[3] = {0, 0, 0};
        if ((rc = mgx_mission_tick_begin(w, d->comms_radius, d->method, d->robot_number_next, d->despawn_finished, st)) != MGX_OK) return rc;
        if (w->robots.size() != R) return fail(MGX_ERR_STATE, "robots joined during mgx_mission_run");
        // (the tick's synchronisation lies behind: the Transforms the tick before sent to the host are complete)
        if (t > 0 && d->translations && ms.tr_host) memcpy(d->translations + (size_t)(t - 1) * R * 3, ms.tr_host, sizeof(float) * 3 * R);
        d->created[t] = st[0];
        d->deleted[t] = st[1];
        d->n_finished[t] = st[2];
        for (int32_t r : ms.last_finished) {
            if (d->finished_total < d->finished_capacity) d->finished[d->finished_total] = r;
            d->finished_total++;
        }
        // update_failed_comms (robot.rs:1593-1601): one draw per robot alive after this tick's despawns, id order
        bool any_off = false;
        if (d->wyrand_state)
            for (size_t r = 0; r < R; r++) {
                const Robot &rb = w->robots[r];
                if (rb.removed || rb.ghost) { ant[r] = 1; continue; }
                const bool fails = always ? true : next_u64() < p_int;
                ant[r] = fails ? 0 : 1;
                any_off = any_off || fails;
            }
        if (d->antennas) memcpy(d->antennas + (size_t)t * R, ant.data(), R);
        (void)any_off;
        if ((rc = mgx_mission_tick_end(w, (d->wyrand_state && d->failure_rate > 0.0) ? ant.data() : nullptr, d->max_speed, d->delta_t, d->steps,
                                       d->n_steps)) != MGX_OK)
            return rc;
        d->ticks_done = t + 1;
        if (!ms.last_leg_ended.empty()) break;  // a leg ended: the caller plans the next one (mgx_mission_legs_ended says whose)
        if (d->stop_when_all_finished) {
            bool all = true;
            for (size_t r = 0; r < R && all; r++) all = !ms.has[r] || ms.finished_tick[r] >= 0;
            if (all) break;
        }
    }
    if (d->ticks_done && d->translations) {  // the last tick's Transforms: behind its launches
        if ((rc = linger_close(w)) != MGX_OK || (rc = confirm_resident(w)) != MGX_OK) return rc;
        HIP_TRY(hipStreamSynchronize(w->stream));
        if (ms.tr_host) memcpy(d->translations + (size_t)(d->ticks_done - 1) * R * 3, ms.tr_host, sizeof(float) * 3 * R);
        if ((rc = check_device_error(w)) != MGX_OK) return rc;
    }
    if (d->finished_total > d->finished_capacity) return fail(MGX_ERR_INVALID, "%u missions completed, room for %u", d->finished_total, d->finished_capacity);
    return MGX_OK;
}

int mgx_mission_finished(mgx_world *w, int32_t *robots, uint32_t capacity, uint32_t *n) {
    MGX_ENTER(w);
    if (!w || !n) return fail(MGX_ERR_INVALID, "null argument");
    const std::vector<int32_t> &f = w->mission.last_finished;
    *n = (uint32_t)f.size();
    if (robots)
        for (size_t i = 0; i < f.size() && i < capacity; i++) robots[i] = f[i];
    return MGX_OK;
}
int mgx_mission_legs_ended(mgx_world *w, int32_t *robots, uint32_t capacity, uint32_t *n) {
    MGX_ENTER(w);
    if (!w || !n) return fail(MGX_ERR_INVALID, "null argument");
    const std::vector<int32_t> &f = w->mission.last_leg_ended;
    *n = (uint32_t)f.size();
    if (robots)
        for (size_t i = 0; i < f.size() && i < capacity; i++) robots[i] = f[i];
    return MGX_OK;
}
int mgx_mission_translations(mgx_world *w, float *translations, uint32_t capacity_robots, uint32_t *n_robots) {
    MGX_ENTER(w);
    if (!w || !translations) return fail(MGX_ERR_INVALID, "null argument");
    const mgx_world::Mission &ms = w->mission;
    const size_t n = std::min<size_t>(ms.tr_n, capacity_robots);
    if (ms.tr_host && n) memcpy(translations, ms.tr_host, sizeof(float) * 3 * n);
    if (n_robots) *n_robots = (uint32_t)ms.tr_n;
    return MGX_OK;
}

int mgx_mission_read(mgx_world *w, float *translations, int32_t *targets, int64_t *finished_tick) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::Mission &ms = w->mission;
    if (!ms.any) return fail(MGX_ERR_STATE, "no robot has a mission");
    if (ms.uploaded && !ms.dirty) {
        int rc = mission_download(w);
        if (rc != MGX_OK) return rc;
    }
    const size_t R = std::min(w->robots.size(), ms.target.size());
    for (size_t r = 0; r < R; r++) {
        if (translations) for (int c = 0; c < 3; c++) translations[3 * r + c] = ms.translation[3 * r + c];
        if (targets) targets[r] = ms.has[r] ? ms.target[r] : -1;
        if (finished_tick) finished_tick[r] = ms.finished_tick[r];
    }
    return check_device_error(w);
}

int mgx_mission_legs_read(mgx_world *w, int32_t *legs_left) {
    MGX_ENTER(w);
    if (!w || !legs_left) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::Mission &ms = w->mission;
    if (!ms.any) return fail(MGX_ERR_STATE, "no robot has a mission");
    if (ms.uploaded && !ms.dirty) {
        int rc = mission_download(w);
        if (rc != MGX_OK) return rc;
    }
    const size_t R = std::min(w->robots.size(), ms.legs_left.size());
    for (size_t r = 0; r < w->robots.size(); r++) legs_left[r] = (r < R && ms.has[r]) ? ms.legs_left[r] : 0;
    return check_device_error(w);
}

int mgx_sweep(mgx_world *w, int32_t robot, uint32_t external_phases, uint32_t internal_phases, uint32_t n_internal,
              uint32_t hints) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if ((external_phases & ~3u) || (internal_phases & ~3u)) return fail(MGX_ERR_INVALID, "bad phase mask");
    if (hints & ~MGX_HINT_NEXT_STARTS_EXTERNAL) return fail(MGX_ERR_INVALID, "bad hints");
    if (n_internal > 1 && internal_phases != 3u) return fail(MGX_ERR_INVALID, "fused iterations need both internal phases");
    const uint32_t h = ((hints & MGX_HINT_NEXT_STARTS_EXTERNAL) && (external_phases & 1u)) ? HINT_IR_DEAD : 0u;
    return sweep(w, robot, external_phases, internal_phases << 2, internal_phases ? (int)n_internal : 0, h);
}

}  // extern "C" (continued in the next part)
