// mgx_world_abi.inc — C ABI: lifecycle, environment, robots, connections, factor kinds, flags.
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// =========================================================================================================
//                                            C ABI
// =========================================================================================================
extern "C" {

const char *mgx_last_error(void) { return g_err.c_str(); }
// for the other translation units of the library (mgx_linalg.cpp): same thread-local text
int mgx_set_error_(int code, const char *text) {
    g_err = text ? text : "";
    return code;
}

int mgx_world_create(const mgx_params *params, mgx_world **out) {
    if (!params || !out) return fail(MGX_ERR_INVALID, "null argument");
    if (!(params->sigma_dynamics > 0) || !(params->sigma_interrobot > 0) || !(params->sigma_obstacle > 0) ||
        !(params->sigma_tracking > 0) || !(params->safety_multiplier > 0))
        return fail(MGX_ERR_INVALID, "sigmas and safety multiplier must be positive");
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
    mgx_world *w = new (std::nothrow) mgx_world();
    if (!w) return fail(MGX_ERR_NOMEM, "out of memory");
    w->p = *params;
    w->trk_ever_on = (params->enable_mask & 8u) != 0;
    *out = w;
    return MGX_OK;
}

int mgx_world_destroy(mgx_world *w) {
    if (!w) return MGX_OK;
    w->batch.steps.clear();
    (void)linger_close(w);  // (nobody is left to post: the launch would wait out its bound)
    if (w->dev_valid) (void)hipStreamSynchronize(w->stream);
    if (w->rccl.comm && g_rccl.ok) (void)g_rccl.comm_destroy(w->rccl.comm);
    if (w->direct.recv) (void)hipFree(w->direct.recv);
    if (w->direct.flags) (void)hipFree(w->direct.flags);
    if (w->xres.area) (void)hipFree(w->xres.area);
    if (w->search.stream) { (void)hipStreamSynchronize(w->search.stream); (void)hipStreamDestroy(w->search.stream); }
    if (w->sweep_err_host) (void)hipHostFree(w->sweep_err_host);
    if (w->mission.ev_host) (void)hipHostFree(w->mission.ev_host);
    if (w->mission.tr_host) (void)hipHostFree(w->mission.tr_host);
    delete w;
    return MGX_OK;
}

int mgx_set_stream(mgx_world *w, void *hip_stream) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (w->dev_valid) HIP_TRY(hipStreamSynchronize(w->stream));
    w->stream = (hipStream_t)hip_stream;
    return MGX_OK;
}

int mgx_synchronize(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
    MGX_CONFIRM(w);
    HIP_TRY(hipStreamSynchronize(w->stream));
    return check_device_error(w);
}

// Everything issued so far is ENQUEUED: recorded schedules are submitted and a lingering launch is told to end (it writes back and
// leaves the stream to what the caller puts behind it) — without waiting for the stream.
int mgx_flush(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    return MGX_OK;
}
int mgx_set_linger(mgx_world *w, int32_t microseconds) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    w->res.set_linger(microseconds);
    return MGX_OK;
}
int mgx_set_specialize(mgx_world *w, int32_t enabled) {
    MGX_ENTER(w);  // (a launch that lingers ends: the next one takes the form asked for here)
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    w->res.specialize = enabled < 0 ? -1 : (enabled ? 1 : 0);
    return MGX_OK;
}
int mgx_linger_stats(mgx_world *w, uint64_t *launches, uint64_t *posts, uint64_t *reruns, uint64_t *ended_by_device) {
    MGX_ENTER_SCHEDULE(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    const ResidentLaunches::Linger &lg = w->res.linger;
    if (launches) *launches = lg.launches;
    if (posts) *posts = lg.posts + (lg.un.active ? lg.un.schedules : 0u);
    if (reruns) *reruns = lg.reruns;
    if (ended_by_device) *ended_by_device = lg.ended_by_device;
    return MGX_OK;
}

int mgx_set_post_merge(mgx_world *w, int32_t mode) {
    MGX_ENTER_SCHEDULE(w);  // (what was recorded under the old mode goes out first; a launch that lingers stays)
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (mode > POST_MERGE_ALWAYS) return fail(MGX_ERR_INVALID, "bad post-merge mode %d", mode);
    w->res.linger.merge_mode = mode < 0 ? -1 : mode;
    return MGX_OK;
}
int mgx_post_merge_stats(mgx_world *w, uint64_t *plans_posted, uint64_t *schedules_in_them, uint64_t *largest) {
    MGX_ENTER_SCHEDULE(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    const ResidentLaunches::Linger &lg = w->res.linger;
    if (plans_posted) *plans_posted = lg.plans_posted;
    if (schedules_in_them) *schedules_in_them = lg.schedules_in_plans;
    if (largest) *largest = lg.largest_plan;
    return MGX_OK;
}

int mgx_world_set_sdf(mgx_world *w, const uint8_t *rgb, uint32_t width, uint32_t height, double world_w, double world_h) {
    MGX_ENTER(w);
    if (!w || !rgb || !width || !height || !(world_w > 0) || !(world_h > 0)) return fail(MGX_ERR_INVALID, "bad sdf arguments");
    w->sdf_red.resize((size_t)width * height);
    for (size_t i = 0; i < w->sdf_red.size(); i++) w->sdf_red[i] = rgb[3 * i];  // pixel[0], obstacle.rs:178
    w->sdf_w = width; w->sdf_h = height; w->world_w = world_w; w->world_h = world_h;
    w->dirty = w->relayout = true;
    return MGX_OK;
}

int mgx_world_set_environment(mgx_world *w, const mgx_env_desc *env) {
    MGX_ENTER(w);
    if (!w || !env) return fail(MGX_ERR_INVALID, "null argument");
    uint32_t W = 0, H = 0;
    const int rc = env_red_plane(env, env->sdf_resolution, env->sdf_expansion, env->sdf_blur, true, w->stream, w->sdf_red, W, H);
    if (rc != MGX_OK) return rc;
    w->sdf_w = W; w->sdf_h = H;
    w->world_w = (double)env->tile_size * (double)env->n_cols;  // robot.rs:1259-1264
    w->world_h = (double)env->tile_size * (double)env->n_rows;
    w->dirty = w->relayout = true;
    return MGX_OK;
}

int mgx_robot_add(mgx_world *w, const mgx_robot_desc *d, int32_t *robot_id) {
    MGX_ENTER(w);
    // (what the descriptor alone says comes first: it needs no world)
    if (d && d->group >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "group %u is not below MGX_GROUPS_MAX (%u)", d->group, MGX_GROUPS_MAX);
    if (d && d->group && d->ghost) return fail(MGX_ERR_INVALID, "a ghost has no group");
    if (!w || !d || !d->mean0 || !d->prior_diag || !d->dt) return fail(MGX_ERR_INVALID, "null argument");
    if (d->K < 3) return fail(MGX_ERR_INVALID, "K must be >= 3");
    if (w->K && (int)d->K != w->K) return fail(MGX_ERR_INVALID, "all robots of a world share K (%d), got %u", w->K, d->K);
    if (!(d->radius > 0)) return fail(MGX_ERR_INVALID, "radius must be positive");
    if (d->group && w->obs.n_ghosts) return fail(MGX_ERR_STATE, "robot groups are for unsharded worlds: this one has ghosts");
    if (d->ghost && w->sets.n_grouped) return fail(MGX_ERR_STATE, "a grouped world takes no ghosts");
    for (const Robot &o : w->robots)
        if (o.order_key == d->order_key) return fail(MGX_ERR_INVALID, "duplicate order_key");
    const int K = (int)d->K, E = 4 * K - 6;
    Robot rb;
    rb.K = K; rb.ghost = d->ghost != 0; rb.radius = d->radius; rb.order_key = d->order_key;
    rb.n_nodes = K + (K - 1) + 2 * (K - 2);
    flush_counts(w);  // launches logged so far do not concern the new robot
    {   // add_internal_edge (factorgraph.rs:304-330): the variable receives an (empty) message, the factor one if enabled
        const uint32_t en = w->kinds_of_group(d->group);  // (the group's own kinds where it was given some: mgx_set_group_enabled)
        rb.cnt[2] =(uint64_t)(2 * (K - 1) + 2 * (K - 2)) + ((en & 1u) ? 2 * (K - 1) : 0) + ((en & 4u) ? K - 2 : 0) + ((en & 8u) ? K - 2 : 0);
        // a robot that joins a world that has iterated: its switched-off factors stay without inbox keys, and switching the kind
        // on has something to thaw even if no sweep runs in between
        if (w->n_layouts > 0) {
            rb.nokey = (uint8_t)(~en & 13u);
            w->stale_kinds |= ~en & 13u;
        }
    }
    rb.prior_eta.assign(4 * K, 0.0); rb.prior_lam.assign(16 * K, 0.0);
    rb.bel_eta.assign(4 * K, 0.0); rb.bel_lam.assign(16 * K, 0.0); rb.bel_mu.assign(4 * K, 0.0); rb.bel_cov.assign(16 * K, 0.0);
    rb.valid.assign(K, 1); rb.snap.assign(24 * K, 0.0); rb.epoch.assign(K, 0);
    rb.fv_eta.assign(4 * E, 0.0); rb.fv_lam.assign(16 * E, 0.0); rb.dyn_m.assign(16 * (K - 1), 0.0);
    rb.trk_record.assign(K - 2, 0); rb.trk_last_pos.assign(2 * (K - 2), 0.f); rb.trk_last_val.assign(K - 2, 0.0);
    for (int i = 0; i < K; i++) {  // VariableNode::new, variable.rs:140-166
        double pd = d->prior_diag[i];
        if (!std::isfinite(pd)) pd = 0.0;  // :146-148
        double lam[16] = {0}, cov[16] = {0};
        for (int a = 0; a < 4; a++) lam[a * 5] = pd;
        const double *m = d->mean0 + 4 * i;
        for (int a = 0; a < 4; a++) {
            double s = 0.0;
            for (int b = 0; b < 4; b++) s += lam[a * 4 + b] * m[b];
            rb.prior_eta[4 * i + a] = s;
            rb.bel_eta[4 * i + a] = s;
            rb.bel_mu[4 * i + a] = m[a];
        }
        memcpy(&rb.prior_lam[16 * i], lam, sizeof lam);
        memcpy(&rb.bel_lam[16 * i], lam, sizeof lam);
        if (!inv4(lam, cov)) memset(cov, 0, sizeof cov);  // :152-154
        memcpy(&rb.bel_cov[16 * i], cov, sizeof cov);
        bool fin = true;
        for (double c : cov) fin = fin && std::isfinite(c);
        rb.valid[i] = fin;
        // what prepare_message() would send (variable.rs:234-240): seeds the tracking factor inbox
        // (factorgraph.rs:315-317); all other inboxes start empty (epoch 0)
        memcpy(&rb.snap[24 * i], &rb.bel_eta[4 * i], 4 * sizeof(double));
        memcpy(&rb.snap[24 * i + 4], lam, sizeof lam);
        memcpy(&rb.snap[24 * i + 20], m, 4 * sizeof(double));
    }
    const double sigma_dynamics = w->sigmas_of_group(d->group).dynamics;  // (the group's own where it was given sigmas: mgx_set_group_sigmas)
    for (int f = 0; f < K - 1; f++) {
        if (!(d->dt[f] > 0)) return fail(MGX_ERR_INVALID, "dt must be positive");
        dynamic_potential(d->dt[f], sigma_dynamics, &rb.dyn_m[16 * f]);
    }
    for (int j = 0; j < K - 2; j++) {  // new_tracking_factor, factor/mod.rs:269-274
        rb.trk_last_pos[2 * j] = (float)d->mean0[4 * (j + 1)];
        rb.trk_last_pos[2 * j + 1] = (float)d->mean0[4 * (j + 1) + 1];
    }
    if (d->n_path && d->path_xy) rb.path.assign(d->path_xy, d->path_xy + 2 * (size_t)d->n_path);
    w->sets.keys.push_back(rb.order_key);
    w->sets.ghost.push_back(rb.ghost ? 1 : 0);
    w->obs.n_ghosts += rb.ghost ? 1 : 0;
    w->sets.radius.push_back(rb.radius);
    w->sets.removed.push_back(0);
    w->sets.group.push_back(d->group);
    w->sets.n_grouped += d->group ? 1 : 0;
    if (w->gkinds.populated.size() <= d->group) w->gkinds.populated.resize((size_t)d->group + 1, 0);
    w->gkinds.populated[d->group] = 1;  // (from here on the group's kinds are fixed)
    w->robots.push_back(std::move(rb));
    w->sets.ensure(w->robots.size());
    w->K = K;
    w->dirty = true;  // (robots were added — a reason of its own: a world with head-room takes them on the device, commit())
    if (robot_id) *robot_id = (int32_t)w->robots.size() - 1;
    return MGX_OK;
}

static int ir_connect(mgx_world *w, int32_t owner, int32_t other, uint64_t first_robot_number) {
    if (!w || owner < 0 || other < 0 || (size_t)owner >= w->robots.size() || (size_t)other >= w->robots.size() || owner == other)
        return fail(MGX_ERR_INVALID, "bad robot ids");
    if (first_robot_number == 0) return fail(MGX_ERR_INVALID, "robot_number is NonZeroUsize");
    // no "already connected" check: the reference creates whatever its connection sets ask for, and
    // a pair can legitimately hold two sets of factors (robot.rs:1391-1404, see mgx_update_topology)
    flush_counts(w, true);  // (the robots' counters: what they answer changes with the connection; the other connections' can wait)
    IrConn c;
    c.owner = owner; c.other = other; c.first_number = first_robot_number;
    c.base[0] = w->cum.nIv[(size_t)owner]; c.base[1] = w->cum.nEv[(size_t)other]; c.base[2] = w->cum.nEf[(size_t)owner];
    c.base[3] = w->cum.on_ir[(size_t)owner]; c.base[4] = w->cum.on_ir[(size_t)other];
    if (!w->pool_edges.empty()) { c.edges.swap(w->pool_edges.back()); w->pool_edges.pop_back(); }  // (a deleted connection's storage)
    if (!w->pool_nodes.empty()) { c.node.swap(w->pool_nodes.back()); w->pool_nodes.pop_back(); }
    c.edges.assign((size_t)w->K - 1, IrEdge{});
    c.node.assign((size_t)w->K - 1, 0);
    // add_internal_edge + add_external_edge + the other variable's belief into the new factor
    // (factorgraph.rs:304-353, robot.rs:1557-1585)
    w->robots[(size_t)owner].cnt[2] += (uint64_t)(w->K - 1);
    w->robots[(size_t)other].cnt[3] += (uint64_t)(w->K - 1);
    if (w->p.enable_mask & 2u) { c.cnt[2] = (uint64_t)(w->K - 1); c.cnt[3] = (uint64_t)(w->K - 1); }
    const bool keyless = !(w->p.enable_mask & 2u);  // created switched off: the two inbox-filling messages are dropped
    for (int &nd : c.node) {  // add_factor, ascending i
        Robot &ow = w->robots[(size_t)owner];
        nd = ow.alloc_node();
        if (ow.slot_uses.size() <= (size_t)nd) ow.slot_uses.resize((size_t)nd + 1, 0);
        const uint32_t u = ++ow.slot_uses[(size_t)nd];
        c.updates_per_sweep += u;
        if (keyless) { c.keys.push_back(0); c.uses.push_back(u); }
    }
    if (keyless) w->n_keyless++;
    c.node_first = c.node.front();
    c.node_last = c.node.back();
    w->conn_hot.push_back(mgx_world::ConnHot{c.owner, c.other, c.node_first, c.node_last, c.first_number, -1, 1});
    w->conns.push_back(std::move(c));
    if (w->cidx.valid && w->cidx.in.size() == w->robots.size()) conn_index_add(w, (int32_t)w->conn_hot.size() - 1);
    else w->cidx.valid = false;
    w->conns_dirty = true;
    return MGX_OK;
}

static int ir_disconnect(mgx_world *w, int32_t a, int32_t b) {
    if (!w || a < 0 || b < 0 || (size_t)a >= w->robots.size() || (size_t)b >= w->robots.size() || a == b)
        return fail(MGX_ERR_INVALID, "bad robot ids");
    flush_counts(w);  // the deleted factors take their counts with them (factorgraph.rs:876-890)
    // delete_interrobot_factors_connected_to on both graphs (factorgraph.rs:380-436): the node
    // slots are vacated in ascending index order
    for (int side = 0; side < 2; side++) {
        const int self = side ? b : a, other = side ? a : b;
        std::vector<int> gone;
        for (const IrConn &c : w->conns)
            if (c.owner == self && c.other == other) gone.insert(gone.end(), c.node.begin(), c.node.end());
        std::sort(gone.begin(), gone.end());
        std::vector<int> &fr = w->robots[(size_t)self].free_nodes;
        fr.insert(fr.end(), gone.begin(), gone.end());
    }
    w->cidx.valid = false;  // (the list closes up: every index behind the holes moves)
    w->conns.erase(std::remove_if(w->conns.begin(), w->conns.end(),
                                  [&](const IrConn &c) { return (c.owner == a && c.other == b) || (c.owner == b && c.other == a); }),
                   w->conns.end());
    w->conn_hot.erase(std::remove_if(w->conn_hot.begin(), w->conn_hot.end(),
                                     [&](const mgx_world::ConnHot &c) { return (c.owner == a && c.other == b) || (c.owner == b && c.other == a); }),
                      w->conn_hot.end());
    if (w->n_keyless > 0) {  // some of them may just have gone
        w->n_keyless = 0;
        for (const IrConn &c : w->conns) w->n_keyless += c.keys.empty() ? 0 : 1;
    }
    w->conns_dirty = true;  // the surviving connections' state stays on the device
    return MGX_OK;
}

// Several (a, b) deletions in one sweep over the connections (a topology pass deletes dozens):
// same effect as ir_disconnect(a, b) for each pair in order.
// the connections listed by owner (what a batch of deletions looks its pairs up in)
static void ir_disconnect_batch(mgx_world *w, const std::vector<std::pair<int, int>> &pairs) {
    if (pairs.empty()) return;
    StageTimer tm("ir_disconnect_batch");
    flush_counts(w, true);
    tm.lap("flush_counts");
    conn_index_ensure(w);  // (who owns what: the index' `out` lists)
    // (scratch kept with the world: a topology pass comes through here every tick)
    std::vector<uint8_t> &dead = w->scratch_dead;
    std::vector<int32_t> &dead_list = w->scratch_dead_list;
    std::vector<int> &gone = w->scratch_gone;
    dead.assign(w->conns.size(), 0);
    dead_list.clear();
    for (const auto &pr : pairs)
        for (int side = 0; side < 2; side++) {
            const int self = side ? pr.second : pr.first, other = side ? pr.first : pr.second;
            gone.clear();  // node slots are vacated in ascending index order (factorgraph.rs:380-436)
            for (const int32_t ci : w->cidx.out[(size_t)self]) {
                if (dead[(size_t)ci] || w->conn_hot[(size_t)ci].other != other) continue;  // (the 16-byte mirror first: a connection is 168 bytes and four vectors)
                const IrConn &c = w->conns[(size_t)ci];
                dead[(size_t)ci] = 1;
                dead_list.push_back(ci);
                gone.insert(gone.end(), c.node.begin(), c.node.end());
            }
            std::sort(gone.begin(), gone.end());
            std::vector<int> &fr = w->robots[(size_t)self].free_nodes;
            fr.insert(fr.end(), gone.begin(), gone.end());
        }
    for (const int32_t ci : dead_list) {
        settle_conn(w, w->conns[(size_t)ci]);  // (what it delivered to its target stays in that robot's counters; its own go with it)
        conn_index_drop(w, ci);
    }
    // the list's order carries no meaning (inbox order comes from order keys and node slots, build_incoming): the last
    // survivors fill the holes
    {
        size_t lo = 0, hi = w->conns.size();
        auto keep_storage = [&](IrConn &c) {  // (for the connections the pass creates next: ir_connect)
            if (w->pool_edges.size() < 4096) { w->pool_edges.push_back(std::move(c.edges)); w->pool_nodes.push_back(std::move(c.node)); }
        };
        for (;;) {
            while (lo < hi && !dead[lo]) lo++;
            while (hi > lo && dead[hi - 1]) { keep_storage(w->conns[hi - 1]); hi--; }
            if (lo >= hi) break;
            keep_storage(w->conns[lo]);
            w->conns[lo] = std::move(w->conns[hi - 1]);  // dead[lo], alive[hi - 1]
            w->conn_hot[lo] = w->conn_hot[hi - 1];
            conn_index_moved(w, (int32_t)(hi - 1), (int32_t)lo);
            dead[lo] = 0;
            hi--;
        }
        w->conns.resize(hi);
        w->conn_hot.resize(hi);
    }
    tm.lap("connection list");
    if (w->n_keyless > 0) {  // some of them may just have gone
        w->n_keyless = 0;
        for (const IrConn &c : w->conns) w->n_keyless += c.keys.empty() ? 0 : 1;
    }
    w->conns_dirty = true;
}

// Entity despawn (robot.rs:2172 + despawn_entity_after): the graph leaves every Bevy query, so it
// is never iterated again and whatever is addressed to it is dropped (robot.rs:1815,1844: the
// `query.get_mut` fails) — the same dataflow as idle with the antenna off, for good.  The other
// robots drop their factors towards it in the following topology passes.
int mgx_robot_remove(mgx_world *w, int32_t robot) {
    MGX_ENTER(w);
    if (!w || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id");
    Robot &rb = w->robots[(size_t)robot];
    if (rb.removed) return fail(MGX_ERR_STATE, "robot %d already removed", robot);
    flush_counts(w);
    rb.removed = true;
    w->sets.removed[(size_t)robot] = 1;
    rb.idle = 1;
    rb.antenna = 0;
    w->sets.cnt[(size_t)robot] = 0;
    w->search.sets_touched();
    w->flags_dirty = true;
    w->mission.alive_dirty = true;
    return MGX_OK;
}

// FactorGraph::change_factor_enabled for every graph (factorgraph.rs:1529-1539, ui/settings.rs:491-496).
// Disabling is exact as it stands: a disabled factor is never updated (its last message stays in the
// variable's inbox and keeps being summed, factorgraph.rs:695,734) and drops whatever is sent to it
// (FactorNode::receive_message_from returns early, factor/mod.rs:307-310) while change_prior still
// empties the variables' inboxes (variable.rs:224-227); the counters stop counting it.  Re-enabling a
// kind that has missed deliveries would need the inbox its factors froze with (the engine derives factor
// inboxes from the variables' current snapshots, DESIGN.md §3) and is refused with MGX_ERR_STATE.
static int ensure_frozen(mgx_world *w) {
    if (w->frozen_live) return MGX_OK;
    const size_t RL = (size_t)std::max(w->d.R_local, 1);
    std::vector<double> z((size_t)frozen_words(w->K) * RL, 0.0);
    std::vector<uint8_t> zf((size_t)(4 * w->K - 6) * RL, 0), zb(RL, 0);
    for (int dr = 0; dr < w->d.R_local; dr++)  // (robots that joined while a kind was off since the world began)
        nokey_flags(w->robots[(size_t)w->robot_of[(size_t)dr]].nokey, w->K, &zf[(size_t)(4 * w->K - 6) * (size_t)dr]);
    HIP_TRY(w->frozen_buf.upload(z, w->stream));
    HIP_TRY(w->frozen_flag_buf.upload(zf, w->stream));
    HIP_TRY(w->thaw_buf.upload(zb, w->stream));
    HIP_TRY(w->skip0_buf.upload(zb, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->frozen_live = true;
    w->d.frozen = w->frozen_buf.p; w->d.frozen_flag = w->frozen_flag_buf.p; w->d.thaw = w->thaw_buf.p;
    return MGX_OK;
}

int mgx_set_enabled(mgx_world *w, uint32_t kind_mask) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (kind_mask & ~15u) return fail(MGX_ERR_INVALID, "unknown factor kind bits 0x%x", kind_mask);
    const uint32_t on = kind_mask & ~w->p.enable_mask, off = w->p.enable_mask & ~kind_mask;
    if (kind_mask == w->p.enable_mask) return MGX_OK;
    if (w->gkinds.masked())
        return fail(MGX_ERR_STATE, "mgx_set_enabled on a world whose groups have enabled kinds or sigmas of their own (mgx_set_group_enabled, mgx_set_group_sigmas): "
                                   "freeze and thaw are world-wide");
    flush_counts(w);  // what was logged so far was sent under the old flags
    // Internal kinds (dynamic, obstacle, tracking): a factor switched off keeps the inbox it has now and
    // resumes from it when it is switched on again (FactorNode::receive_message_from drops everything in
    // between, factor/mod.rs:307-310).  The engine derives factor inboxes from the variables' snapshots, so
    // the inboxes are materialised here (k_freeze) and consumed by k_thaw in front of the first factor sweep.
    const uint32_t off_int = off & 13u, thaw_int = on & 13u & w->stale_kinds;
    if ((off_int || thaw_int) && !w->robots.empty()) {
        int rc = commit(w);  // the device holds the state the inboxes are derived from
        if (rc != MGX_OK) return rc;
        rc = ensure_frozen(w);
        if (rc != MGX_OK) return rc;
        if (off_int) {
            HIP_TRY(launch_freeze(w->d, off_int, w->stream));
            HIP_TRY(launch_or_bytes(w->thaw_buf.p, w->d.R_local, (uint8_t)~off_int, 0, w->stream));  // off again: nothing to thaw
        }
        if (thaw_int) {
            HIP_TRY(launch_or_bytes(w->thaw_buf.p, w->d.R_local, 0xff, (uint8_t)thaw_int, w->stream));
            w->thaw_kinds |= thaw_int;
            w->d.skip0 = w->skip0_buf.p;
        }
    }
    // Inter-robot factors: F_AB's inbox entry from A's variable is what that variable last sent to its own
    // factors; it is kept per variable when the kind goes off (k_ir_freeze) and used by k_thaw_ir, in front of
    // launches with an external factor sweep, for as long as the variable has not delivered again.
    if (((off & 2u) || ((on & 2u) & w->stale_kinds)) && !w->robots.empty()) {
        int rc = commit(w);
        if (rc != MGX_OK) return rc;
        // A sharded world with the exchange inside the engine: the records frozen here and the delivery counts thawed against
        // include the ghosts', which must be their owners' CURRENT ones — the plain copies are as old as the last exchange
        // kernel (resident launches never touch them: the ghosts' records travel inside those).  Every rank switches
        // together (ShardedWorld.set_enabled), so the exchange is one all ranks take part in.
        if (w->direct.connected) {
            rc = direct_exchange(w);
            if (rc != MGX_OK) return rc;
        } else if (w->rccl.connected) {
            rc = rccl_exchange(w);
            if (rc != MGX_OK) return rc;
        }
        const size_t V = (size_t)w->d.V;
        if (!w->ir_frozen_live) {  // never frozen before: nothing was ever received (kind off since the world began)
            std::vector<double> z(24 * V, 0.0);
            std::vector<uint32_t> ze(V, 0);
            HIP_TRY(w->ir_frozen_snap_buf.upload(z, w->stream));
            HIP_TRY(w->ir_frozen_epoch_buf.upload(ze, w->stream));
            HIP_TRY(w->ir_thaw_epoch_buf.upload(ze, w->stream));
            HIP_TRY(hipStreamSynchronize(w->stream));
            w->ir_frozen_live = true;
        }
        if (off & 2u) {
            HIP_TRY(launch_ir_freeze(w->d, w->ir_frozen_snap_buf.p, w->ir_frozen_epoch_buf.p, w->stream));
            w->ir_thaw_active = false;
            w->d.ir_frozen_snap = nullptr; w->d.ir_frozen_epoch = nullptr; w->d.ir_thaw_epoch = nullptr;
            w->flags_dirty = true;
        } else {
            HIP_TRY(hipMemcpyAsync(w->ir_thaw_epoch_buf.p, w->d.snap_epoch[w->d.cur], sizeof(uint32_t) * V, hipMemcpyDeviceToDevice, w->stream));
            w->ir_thaw_active = true;
            w->d.ir_frozen_snap = w->ir_frozen_snap_buf.p; w->d.ir_frozen_epoch = w->ir_frozen_epoch_buf.p;
            w->d.ir_thaw_epoch = w->ir_thaw_epoch_buf.p;
        }
    }
    w->p.enable_mask = kind_mask;
    w->d.enable = kind_mask;
    if (kind_mask & 8u) { w->trk_ever_on = true; w->d.trk_cols = 1; }
    w->stale_kinds &= ~kind_mask;
    return MGX_OK;
}

// The enabled kinds of ONE robot group (include/mgx.h, ROBOT GROUPS): fixed before the group's first robot joins, so a factor of a
// switched-off kind is off from its creation — nothing to freeze, nothing to thaw, no inbox keys ever.  Only the internal kinds
// may differ from the world's; a mask equal to the world's is no mask at all (the group follows the world, as if never set).
int mgx_set_group_enabled(mgx_world *w, uint32_t group, uint32_t kind_mask) {
    // (what the arguments alone say comes first: it needs no world and no device)
    if (kind_mask & ~15u) return fail(MGX_ERR_INVALID, "unknown factor kind bits 0x%x", kind_mask);
    if (group >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "group %u is not below MGX_GROUPS_MAX (%u)", group, MGX_GROUPS_MAX);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    MGX_ENTER(w);
    mgx_world::GroupKinds &gk = w->gkinds;
    if ((kind_mask ^ w->p.enable_mask) & 2u)
        return fail(MGX_ERR_INVALID, "group %u: the inter-robot kind (bit 2) must equal the world's (%s): residency, keyless factors and the inter-robot "
                                     "freeze are world-wide", group, (w->p.enable_mask & 2u) ? "on" : "off");
    if (group < gk.populated.size() && gk.populated[group])
        return fail(MGX_ERR_STATE, "group %u has had robots: a group's enabled kinds are fixed before its first robot is added", group);
    if (w->frozen_live || w->ir_frozen_live || w->thaw_kinds || w->ir_thaw_active || w->n_keyless > 0)
        return fail(MGX_ERR_STATE, "enabled kinds per group on a world that has switched a factor kind (mgx_set_enabled): freeze and thaw are world-wide");
    if (w->obs.n_ghosts || w->xres.connected || w->direct.connected || w->rccl.connected)
        return fail(MGX_ERR_STATE, "enabled kinds per group on a sharded world: ghosts have no group");
    if (gk.has.size() <= group) { gk.has.resize((size_t)group + 1, 0); gk.mask.resize((size_t)group + 1, 0u); }
    const bool own = kind_mask != w->p.enable_mask;
    gk.n_masked += (own ? 1u : 0u) - (gk.has[group] ? 1u : 0u);
    gk.has[group] = own ? 1 : 0;
    gk.mask[group] = kind_mask;
    if (own && (kind_mask & 8u)) { w->trk_ever_on = true; w->d.trk_cols = 1; }  // (on if ANY group has tracking on)
    return MGX_OK;
}
int mgx_get_group_enabled(mgx_world *w, uint32_t group, uint32_t *kind_mask) {
    if (group >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "group %u is not below MGX_GROUPS_MAX (%u)", group, MGX_GROUPS_MAX);
    if (!w || !kind_mask) return fail(MGX_ERR_INVALID, "null argument");
    *kind_mask = w->kinds_of_group(group);
    return MGX_OK;
}
int mgx_group_enabled_stats(mgx_world *w, uint64_t *masked_plans, uint64_t *masked_launches) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (masked_plans) *masked_plans = w->gkinds.masked_plans;
    if (masked_launches) *masked_launches = w->gkinds.masked_launches;
    return MGX_OK;
}
// The factor sigmas of ONE robot group (include/mgx.h, ROBOT GROUPS), under the rules of mgx_set_group_enabled: fixed before the
// group's first robot joins, a set equal to the world's is none at all.  sigma_dynamics goes into the dyn_m of the group's robots
// as they are added (mgx_robot_add); the other three reach the kernels as 1 / sigma^2 by group id (ensure_group_kinds).
int mgx_set_group_sigmas(mgx_world *w, uint32_t group, const mgx_group_sigmas *s) {
    // (what the arguments alone say comes first: it needs no world and no device)
    if (!s) return fail(MGX_ERR_INVALID, "null sigmas");
    for (const double v : {s->dynamics, s->interrobot, s->obstacle, s->tracking})
        if (!(std::isfinite(v) && v > 0)) return fail(MGX_ERR_INVALID, "sigmas must be finite and positive");
    if (group >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "group %u is not below MGX_GROUPS_MAX (%u)", group, MGX_GROUPS_MAX);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    MGX_ENTER(w);
    mgx_world::GroupKinds &gk = w->gkinds;
    if (group < gk.populated.size() && gk.populated[group])
        return fail(MGX_ERR_STATE, "group %u has had robots: a group's sigmas are fixed before its first robot is added", group);
    if (w->frozen_live || w->ir_frozen_live || w->thaw_kinds || w->ir_thaw_active || w->n_keyless > 0)
        return fail(MGX_ERR_STATE, "sigmas per group on a world that has switched a factor kind (mgx_set_enabled): freeze and thaw evaluate factors with the world's sigmas");
    if (w->obs.n_ghosts || w->xres.connected || w->direct.connected || w->rccl.connected)
        return fail(MGX_ERR_STATE, "sigmas per group on a sharded world: ghosts have no group");
    if (gk.sig_has.size() <= group) { gk.sig_has.resize((size_t)group + 1, 0); gk.sig.resize((size_t)group + 1, mgx_group_sigmas{0.0, 0.0, 0.0, 0.0}); }
    const bool own = s->dynamics != w->p.sigma_dynamics || s->interrobot != w->p.sigma_interrobot || s->obstacle != w->p.sigma_obstacle ||
                     s->tracking != w->p.sigma_tracking;
    gk.n_sigma += (own ? 1u : 0u) - (gk.sig_has[group] ? 1u : 0u);
    gk.sig_has[group] = own ? 1 : 0;
    gk.sig[group] = *s;
    return MGX_OK;
}
int mgx_get_group_sigmas(mgx_world *w, uint32_t group, mgx_group_sigmas *out) {
    if (group >= MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "group %u is not below MGX_GROUPS_MAX (%u)", group, MGX_GROUPS_MAX);
    if (!w || !out) return fail(MGX_ERR_INVALID, "null argument");
    *out = w->sigmas_of_group(group);
    return MGX_OK;
}
// A masked world's equal schedules as resident launches of the masked form (include/mgx.h, ROBOT GROUPS).  A switch of the world,
// off by default; like every call that is no schedule it ends a lingering launch first, so no launch outlives the form it was
// chosen under.
int mgx_set_group_resident(mgx_world *w, int32_t enabled) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    MGX_ENTER(w);
    MGX_CONFIRM(w);  // (a launch the census declined is run again under the setting it was issued with)
    w->gkinds.resident = enabled != 0;
    return MGX_OK;
}
int mgx_group_resident_stats(mgx_world *w, uint64_t *launches, uint64_t *posts, uint64_t *fallbacks) {
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (launches) *launches = w->gkinds.res_launches;
    if (posts) *posts = w->gkinds.res_posts;
    if (fallbacks) *fallbacks = w->gkinds.res_fallbacks;
    return MGX_OK;
}

// FactorGraph::update_inter_robot_safety_distance_multiplier for every graph + the config entry new factors read
// (factorgraph.rs:892-910, interrobot.rs:87-89, ui/settings.rs:586-590).  The multiplier lives in w->p: every record the host
// forms later (ir_connect -> retopo's slot records, commit's edge records) takes it from there.  The records the DEVICE holds
// are rewritten in place by k_set_safety: the edge records of the layout there now, and — where the next topology pass will read
// them (rinc.all: it will not, every robot sends its piece) — the slot records.  A world whose device arrays are about to be
// laid out again anyway (dirty, or never laid out) needs nothing but the scalar.  No pull, no commit, no upload.
int mgx_set_safety_multiplier(mgx_world *w, double multiplier) {
    MGX_ENTER(w);
    if (!std::isfinite(multiplier) || !(multiplier > 0)) return fail(MGX_ERR_INVALID, "safety multiplier must be finite and > 0");
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    // (a resident launch the census declined is run again first: its schedule was issued under the old distance)
    MGX_CONFIRM(w);
    w->p.safety_multiplier = multiplier;
    // (robots that only wait to be appended have no records on the device yet: theirs are formed from w->p later)
    if (w->relayout || !w->dev_valid || w->dev_in_ptr.empty()) return MGX_OK;
    const size_t n_slots = (size_t)w->dev_in_ptr.back(), n_edges = n_slots * (size_t)(w->K - 1);
    if (n_edges == 0) return MGX_OK;
    if (n_edges > w->ir_rec.n || (size_t)w->d.R_total > w->radius_dev.n)
        return fail(MGX_ERR_STATE, "internal: %zu edges on the device, %zu records, %zu radii for %d robots", n_edges, w->ir_rec.n, w->radius_dev.n, w->d.R_total);
    const bool slots_live = !w->rinc.all && n_slots <= w->slot_recs.n;
    if (!slots_live) w->rinc.all = true;  // (no slot records there to rewrite: the next pass sends everybody's, with the new distance)
    HIP_TRY(launch_set_safety((int)n_edges, w->ir_rec.p, slots_live ? (int)n_slots : 0, w->slot_recs.p, w->d.R_total, w->radius_dev.p,
                              multiplier, w->stream));
    return MGX_OK;
}

int mgx_set_antenna(mgx_world *w, int32_t robot, int32_t active) {
    MGX_ENTER(w);
    if (!w || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id");
    if (w->robots[(size_t)robot].removed) return fail(MGX_ERR_STATE, "robot %d was removed", robot);
    if (w->robots[(size_t)robot].antenna != (active ? 1 : 0)) flush_counts(w);
    w->robots[(size_t)robot].antenna = active ? 1 : 0;
    w->flags_dirty = true;
    return MGX_OK;
}
int mgx_set_idle(mgx_world *w, int32_t robot, int32_t idle) {
    MGX_ENTER(w);
    if (!w || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id");
    if (w->robots[(size_t)robot].removed) return fail(MGX_ERR_STATE, "robot %d was removed", robot);
    if (w->robots[(size_t)robot].idle != (idle ? 1 : 0)) flush_counts(w);
    w->robots[(size_t)robot].idle = idle ? 1 : 0;
    w->flags_dirty = true;
    return MGX_OK;
}

int mgx_get_idle(mgx_world *w, int32_t robot, int32_t *idle) {
    if (!w || !idle || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    *idle = w->robots[(size_t)robot].idle ? 1 : 0;
    return MGX_OK;
}

int mgx_set_antennas(mgx_world *w, uint32_t n, const int32_t *robots, const uint8_t *active) {
    MGX_ENTER(w);
    if (!w || (n && (!robots || !active))) return fail(MGX_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < n; i++) {
        if (robots[i] < 0 || (size_t)robots[i] >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id");
        if (w->robots[(size_t)robots[i]].removed) return fail(MGX_ERR_STATE, "robot %d was removed", robots[i]);
    }
    for (uint32_t i = 0; i < n; i++)
        if (w->robots[(size_t)robots[i]].antenna != (active[i] ? 1 : 0)) { flush_counts(w); break; }
    for (uint32_t i = 0; i < n; i++) w->robots[(size_t)robots[i]].antenna = active[i] ? 1 : 0;
    w->flags_dirty = true;
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
