// mgx_world_commit.inc — commit (host mirror -> device arrays), the connection index, the incoming tables, retopo (edge tables rebuilt on the device).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// ---- commit: host mirror -> device arrays ---------------------------------------------------------
static int upload_flags(mgx_world *w) {
    // antenna[R] | idle[R] staged in one pinned block and moved by a copy kernel, the edge gates
    // derived from them on the device: no blocking copy, no synchronisation (update_failed_comms
    // rewrites every antenna each tick)
    const size_t R = w->robot_of.size(), NE = (size_t)std::max(w->d.NI, 1);
    void *hp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(2 * R, &hp, &slot));
    uint8_t *an = (uint8_t *)hp, *id = an + R;
    for (size_t dr = 0; dr < R; dr++) {
        an[dr] = w->robots[(size_t)w->robot_of[dr]].antenna;
        id[dr] = w->robots[(size_t)w->robot_of[dr]].idle;
    }
    HIP_TRY(w->antenna.reserve(std::max(R, (size_t)w->R_cap)));  // (a reserved world's head-room: k_append_robots writes the bytes of the robots that join)
    HIP_TRY(w->idle.reserve(std::max(R, (size_t)w->R_cap)));
    HIP_TRY(w->ir_gate.reserve(NE));
    void *dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    const uint8_t *src = (const uint8_t *)dp;
    HIP_TRY(launch_copy_bytes(w->antenna.p, src, R, w->stream));
    HIP_TRY(launch_copy_bytes(w->idle.p, src + R, R, w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    // edge gates: the owner of the edge is on air
    const int n_edges = w->dev_in_ptr.empty() ? 0 : w->dev_in_ptr.back() * (w->K - 1);
    if (n_edges == 0) HIP_TRY(hipMemsetAsync(w->ir_gate.p, 0, NE, w->stream));
    HIP_TRY(launch_edge_gates(n_edges, w->ir_rec.p, w->antenna.p, w->idle.p, w->ir_gate.p, w->stream));
    w->d.antenna = w->antenna.p;
    w->d.idle = w->idle.p;
    w->d.ir_gate = w->ir_gate.p;
    w->flags_dirty = false;
    return MGX_OK;
}

static size_t edge_index(const std::vector<int32_t> &in_ptr, int K, int r, int j, int slot) {
    const int n_in = in_ptr[(size_t)r + 1] - in_ptr[(size_t)r];
    return (size_t)(K - 1) * (size_t)in_ptr[(size_t)r] + (size_t)j * (size_t)n_in + (size_t)(slot - in_ptr[(size_t)r]);
}
// ---- the connection index (ConnIndex) ------------------------------------------------------------------------------------------
static bool conn_before(const mgx_world *w, int32_t a, int32_t b, bool *interleaved) {  // the inbox order of two connections of one target
    const mgx_world::ConnHot &ca = w->conn_hot[(size_t)a], &cb = w->conn_hot[(size_t)b];
    const uint64_t ka = w->sets.keys[(size_t)ca.owner], kb = w->sets.keys[(size_t)cb.owner];
    if (ka != kb) return ka < kb;
    if ((ca.node_first < cb.node_first) != (ca.node_last < cb.node_last)) *interleaved = true;
    return ca.node_first < cb.node_first;
}
static void conn_index_add(mgx_world *w, int32_t ci) {
    ConnIndex &x = w->cidx;
    const mgx_world::ConnHot &c = w->conn_hot[(size_t)ci];
    std::vector<int32_t> &lst = x.in[(size_t)c.other];
    size_t at = lst.size();
    while (at > 0 && conn_before(w, ci, lst[at - 1], &x.interleaved)) at--;
    lst.insert(lst.begin() + (long)at, ci);
    x.out[(size_t)c.owner].push_back(ci);
    w->rinc.mark_in(c.other);  // (what retopo sends of this change: the target's slot list, both ends' peer rows)
    w->rinc.mark_peer(c.other);
    w->rinc.mark_peer(c.owner);
}
static void conn_index_rebuild(mgx_world *w) {
    ConnIndex &x = w->cidx;
    const size_t n = w->robots.size();
    x.in.assign(n, {});
    x.out.assign(n, {});
    x.interleaved = false;
    for (size_t ci = 0; ci < w->conn_hot.size(); ci++) conn_index_add(w, (int32_t)ci);
    x.valid = true;
    w->rinc.all = true;  // (whatever happened to the list while the index was not told: every robot's tables go out again)
}
static void conn_index_ensure(mgx_world *w) {
    if (!w->cidx.valid || w->cidx.in.size() != w->robots.size()) conn_index_rebuild(w);
}
static void conn_index_drop(mgx_world *w, int32_t ci) {  // connection ci leaves the list
    ConnIndex &x = w->cidx;
    const mgx_world::ConnHot &c = w->conn_hot[(size_t)ci];
    std::vector<int32_t> &a = x.in[(size_t)c.other], &b = x.out[(size_t)c.owner];
    a.erase(std::find(a.begin(), a.end(), ci));
    b.erase(std::find(b.begin(), b.end(), ci));
    w->rinc.mark_in(c.other);
    w->rinc.mark_peer(c.other);
    w->rinc.mark_peer(c.owner);
}
static void conn_index_moved(mgx_world *w, int32_t from, int32_t to) {  // connection `from` now sits at `to` (conn_hot[to] holds it already)
    ConnIndex &x = w->cidx;
    const mgx_world::ConnHot &c = w->conn_hot[(size_t)to];
    std::vector<int32_t> &a = x.in[(size_t)c.other], &b = x.out[(size_t)c.owner];
    *std::find(a.begin(), a.end(), from) = to;
    *std::find(b.begin(), b.end(), from) = to;
}
static void build_incoming(const mgx_world *w, int R_local, Incoming &t, bool want_peers = false) {
    const int K = w->K;
    const uint64_t *key = w->sets.keys.data();  // (compact copies of the robots' order keys and ghost flags: a Robot is a dozen vectors wide)
    const uint8_t *ghost = w->sets.ghost.data();
    const int32_t *dev_of = w->dev_of.data();
    const mgx_world::ConnHot *conns = w->conn_hot.data();  // (owner, other, first and last node slot of every connection)
    const size_t n_conns = w->conns.size(), R = (size_t)R_local;
    t.in_ptr.assign(R + 1, 0);
    t.mid.assign((size_t)std::max(R_local, 1), 0);
    int32_t *pp = nullptr;
    t.blocks_ok = true;
    t.peers.clear();
    if (want_peers) {
        t.peers.assign(R + 1 + std::max<size_t>(2 * n_conns, 1), 0);
        pp = t.peers.data();
    }
    for (size_t ci = 0; ci < n_conns; ci++) {
        const size_t o = (size_t)dev_of[(size_t)conns[ci].owner], tt = (size_t)dev_of[(size_t)conns[ci].other];
        if (!ghost[(size_t)conns[ci].other]) t.in_ptr[tt + 1]++;  // ghost target: another rank's
        if (pp) {
            if (o < R) pp[o + 1]++;
            if (tt < R) pp[tt + 1]++;
        }
    }
    for (size_t r = 0; r < R; r++) t.in_ptr[r + 1] += t.in_ptr[r];
    t.in_list.assign((size_t)t.in_ptr[R], 0);
    std::vector<int32_t> &fill = t.fill, &pfill = t.pfill;
    fill.assign(t.in_ptr.begin(), t.in_ptr.end() - 1);
    if (pp) {
        for (size_t r = 0; r < R; r++) pp[r + 1] += pp[r];
        pfill.assign(pp, pp + R);
    }
    int32_t *pidx = pp ? pp + R + 1 : nullptr;
    for (size_t ci = 0; ci < n_conns; ci++) {
        const int o = dev_of[(size_t)conns[ci].owner], tt = dev_of[(size_t)conns[ci].other];
        if (!ghost[(size_t)conns[ci].other]) t.in_list[(size_t)fill[(size_t)tt]++] = (int32_t)ci;
        if (pp) {
            if ((size_t)o < R) pidx[(size_t)pfill[(size_t)o]++] = tt;
            if ((size_t)tt < R) pidx[(size_t)pfill[(size_t)tt]++] = o;
        }
    }
    if (pp) t.peers.resize(R + 1 + (size_t)std::max(pp[R], 1));
    t.ir_max_edges = 0;
    for (int r = 0; r < R_local; r++) {
        int32_t *seg = t.in_list.data() + t.in_ptr[(size_t)r];
        const int n_in = t.in_ptr[(size_t)r + 1] - t.in_ptr[(size_t)r];
        auto before = [&](int32_t a, int32_t b) {
            const mgx_world::ConnHot &ca = conns[(size_t)a], &cb = conns[(size_t)b];
            const uint64_t ka = key[(size_t)ca.owner], kb = key[(size_t)cb.owner];
            if (ka != kb) return ka < kb;
            if ((ca.node_first < cb.node_first) != (ca.node_last < cb.node_last)) t.blocks_ok = false;
            return ca.node_first < cb.node_first;
        };
        for (int a = 1; a < n_in; a++) {  // insertion sort: a handful of connections per robot
            const int32_t v = seg[a];
            int b = a;
            while (b > 0 && before(v, seg[b - 1])) { seg[b] = seg[b - 1]; b--; }
            seg[b] = v;
        }
        const uint64_t own_key = key[(size_t)w->robot_of[(size_t)r]];
        int mid = n_in;  // first connection whose owner has a HIGHER key than the target
        for (int q = n_in - 1; q >= 0; q--)
            if (key[(size_t)conns[(size_t)seg[q]].owner] > own_key) mid = q;
        t.mid[(size_t)r] = mid;
        t.ir_max_edges = std::max(t.ir_max_edges, n_in * (K - 1));
    }
}
// the constant record of edge (connection c, variable j + 1); `created` is the caller's
static IrEdgeRec edge_record(const mgx_world *w, const IrConn &c, int j) {
    const Robot &ow = w->robots[(size_t)c.owner], &ot = w->robots[(size_t)c.other];
    IrEdgeRec rec;
    rec.src_var = w->dev_of[(size_t)c.owner] * w->K + j + 1;
    rec.src_robot = w->dev_of[(size_t)c.owner];
    rec.created = 0;
    rec.dst = (int32_t)(j + 1) | ((ot.order_key > ow.order_key) ? (1 << 16) : 0);
    rec.d_safe = w->p.safety_multiplier * ow.radius;                      // interrobot.rs:64
    rec.offset = (double)1e-6f * (double)(c.first_number + (uint64_t)j);  // interrobot.rs:52,75
    return rec;
}

static int upload_flags(mgx_world *w);

// Only inter-robot connections changed (create_ / delete_interrobot_factors between two ticks):
// the edge tables are rebuilt on the device from the old ones — surviving edges keep their state
// (message, response mean, creation epoch), new edges are initialised from the owner's current
// delivery count and the target's current belief mean (robot.rs:1549-1585) — without moving any
// robot state between host and device.  What travels are DIFFERENCES (RetopoBlock): the slot ranges of all robots (a prefix sum
// over the index' list lengths), and slot records, key split and peer row only of the robots whose lists the index saw change
// since the last pass (a world that follows its topology changes a few dozen of its thousands of connections per tick); the
// per-edge arrays are laid out by k_retopo_robots, which keeps the slot records of everybody else on the device.
static int retopo(mgx_world *w) {
    const int K = w->K, K1 = K - 1, R_local = w->d.R_local;
    const size_t R = (size_t)R_local;
    StageTimer tm("retopo");
    mgx_world::RetopoInc &ri = w->rinc;
    // (a world whose schedules can run as resident launches gets that kernel's peer table in the same block)
    const bool want_peers = (w->d.R_total == w->d.R_local || w->xres.connected) && (w->p.enable_mask & 2u) && w->res.sweep_flag_buf.p;
    conn_index_ensure(w);
    const ConnIndex &x = w->cidx;
    if (x.interleaved) return fail(MGX_ERR_STATE, "internal: node slots of two connections interleave");
    mgx_world::ConnHot *hot = w->conn_hot.data();  // (positions, numbers and the "fresh" marks sit in the connections' mirror)
    const int32_t *dev_of = w->dev_of.data();
    const uint64_t *key = w->sets.keys.data();
    if (ri.mid.size() != R) {
        ri.mid.assign(R, 0);
        ri.all = true;
    }
    // slot ranges of everybody
    ri.in_ptr.resize(R + 1);
    ri.in_ptr[0] = 0;
    int ir_max_edges = 0;
    for (size_t r = 0; r < R; r++) {
        const int n_in = (int)x.in[(size_t)w->robot_of[r]].size();
        ri.in_ptr[r + 1] = ri.in_ptr[r] + n_in;
        ir_max_edges = std::max(ir_max_edges, n_in * K1);
    }
    const size_t n_slots = (size_t)ri.in_ptr[R], NI = n_slots * (size_t)K1, NIs = std::max<size_t>(NI, 1);
    auto local_of = [&](int32_t id) -> long { return ((size_t)id < w->dev_of.size() && (size_t)dev_of[(size_t)id] < R) ? (long)dev_of[(size_t)id] : -1; };
    // (the peer table the device holds is only good for the robots it is not told about if it IS the table of the layout being
    // replaced: a world that could not run resident launches a moment ago has none)
    if (want_peers && !w->res.peers_valid) ri.all = true;
    // which robots send their piece: the ones whose incoming list or peer row the index saw change
    ri.mark.assign(std::max<size_t>(R, 1), ri.all ? 1 : 0);
    if (!ri.all) {
        for (const int32_t id : ri.in_changed) { const long r = local_of(id); if (r >= 0) ri.mark[(size_t)r] = 1; }
        for (const int32_t id : ri.peer_changed) { const long r = local_of(id); if (r >= 0) ri.mark[(size_t)r] = 1; }
    }
    auto pad4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    size_t n16 = 0, n_peers = 0;  // the pieces' size in 16-byte units; entries of the new peer table
    for (size_t r = 0; r < R; r++) {
        const size_t id = (size_t)w->robot_of[r];
        const size_t n_in = x.in[id].size(), pc = n_in + x.out[id].size();
        n_peers += pc;
        if (ri.mark[r]) n16 += 2 * n_in + pad4(pc) / 4;
    }
    tm.lap("ranges");
    // ONE pinned block of the argument ring, written in place; ONE kernel reads it over the host link and lays out everything
    // derived — no copies, no synchronisation (the block is released by an event after the kernel)
    const size_t b_hdr = sizeof(RetopoHeader) * (R + 1), b_data = 16 * std::max<size_t>(n16, 1);
    void *hp = nullptr, *dp = nullptr;
    int ring_slot = 0;
    HIP_TRY(w->stage.acquire(b_hdr + b_data, &hp, &ring_slot));
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    RetopoHeader *hdr = (RetopoHeader *)hp;
    char *data = (char *)hp + b_hdr;
    size_t at = 0;   // (16-byte units)
    int32_t pp = 0;
    for (size_t r = 0; r < R; r++) {
        const size_t id = (size_t)w->robot_of[r];
        const std::vector<int32_t> &lst = x.in[id], &out = x.out[id];
        const int n_in = (int)lst.size();
        RetopoHeader &h = hdr[r];
        h.in0 = ri.in_ptr[r];
        h.pp0 = pp;
        pp += want_peers ? n_in + (int)out.size() : 0;
        if (!ri.mark[r]) { h.mid = ri.mid[r]; h.off = -1; continue; }
        // the robot's piece: the slot records of its new list (its connections learn their new positions), its peer row (owners
        // of incoming, targets of outgoing connections: device indices)
        h.off = (int32_t)at;
        IrSlotRec *recs = (IrSlotRec *)(data + 16 * at);
        const uint64_t own_key = key[id];
        int mid = n_in;  // first connection whose owner has a HIGHER key than the target
        for (int q = 0; q < n_in; q++) {
            const int32_t ci = lst[(size_t)q];
            mgx_world::ConnHot &c = hot[(size_t)ci];
            const uint64_t owner_key = key[(size_t)c.owner];
            IrSlotRec &sl = recs[q];
            sl.tgt_robot = (int32_t)r;
            sl.src_robot = dev_of[(size_t)c.owner];
            sl.old_slot = c.dev_q;
            sl.flags = own_key > owner_key ? 1 : 0;
            sl.d_safe = w->p.safety_multiplier * w->sets.radius[(size_t)c.owner];
            sl.first_number = c.first_number;
            c.dev_q = q;  // (from here on the connection's position in the tables being built)
            if (c.has_fresh) {
                for (IrEdge &ed : w->conns[(size_t)ci].edges) ed.fresh = false;
                c.has_fresh = 0;
            }
            if (mid == n_in && owner_key > own_key) mid = q;
        }
        h.mid = ri.mid[r] = mid;
        int32_t *row = (int32_t *)(recs + n_in);
        int n = 0;
        for (const int32_t ci : lst) row[n++] = dev_of[(size_t)hot[(size_t)ci].owner];
        for (const int32_t ci : out) row[n++] = dev_of[(size_t)hot[(size_t)ci].other];
        at += 2 * (size_t)n_in + pad4((size_t)n) / 4;
    }
    hdr[R] = RetopoHeader{ri.in_ptr[R], pp, 0, -1};
    if (at != n16) return fail(MGX_ERR_STATE, "internal: topology block counted %zu units, written %zu", n16, at);
    tm.lap("block");
    static const bool check_index = getenv("MGX_CHECK_INDEX") != nullptr;
    if (check_index) {  // (diagnostics: what the device will hold against the tables of two passes over the connection list)
        Incoming &full = w->retopo_tables;
        build_incoming(w, R_local, full, true);
        bool same = full.in_ptr == ri.in_ptr && full.mid.size() >= R && std::equal(ri.mid.begin(), ri.mid.end(), full.mid.begin()) &&
                    full.ir_max_edges == ir_max_edges && full.blocks_ok;
        for (size_t g = 0; g < full.in_list.size() && same; g++) {
            const mgx_world::ConnHot &c = hot[(size_t)full.in_list[g]];
            same = ri.in_ptr[(size_t)dev_of[(size_t)c.other]] + c.dev_q == (int32_t)g;
        }
        for (size_t r = 0; r < R && same; r++) {  // (a row's order carries no meaning: compared as multisets; the pieces that went out)
            if (hdr[r].off < 0) continue;
            const int n_in = ri.in_ptr[r + 1] - ri.in_ptr[r];
            const int32_t *row = (const int32_t *)(data + 16 * (size_t)hdr[r].off + sizeof(IrSlotRec) * (size_t)n_in);
            std::vector<int32_t> a(full.peers.begin() + (long)(R + 1) + full.peers[r], full.peers.begin() + (long)(R + 1) + full.peers[r + 1]),
                b(row, row + (want_peers ? hdr[r + 1].pp0 - hdr[r].pp0 : (int)a.size()));
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            same = a == b;
        }
        if (!same) return fail(MGX_ERR_STATE, "internal: the connection index and the connection list disagree (MGX_CHECK_INDEX)");
    }
    hipStream_t s = w->stream;
    HIP_TRY(w->slot_recs_b.reserve(n_slots + 1));  // (slot_recs holds the layout being replaced: left alone)
    HIP_TRY(w->in_ptr_dev_b.reserve(std::max(R, (size_t)w->R_cap) + 1));  // (with the head-room of a reserved world: the next "old" ranges, which an append extends)
    HIP_TRY(w->ir_rec_b.reserve(NIs));
    HIP_TRY(w->ir_fv_eta_b.reserve(4 * NIs));
    HIP_TRY(w->ir_fv_lam_b.reserve(16 * NIs));
    HIP_TRY(w->ir_bmu_b.reserve(4 * NIs));
    const bool gates_along = !w->flags_dirty;
    if (gates_along) HIP_TRY(w->ir_gate.reserve(NIs));
    const size_t peer_words = R + 1 + std::max<size_t>(n_peers, 1);
    if (want_peers) HIP_TRY(w->res.peer_ptr_dev_b.reserve(peer_words));
    RetopoBlock blk;
    blk.hdr = (const RetopoHeader *)dp;
    blk.data = (const uint4 *)((const char *)dp + b_hdr);
    HIP_TRY(launch_retopo_robots(w->d, blk, w->in_ptr_dev.p, w->slot_recs.p, w->res.peer_ptr_dev.p, w->in_ptr_dev_b.p, w->slot_recs_b.p,
                                 want_peers ? w->res.peer_ptr_dev_b.p : nullptr, w->ir_var_ptr.p, w->ir_var_mid.p, (int)NIs, w->ir_rec_b.p, w->ir_fv_eta_b.p,
                                 w->ir_fv_lam_b.p, w->ir_bmu_b.p, gates_along ? w->ir_gate.p : nullptr, s));
    HIP_TRY(w->stage.release(ring_slot, s));
    tm.lap("launch");
    w->ir_rec.swap(w->ir_rec_b);
    w->ir_fv_eta.swap(w->ir_fv_eta_b);
    w->ir_fv_lam.swap(w->ir_fv_lam_b);
    w->ir_bmu.swap(w->ir_bmu_b);
    w->in_ptr_dev.swap(w->in_ptr_dev_b);
    w->slot_recs.swap(w->slot_recs_b);
    DevWorld &d = w->d;
    d.NI = (int)NIs;
    d.ir_rec = w->ir_rec.p; d.ir_fv_eta = w->ir_fv_eta.p; d.ir_fv_lam = w->ir_fv_lam.p; d.ir_bmu = w->ir_bmu.p;
    if (ir_max_edges != d.ir_max_edges) w->res.lds_footprint_changed();
    d.ir_max_edges = ir_max_edges;
    w->dev_in_ptr.assign(ri.in_ptr.begin(), ri.in_ptr.end());
    ri.all = false;
    ri.clear_marks();
    w->conns_dirty = false;
    w->res.peers_rebuilt(want_peers, R, d);
    int rc_flags = MGX_OK;  // the gate bytes follow the edges (the robots' own flags only when they changed too)
    if (w->flags_dirty) {
        rc_flags = upload_flags(w);
    } else {
        if (NI == 0) HIP_TRY(hipMemsetAsync(w->ir_gate.p, 0, NIs, s));
        d.ir_gate = w->ir_gate.p;  // (written by k_retopo_robots)
    }
    tm.lap("bookkeeping + gates");
    return rc_flags;
}


// What commit() packs of ONE robot, for both of its paths: the full layout (the world's host arrays: strided tables, stride
// dyn_cs between components) and the append (the robot's record of the staged block: item-major, dyn_is = 16).  Paths, radius,
// iteration count and flags are scalars and spans the callers place themselves.
struct RobotSink {
    double *blob, *snap;  // [BS], [K][24]
    uint32_t *epoch;      // [K]
    double *dyn;          // component c of factor f at dyn[c * dyn_cs + f * dyn_is]
    size_t dyn_cs, dyn_is;
    int32_t *trk_rec;     // [K-2] ...
    float *trk_x, *trk_y;
    double *trk_val;
};
static void pack_robot(const Robot &rb, const RobotSink &o) {
    const int K = rb.K;
    blob_pack(rb, o.blob);
    memcpy(o.snap, rb.snap.data(), 24 * (size_t)K * sizeof(double));
    for (int i = 0; i < K; i++) o.epoch[i] = rb.epoch[i];
    if (rb.ghost) return;
    for (int f = 0; f < K - 1; f++)
        for (int c = 0; c < 16; c++) o.dyn[(size_t)c * o.dyn_cs + (size_t)f * o.dyn_is] = rb.dyn_m[16 * f + c];
    for (int j = 0; j < K - 2; j++) {
        o.trk_rec[j] = rb.trk_record[j];
        o.trk_x[j] = rb.trk_last_pos[2 * j];
        o.trk_y[j] = rb.trk_last_pos[2 * j + 1];
        o.trk_val[j] = rb.trk_last_val[j];
    }
}
constexpr size_t APPEND_PATH_POINTS = 32;  // (path slack per free place of a reserved world, in points, when no robot has a longer path)

// ---- robots that join a laid-out world with head-room: appended on the device ------------------------------------------------
static size_t device_path_points(const mgx_world *w) {  // what the packed path array holds (Robot::path is the truth of paths)
    size_t n = 0;
    for (const int id : w->robot_of) n += w->robots[(size_t)id].path.size() / 2;
    return n;
}
// the packed path array of a reserved world keeps its slack when the paths are packed again (mgx_set_tracking_path, mgx_apply_global_paths)
static size_t path_room_for(const mgx_world *w, size_t floats, size_t longest) {
    const size_t free_places = (size_t)std::max(w->R_cap - w->d.R_local, 0);
    return floats + free_places * std::max<size_t>(longest, 2 * APPEND_PATH_POINTS);
}
// The conditions of mgx_apply_global_paths' in-place form, and room: in the per-robot arrays (R_cap, and — an array another pass
// has re-allocated since — every allocation itself) and in the packed paths.  Anything else is laid out in full.
static bool append_fits(const mgx_world *w) {
#ifdef MGX_STAMPS
    return false;  // (the diagnostic words are sized by the robot count)
#endif
    const DevWorld &d = w->d;
    const size_t R0 = w->robot_of.size(), R1 = w->robots.size(), K = (size_t)w->K;
    if (!w->reserve_want || R1 > (size_t)w->R_cap || (size_t)d.R_local != R0 || d.R_total != d.R_local) return false;
    if (w->xres.connected || w->direct.connected || w->rccl.connected) return false;
    if (w->frozen_live || w->ir_frozen_live || w->thaw_kinds != 0 || w->n_keyless != 0) return false;
    size_t pts = device_path_points(w);
    for (size_t id = R0; id < R1; id++) {
        const Robot &rb = w->robots[id];
        if (rb.ghost || rb.K != w->K) return false;
        pts += rb.path.size() / 2;
    }
    const size_t K2 = K - 2;
    return 2 * pts <= w->path_xy.cap && R1 + 1 <= w->path_ptr.cap && (size_t)d.BS * R1 <= w->blob.cap && 24 * K * R1 <= std::min(w->snap0.cap, w->snap1.cap) &&
           K * R1 <= std::min(w->epoch0.cap, w->epoch1.cap) && (K - 1) * R1 <= (size_t)d.ND && 16 * (size_t)d.ND <= w->dyn_m.cap &&
           std::max<size_t>(K2, 1) * R1 <= (size_t)d.NT && (size_t)d.NT <= std::min(w->trk_record.cap, w->trk_last_val.cap) && 2 * (size_t)d.NT <= w->trk_last_pos.cap &&
           R1 <= w->iter_factor.cap && R1 <= w->radius_dev.cap && R1 <= std::min(w->antenna.cap, w->idle.cap) && R1 + 1 <= w->in_ptr_dev.cap &&
           R1 <= w->in_mid_dev.cap && K * R1 + 1 <= w->ir_var_ptr.cap && K * R1 <= w->ir_var_mid.cap && w->dev_in_ptr.size() == R0 + 1;
}
// All robots added since the last commit, together: one staged block (one record each, as commit() packs them: pack_robot),
// one dispatch (k_append_robots).  Unsharded, so the device order is the id order and the new robots' device indices follow
// the old ones'.  Nothing is pulled: the host mirror of the robots already there stays as stale as it is between two pulls.
static int append_robots(mgx_world *w) {
    StageTimer tm("append");
    DevWorld &d = w->d;
    const int K = w->K, R0 = d.R_local, R1 = (int)w->robots.size(), n = R1 - R0;
    const AppendLayout L{K, d.BS};
    const size_t RW = (size_t)L.words();
    size_t path_floats = 0;
    for (int id = R0; id < R1; id++) path_floats += w->robots[(size_t)id].path.size();
    void *hp = nullptr, *dp = nullptr;
    int slot = 0;
    HIP_TRY(w->stage.acquire(RW * sizeof(double) * (size_t)n + path_floats * sizeof(float), &hp, &slot));
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    double *rec0 = (double *)hp;
    float *paths = (float *)(rec0 + RW * (size_t)n);
    size_t path_at = 0, path_base = device_path_points(w);
    memset(hp, 0, RW * sizeof(double) * (size_t)n);
    for (int a = 0; a < n; a++) {
        const Robot &rb = w->robots[(size_t)(R0 + a)];
        double *rec = rec0 + RW * (size_t)a;
        AppendHeader *h = (AppendHeader *)rec;
        h->path_at = (int32_t)path_at;
        h->n_path = (int32_t)(rb.path.size() / 2);
        h->path_base = (int32_t)path_base;
        h->iter_factor = rb.iter_factor;
        h->radius = rb.radius;
        h->antenna = rb.antenna;
        h->idle = rb.idle;
        float *tp = (float *)(rec + L.trk_pos());
        pack_robot(rb, RobotSink{rec + L.blob(), rec + L.snap(), (uint32_t *)(rec + L.epoch()), rec + L.dyn(), 1, 16, (int32_t *)(rec + L.trk_rec()),
                                 tp, tp + (K - 2), rec + L.trk_val()});
        std::copy(rb.path.begin(), rb.path.end(), paths + path_at);
        path_at += rb.path.size();
        path_base += rb.path.size() / 2;
    }
    tm.lap("block");
    AppendTargets t{};
    t.block = (const double *)dp;
    t.n = n;
    t.room = w->R_cap;
    t.path_room = (int)(w->path_xy.cap / 2);
    t.in_end = w->dev_in_ptr.back();
    t.path_ptr = w->path_ptr.p; t.path_xy = w->path_xy.p; t.radius = w->radius_dev.p;
    t.antenna = w->antenna.p; t.idle = w->idle.p;
    t.in_ptr = w->in_ptr_dev.p; t.in_mid = w->in_mid_dev.p; t.var_ptr = w->ir_var_ptr.p; t.var_mid = w->ir_var_mid.p;
    HIP_TRY(launch_append_robots(d, L, t, w->stream));
    HIP_TRY(w->stage.release(slot, w->stream));
    tm.lap("launch");
    // the host's picture of the layout
    w->dev_of.resize(w->robots.size(), -1);
    for (int id = R0; id < R1; id++) {
        w->dev_of[(size_t)id] = id;
        w->robot_of.push_back(id);
        w->dev_in_ptr.push_back(t.in_end);
    }
    d.R_local = d.R_total = R1;
    d.V = R1 * K;
    w->path_ptr.n = std::max(w->path_ptr.n, (size_t)R1 + 1);
    w->path_xy.n = std::max(w->path_xy.n, 2 * path_base);
    w->radius_dev.n = std::max(w->radius_dev.n, (size_t)R1);
    w->iter_factor.n = std::max(w->iter_factor.n, (size_t)R1);
    w->rinc.all = true;  // (every robot's peer row moves with the row pointers' count: the next topology pass sends everybody's piece — a device pass)
    w->res.robots_appended();
    w->halo_dirty = true;
    w->direct.aimed = false;
    w->search.sets_touched();
    w->mission.alive_dirty = true;
    w->dirty = false;
    w->n_appends++;
    w->n_robots_appended += (uint64_t)n;
    tm.lap("bookkeeping");
    return MGX_OK;
}

static int commit(mgx_world *w) {
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
    MGX_CONFIRM(w);
    // (whoever comes through here enqueues work or reads state: a lingering launch ends first — unless the caller is on its way
    // to post a schedule into it)
    if (!w->res.linger.hold) { const int rcl = linger_close(w); if (rcl != MGX_OK) return rcl; }
    if (w->dirty && !w->relayout && w->dev_valid) {
        // nothing but robots joined since the arrays were laid out: a world with head-room takes them on the device
        if (w->robots.size() == w->robot_of.size()) {
            w->dirty = false;
        } else if (append_fits(w)) {
            if (w->res.linger.open) { const int rcl = linger_close(w); if (rcl != MGX_OK) return rcl; }  // (every call that adds a robot has ended it already)
            const int rca = append_robots(w);
            if (rca != MGX_OK) return rca;
        }
    }
    if (!w->dirty) {
        if (w->conns_dirty) return retopo(w);
        if (w->flags_dirty) return upload_flags(w);
        return MGX_OK;
    }
    if (w->robots.empty()) return fail(MGX_ERR_STATE, "world has no robots");
    StageTimer tmc("commit");
    // (a reserved world that was laid out before and has new robots, on the full path all the same: what mgx_append_stats calls a fallback)
    if (w->reserve_want && !w->robot_of.empty() && w->robots.size() > w->robot_of.size()) w->n_append_fallbacks++;
    int rc = pull(w);
    if (rc != MGX_OK) return rc;
    tmc.lap("pull (device -> host mirror)");
    const int K = w->K, E = 4 * K - 6;
    if (!sweep_supports(K) || sweep_lds_bytes(K, 0) > 60 * 1024) return fail(MGX_ERR_INVALID, "K = %d not supported (3 <= K <= 45: the robot's graph has to fit 60 KB of LDS)", K);

    // device robot order: locals (id order), then ghosts
    const std::vector<int> order_before = std::move(w->robot_of);
    const int R_local_before = w->d.R_local;
    w->robot_of.clear();
    w->dev_of.assign(w->robots.size(), -1);
    for (size_t r = 0; r < w->robots.size(); r++)
        if (!w->robots[r].ghost) { w->dev_of[r] = (int)w->robot_of.size(); w->robot_of.push_back((int)r); }
    const int R_local = (int)w->robot_of.size();
    for (size_t r = 0; r < w->robots.size(); r++)
        if (w->robots[r].ghost) { w->dev_of[r] = (int)w->robot_of.size(); w->robot_of.push_back((int)r); }
    const int R_total = (int)w->robot_of.size();
    // Head-room (mgx_world_reserve): the per-robot arrays are sized, and the strided tables strided, for R_cap robots — what the
    // caller asked for, or twice the robots there are once they outgrew that (a logarithmic number of layouts).  Ghosts follow
    // the locals in device order, so a world that holds any has none; a world that never asked has R_cap == R_local, and every
    // array below is what it always was.
    const int R_cap = (w->reserve_want && R_total == R_local) ? ((uint32_t)R_local > w->reserve_want ? 2 * R_local : (int)w->reserve_want) : R_local;
    const int RT_cap = R_total + (R_cap - R_local);
    const size_t V = (size_t)R_total * K, V_cap = (size_t)RT_cap * K, EI = (size_t)std::max(R_cap, 1) * E, ND = (size_t)std::max(R_cap, 1) * (K - 1),
                 NT = (size_t)std::max(R_cap, 1) * std::max(K - 2, 1);

    // initialise fresh inter-robot edges from the (pulled) current state: created epoch of the
    // owner's variable (its inbox slot stays empty until the owner's next delivery) and the target
    // variable's current belief mean (robot.rs:1549-1585)
    for (IrConn &c : w->conns)
        for (size_t j = 0; j < c.edges.size(); j++) {
            IrEdge &ed = c.edges[j];
            if (!ed.fresh) continue;
            const Robot &ow = w->robots[(size_t)c.owner], &ot = w->robots[(size_t)c.other];
            ed.created = ow.epoch[j + 1];
            for (int q = 0; q < 4; q++) ed.bmu[q] = (w->p.enable_mask & 2u) ? ot.bel_mu[4 * (j + 1) + q] : 0.0;  // dropped while the kind is off
            ed.fresh = false;
        }

    Incoming t;
    build_incoming(w, R_local, t);
    if (!t.blocks_ok) return fail(MGX_ERR_STATE, "internal: node slots of two connections interleave");
    const size_t n_slots = t.in_list.size(), NI = n_slots * (size_t)(K - 1), NIs = std::max<size_t>(NI, 1);
    std::vector<IrEdgeRec> recs(NIs, IrEdgeRec{0, 0, 0, 0, 0.0, 0.0});
    std::vector<double> ife(4 * NIs, 0.0), ifl(16 * NIs, 0.0), ibm(4 * NIs, 0.0);
    for (mgx_world::ConnHot &h : w->conn_hot) h.dev_q = -1;
    for (size_t g = 0; g < n_slots; g++) {
        IrConn &c = w->conns[(size_t)t.in_list[g]];
        const int r = w->dev_of[(size_t)c.other];
        w->conn_hot[(size_t)t.in_list[g]].dev_q = (int32_t)g - t.in_ptr[(size_t)r];
        for (int j = 0; j < K - 1; j++) {
            const size_t e = edge_index(t.in_ptr, K, r, j, (int)g);
            const IrEdge &ed = c.edges[(size_t)j];
            recs[e] = edge_record(w, c, j);
            recs[e].created = ed.created;
            scatter(ife, NIs, e, ed.fv_eta, 4);
            scatter(ifl, NIs, e, ed.fv_lam, 16);
            scatter(ibm, NIs, e, ed.bmu, 4);
        }
    }
    w->dev_in_ptr = t.in_ptr;
    const int ir_max_edges = t.ir_max_edges;

    const size_t BS = (size_t)blob_words(K);
    std::vector<double> blb(BS * (size_t)RT_cap, 0.0), sn(24 * V_cap), dm(16 * ND, 0.0), tlv(NT, 0.0);
    std::vector<int32_t> trc(NT, 0), pptr((size_t)R_cap + 1, 0), itf((size_t)std::max(R_cap, 1), 0);
    std::vector<uint32_t> ep(V_cap);
    std::vector<float> tlp(2 * NT, 0.f), pxy;
    std::vector<double> rad((size_t)RT_cap, 0.0);
    size_t longest_path = 0;
    for (int dr = 0; dr < R_total; dr++) {
        const Robot &rb = w->robots[(size_t)w->robot_of[(size_t)dr]];
        rad[(size_t)dr] = rb.radius;
        const size_t d0 = (size_t)dr * (K - 1), t0 = (size_t)dr * (K - 2);
        pack_robot(rb, RobotSink{&blb[(size_t)dr * BS], &sn[(size_t)dr * K * 24], &ep[(size_t)dr * K], dm.data() + d0, ND, 1, trc.data() + t0,
                                 tlp.data() + t0, tlp.data() + NT + t0, tlv.data() + t0});
        if (rb.ghost) continue;
        pptr[(size_t)dr] = (int32_t)(pxy.size() / 2);
        pxy.insert(pxy.end(), rb.path.begin(), rb.path.end());
        pptr[(size_t)dr + 1] = (int32_t)(pxy.size() / 2);
        itf[(size_t)dr] = rb.iter_factor;
        longest_path = std::max(longest_path, rb.path.size());
    }
    for (int dr = R_local; dr < R_cap; dr++) {  // the head-room's (empty) ranges end where the last robot's do
        pptr[(size_t)dr + 1] = pptr[(size_t)R_local];
        t.in_ptr.push_back(t.in_ptr[(size_t)R_local]);
    }
    t.mid.resize((size_t)std::max(R_cap, 1), 0);
    if (pxy.empty()) pxy.assign(2, 0.f);
    // (path slack: a robot that joins brings a path; room for one as long as the longest so far, 32 points at the least, per free place)
    const size_t path_room = pxy.size() + (size_t)(R_cap - R_local) * std::max<size_t>(longest_path, 2 * APPEND_PATH_POINTS);
    if (recs.empty()) recs.push_back(IrEdgeRec{0, 0, 0, 0, 0.0, 0.0});
    if (w->sdf_red.empty()) {  // no image: every lookup is "outside" => h = 0
        w->sdf_red.assign(1, 255);
        w->sdf_w = w->sdf_h = 0;
    }

    tmc.lap("host arrays");
    hipStream_t s = w->stream;
    HIP_TRY(w->blob.upload(blb, s));
    HIP_TRY(w->snap0.upload(sn, s));
    HIP_TRY(w->snap1.upload(sn, s));
    HIP_TRY(w->epoch0.upload(ep, s));
    HIP_TRY(w->epoch1.upload(ep, s));
    HIP_TRY(w->dyn_m.upload(dm, s));
    HIP_TRY(w->trk_record.upload(trc, s));
    HIP_TRY(w->trk_last_pos.upload(tlp, s));
    HIP_TRY(w->trk_last_val.upload(tlv, s));
    HIP_TRY(w->path_ptr.upload(pptr, s));
    HIP_TRY(w->path_xy.upload(pxy, s, path_room));
    HIP_TRY(w->iter_factor.upload(itf, s));
    HIP_TRY(w->radius_dev.upload(rad, s));
    HIP_TRY(w->in_ptr_dev.upload(t.in_ptr, s));
    HIP_TRY(w->in_mid_dev.upload(t.mid, s));
    HIP_TRY(w->ir_var_ptr.reserve((size_t)R_cap * K + 1));
    HIP_TRY(w->ir_var_mid.reserve((size_t)std::max(R_cap, 1) * K));
    HIP_TRY(launch_var_tables(R_local, K, w->in_ptr_dev.p, w->in_mid_dev.p, w->ir_var_ptr.p, w->ir_var_mid.p, s));
    HIP_TRY(w->ir_rec.upload(recs, s));
    HIP_TRY(w->ir_fv_eta.upload(ife, s));
    HIP_TRY(w->ir_fv_lam.upload(ifl, s));
    HIP_TRY(w->ir_bmu.upload(ibm, s));
    HIP_TRY(w->sdf.upload(w->sdf_red, s));
    std::vector<double> fzd;
    std::vector<uint8_t> fzf, thw, zero_bytes;
    if (w->frozen_live) {  // robots that joined since start with empty frozen inboxes and nothing to thaw
        const size_t FZ = (size_t)frozen_words(K), RL = (size_t)std::max(R_local, 1);
        fzd.assign(RL * FZ, 0.0);
        fzf.assign(RL * (size_t)E, 0);
        thw.assign(RL, 0);
        zero_bytes.assign(RL, 0);
        for (int dr = 0; dr < R_local; dr++) {
            const Robot &rb = w->robots[(size_t)w->robot_of[(size_t)dr]];
            if (rb.frozen.size() == FZ) std::copy(rb.frozen.begin(), rb.frozen.end(), fzd.begin() + (long)((size_t)dr * FZ));
            if (rb.frozen_flag.size() == (size_t)E) std::copy(rb.frozen_flag.begin(), rb.frozen_flag.end(), fzf.begin() + (long)((size_t)dr * (size_t)E));
            else nokey_flags(rb.nokey, K, &fzf[(size_t)dr * (size_t)E]);  // (joined while kinds were off: those factors have no inbox keys)
            thw[(size_t)dr] = rb.thaw;
        }
        HIP_TRY(w->frozen_buf.upload(fzd, s));
        HIP_TRY(w->frozen_flag_buf.upload(fzf, s));
        HIP_TRY(w->thaw_buf.upload(thw, s));
        HIP_TRY(w->skip0_buf.upload(zero_bytes, s));
    }
    std::vector<double> ifs;
    std::vector<uint32_t> ife_, ite;
    if (w->ir_frozen_live) {  // robots that joined since have sent nothing their (disabled) factors could have kept
        ifs.assign(24 * V, 0.0);
        ife_.assign(V, 0);
        ite.assign(V, 0xffffffffu);  // "has delivered since": a joiner's live record is its inbox
        for (int dr = 0; dr < R_total; dr++) {
            const Robot &rb = w->robots[(size_t)w->robot_of[(size_t)dr]];
            if (rb.ir_frozen_snap.size() == (size_t)24 * K) std::copy(rb.ir_frozen_snap.begin(), rb.ir_frozen_snap.end(), ifs.begin() + (long)((size_t)dr * K * 24));
            if (rb.ir_frozen_epoch.size() == (size_t)K) std::copy(rb.ir_frozen_epoch.begin(), rb.ir_frozen_epoch.end(), ife_.begin() + (long)((size_t)dr * K));
            if (rb.ir_thaw_epoch.size() == (size_t)K) std::copy(rb.ir_thaw_epoch.begin(), rb.ir_thaw_epoch.end(), ite.begin() + (long)((size_t)dr * K));
        }
        HIP_TRY(w->ir_frozen_snap_buf.upload(ifs, s));
        HIP_TRY(w->ir_frozen_epoch_buf.upload(ife_, s));
        HIP_TRY(w->ir_thaw_epoch_buf.upload(ite, s));
    }
    HIP_TRY(hipStreamSynchronize(s));  // host staging vectors die at scope exit
    tmc.lap("uploads + synchronisation");

    DevWorld &d = w->d;
    d.R_local = R_local; d.R_total = R_total; d.K = K; d.E = E;
    d.V = (int)V; d.EI = (int)EI; d.ND = (int)ND; d.NT = (int)NT; d.NI = (int)NIs;
    d.cur = 0;
    d.ir_max_edges = ir_max_edges;
    d.trk_cols = w->trk_ever_on ? 1 : 0;
    d.upd = nullptr; d.upd_max_speed = 0.0; d.upd_delta_t = 0.0;
    d.ir_frozen_snap = w->ir_thaw_active ? w->ir_frozen_snap_buf.p : nullptr;
    d.ir_frozen_epoch = w->ir_thaw_active ? w->ir_frozen_epoch_buf.p : nullptr;
    d.ir_thaw_epoch = w->ir_thaw_active ? w->ir_thaw_epoch_buf.p : nullptr;
    d.frozen = w->frozen_live ? w->frozen_buf.p : nullptr;
    d.frozen_flag = w->frozen_live ? w->frozen_flag_buf.p : nullptr;
    d.thaw = w->frozen_live ? w->thaw_buf.p : nullptr;
    d.skip0 = (w->frozen_live && w->thaw_kinds) ? w->skip0_buf.p : nullptr;
    d.enable = w->p.enable_mask;
    d.blob = w->blob.p; d.BS = (int)BS;
    d.snap[0] = w->snap0.p; d.snap[1] = w->snap1.p;
    d.snap_epoch[0] = w->epoch0.p; d.snap_epoch[1] = w->epoch1.p;
    d.dyn_m = w->dyn_m.p;
    d.trk_record = w->trk_record.p; d.trk_last_pos = w->trk_last_pos.p; d.trk_last_val = w->trk_last_val.p;
    d.path_ptr = w->path_ptr.p; d.path_xy = w->path_xy.p; d.iter_factor = w->iter_factor.p;
    d.ir_var_ptr = w->ir_var_ptr.p; d.ir_var_mid = w->ir_var_mid.p; d.ir_rec = w->ir_rec.p;
    d.ir_fv_eta = w->ir_fv_eta.p; d.ir_fv_lam = w->ir_fv_lam.p; d.ir_bmu = w->ir_bmu.p;
    d.sdf = w->sdf.p; d.sdf_w = w->sdf_w; d.sdf_h = w->sdf_h; d.world_w = w->world_w; d.world_h = w->world_h;
    // ObstacleFactor::new jacobian_delta (obstacle.rs:98-102)
    d.obs_delta = (w->sdf_w && w->sdf_h) ? (w->world_w / (double)w->sdf_w + w->world_h / (double)w->sdf_h) / 2.0 : 1.0;
    if (f64_bits(w->obs_delta_checked) != f64_bits(d.obs_delta)) {
        w->obs_inv_delta = obstacle_inv_delta(d.obs_delta);
        w->obs_delta_checked = d.obs_delta;
    }
    if (!(f64_bits(w->obs_inv_delta) << 1))
        return fail(MGX_ERR_INVALID, "obstacle factors: jacobian delta %g (world size / image size) has no reciprocal that reproduces the division (zero, not finite, or near the ends of the f64 range)", d.obs_delta);
    d.obs_inv_delta = w->obs_inv_delta;
    d.inv_s2_obs = 1.0 / (w->p.sigma_obstacle * w->p.sigma_obstacle);    // FactorState::new, factor/mod.rs:631-632
    d.inv_s2_ir = 1.0 / (w->p.sigma_interrobot * w->p.sigma_interrobot);
    d.inv_s2_trk = 1.0 / (w->p.sigma_tracking * w->p.sigma_tracking);
    d.trk_pad = w->p.tracking_switch_padding;
    d.trk_attr = w->p.tracking_attraction_distance;
#ifdef MGX_STAMPS
    {
        // [.. * 16): stages per wave, then 16 sub-stage sums per wave; behind them the hand-off timeline, 16 segments x 4 per robot
        std::vector<unsigned long long> z((size_t)(R_local + 4) * 48 + (size_t)R_local * 64, 0ull);
        HIP_TRY(w->dbg.upload(z, s));
        HIP_TRY(hipStreamSynchronize(s));
        d.dbg = w->dbg.p;
    }
#else
    d.dbg = nullptr;
#endif
    w->dirty = w->relayout = false;
    w->R_cap = R_cap;
    w->conns_dirty = false;
    w->rinc.all = true;  // (no slot records on the device yet, device indices may have moved: the first topology change sends everything)
    w->rinc.clear_marks();
    w->dev_valid = true;
    w->n_layouts++;
    w->halo_dirty = true;
    w->res.arrays_rebuilt();
    w->xres.connected = false;  // ghost slots and progress words belonged to the old layout: the ranks wire them again
    // the direct exchange's pushes name device indices and ghost slots: they stay good for as long as the robots' device order does
    // (a relayout for new obstacles or reset variables keeps it; a robot that joins, migrates or is released does not)
    if (w->robot_of != order_before || R_local != R_local_before) w->direct.aimed = false;
    d.gxrec[0] = d.gxrec[1] = nullptr; d.gflag = nullptr; d.xp_ptr = nullptr; d.xp_rec = nullptr;
    w->xres.agree = nullptr; d.agree = nullptr; d.n_ranks = 0;
    if (!w->sweep_err_host) {  // the word device code reports a wait that gave up in (resident launches, direct halo waits)
        HIP_TRY(hipHostMalloc((void **)&w->sweep_err_host, sizeof(unsigned long long), hipHostMallocMapped));
        *w->sweep_err_host = 0ull;
    }
    {
        void *dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, w->sweep_err_host, 0));
        w->d.sweep_err = (unsigned long long *)dp;
    }
    rc = upload_flags(w);
    tmc.lap("flags");
    return rc;
}

// A wait on the device gave up — a direct halo exchange whose producer never published, or a resident schedule
// launch whose neighbour never did: the waiting kernels end (never a hung GPU) but what they computed from stale
// records is wrong.  Sticky: every later sweep, synchronisation and read-back reports it.
static int check_device_error(mgx_world *w) {
    if (w->sticky_rc != MGX_OK)
        return fail(w->sticky_rc, "a schedule that had to be run again launch by launch (its resident launch was declined) failed with code %d "
                    "inside a call that edits the graph: the world is behind the schedules issued", w->sticky_rc);
    if (w->sweep_err_host && *w->sweep_err_host != 0ull)
        return fail(MGX_ERR_STATE, "a wait on the device timed out (exchange / progress word %llu): a peer rank or a neighbouring "
                    "workgroup never published its records, the world's beliefs are invalid", *w->sweep_err_host);
    return MGX_OK;
}
