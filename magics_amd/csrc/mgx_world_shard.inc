// mgx_world_shard.inc — C ABI: sharded worlds — exchange lists, migration, the in-engine transports (RCCL, direct, ghost records inside resident launches), hipIpc, pack / unpack.
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
extern "C" {
uint32_t mgx_halo_words(uint32_t K) { return (SNAP_W + 1) * K; }

int mgx_halo_plan(mgx_world *w, uint32_t n_send, const int32_t *send_robots, uint32_t n_recv, const int32_t *recv_ghosts) {
    MGX_ENTER(w);
    if (!w || (n_send && !send_robots) || (n_recv && !recv_ghosts)) return fail(MGX_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < n_send; i++)
        if (send_robots[i] < 0 || (size_t)send_robots[i] >= w->robots.size() || w->robots[(size_t)send_robots[i]].ghost)
            return fail(MGX_ERR_INVALID, "send list entry %u is not a local robot", i);
    for (uint32_t i = 0; i < n_recv; i++)
        if (recv_ghosts[i] < 0 || (size_t)recv_ghosts[i] >= w->robots.size() || !w->robots[(size_t)recv_ghosts[i]].ghost)
            return fail(MGX_ERR_INVALID, "receive list entry %u is not a ghost robot", i);
    w->halo_send.assign(send_robots, send_robots + n_send);
    w->halo_recv.assign(recv_ghosts, recv_ghosts + n_recv);
    w->halo_dirty = true;
    w->direct.aimed = false;
    return MGX_OK;
}

// The exchange lists a rank needs for the connections it holds: every connection A -> B is evaluated on
// the rank of B, which needs A's snapshot records.  With the replicated bookkeeping of a sharded world
// that follows its topology (all robots present everywhere) both ends derive the same lists.
int mgx_halo_plan_from_connections(mgx_world *w, const int32_t *rank_of, uint32_t n_robots, int32_t my_rank, uint32_t n_ranks,
                                   uint32_t *send_counts, uint32_t *recv_counts) {
    MGX_ENTER(w);
    if (!w || !rank_of || !send_counts || !recv_counts) return fail(MGX_ERR_INVALID, "null argument");
    if (n_robots != w->robots.size() || my_rank < 0 || (uint32_t)my_rank >= n_ranks) return fail(MGX_ERR_INVALID, "bad rank table");
    for (uint32_t r = 0; r < n_robots; r++) {
        if (rank_of[r] < 0 || (uint32_t)rank_of[r] >= n_ranks) return fail(MGX_ERR_INVALID, "robot %u: bad rank %d", r, rank_of[r]);
        if ((rank_of[r] != my_rank) != w->robots[r].ghost) return fail(MGX_ERR_INVALID, "robot %u: rank table and ghost flag disagree", r);
    }
    std::vector<std::vector<int32_t>> send(n_ranks), recv(n_ranks);
    for (const IrConn &c : w->conns) {
        const int ro = rank_of[(size_t)c.owner], rt = rank_of[(size_t)c.other];
        if (ro == rt) continue;
        if (rt == my_rank) recv[(size_t)ro].push_back(c.owner);
        else if (ro == my_rank) send[(size_t)rt].push_back(c.owner);
    }
    w->halo_send.clear();
    w->halo_recv.clear();
    for (uint32_t p = 0; p < n_ranks; p++) {
        for (std::vector<int32_t> *l : {&send[p], &recv[p]}) {
            std::sort(l->begin(), l->end());
            l->erase(std::unique(l->begin(), l->end()), l->end());
        }
        send_counts[p] = (uint32_t)send[p].size();
        recv_counts[p] = (uint32_t)recv[p].size();
        w->halo_send.insert(w->halo_send.end(), send[p].begin(), send[p].end());
        w->halo_recv.insert(w->halo_recv.end(), recv[p].begin(), recv[p].end());
    }
    w->halo_dirty = true;
    w->direct.aimed = false;
    return MGX_OK;
}

// the exchange lists as they stand (robot ids; send list by consumer rank, receive list by producer rank — the order of the counts
// mgx_halo_plan_from_connections returned): n_send / n_recv receive the lengths, the arrays are filled up to their capacities
int mgx_halo_get_lists(mgx_world *w, int32_t *send_robots, uint32_t send_capacity, int32_t *recv_robots, uint32_t recv_capacity,
                       uint32_t *n_send, uint32_t *n_recv) {
    MGX_ENTER(w);
    if (!w || !n_send || !n_recv) return fail(MGX_ERR_INVALID, "null argument");
    *n_send = (uint32_t)w->halo_send.size();
    *n_recv = (uint32_t)w->halo_recv.size();
    if (send_robots) for (size_t i = 0; i < w->halo_send.size() && i < send_capacity; i++) send_robots[i] = w->halo_send[i];
    if (recv_robots) for (size_t i = 0; i < w->halo_recv.size() && i < recv_capacity; i++) recv_robots[i] = w->halo_recv[i];
    return MGX_OK;
}

// ---- migration: a robot changes its owning rank (worlds that follow their topology) --------------------------------------
// Everything that exists on the owner's rank ONLY travels in one flat record: the graph's numeric state (priors, beliefs,
// factor -> variable messages, snapshot records and delivery counts, tracking records, iteration count, the path, the
// frozen inboxes of switched-off kinds), the totals of its own MessageCount, and the state of every inter-robot factor
// attached to its variables (kept at the TARGET's rank).  The replicated bookkeeping — connection sets, node slots, robot
// numbers, flags, the connections' counters — is the same on every rank already and stays where it is.
}  // extern "C" (the record's writer and reader are templates)
namespace {
struct MigWriter {
    std::vector<uint8_t> b;
    template <class T> void pod(const T &v) { const uint8_t *p = reinterpret_cast<const uint8_t *>(&v); b.insert(b.end(), p, p + sizeof(T)); }
    template <class T> void vec(const std::vector<T> &v) {
        pod((uint64_t)v.size());
        const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
        b.insert(b.end(), p, p + sizeof(T) * v.size());
        while (b.size() & 7) b.push_back(0);
    }
};
struct MigReader {
    const uint8_t *p, *end;
    bool ok = true;
    template <class T> void pod(T &v) {
        if (!ok || (size_t)(end - p) < sizeof(T)) { ok = false; return; }
        memcpy(&v, p, sizeof(T));
        p += sizeof(T);
    }
    template <class T> void vec(std::vector<T> &v, size_t want = (size_t)-1) {
        uint64_t n = 0;
        pod(n);
        if (!ok || n > (uint64_t)(end - p) / sizeof(T) || (want != (size_t)-1 && n != want)) { ok = false; return; }
        v.resize((size_t)n);
        if (n) memcpy(v.data(), p, sizeof(T) * (size_t)n);
        p += ((sizeof(T) * (size_t)n + 7) & ~(size_t)7);
        if (p > end) ok = false;
    }
};
constexpr uint32_t MIG_MAGIC = 0x4d47584du;  // "MXGM"
constexpr uint32_t MIG_VERSION = 1;
}  // namespace
extern "C" {

// The record of a robot this rank owns (mgx_robot_import takes it on the rank that is to own it).  `bytes` receives the
// record's size; with buf == NULL or capacity too small nothing is copied (MGX_ERR_INVALID when a buffer was given).
// The world is brought up to date first: schedules issued so far have run, the tables of the last topology pass are laid
// out.  Call it BETWEEN ticks — after the sweeps that followed the last topology pass — on every rank at the same point.
int mgx_robot_export(mgx_world *w, int32_t robot, void *buf, uint64_t capacity, uint64_t *bytes) {
    MGX_ENTER(w);
    if (!w || !bytes || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    if (w->robots[(size_t)robot].ghost) return fail(MGX_ERR_INVALID, "robot %d is a ghost here: its owner exports it", robot);
    if ((size_t)robot < w->mission.has.size() && w->mission.has[(size_t)robot])
        return fail(MGX_ERR_STATE, "robot %d has a mission on this device (mgx_mission_set): missions do not migrate — routes, next waypoints "
                                   "and Transforms are state of unsharded worlds (include/mgx.h)", robot);
    int rc = check_device_error(w);
    if (rc != MGX_OK) return rc;
    if (w->dev_valid && (w->dirty || w->conns_dirty || w->flags_dirty)) {  // (not valid: the host mirror is the truth already)
        rc = commit(w);
        if (rc != MGX_OK) return rc;
    }
    rc = pull(w);
    if (rc != MGX_OK) return rc;
    flush_counts(w);
    const Robot &rb = w->robots[(size_t)robot];
    MigWriter wr;
    wr.pod(MIG_MAGIC); wr.pod(MIG_VERSION);
    wr.pod((int32_t)rb.K); wr.pod((int32_t)robot);
    wr.pod((uint64_t)rb.order_key);
    wr.pod((int32_t)rb.iter_factor); wr.pod((int32_t)rb.thaw);
    for (int q = 0; q < 4; q++) wr.pod((uint64_t)rb.cnt[q]);
    wr.vec(rb.prior_eta); wr.vec(rb.prior_lam); wr.vec(rb.bel_eta); wr.vec(rb.bel_lam); wr.vec(rb.bel_mu); wr.vec(rb.bel_cov);
    wr.vec(rb.valid); wr.vec(rb.snap); wr.vec(rb.epoch); wr.vec(rb.fv_eta); wr.vec(rb.fv_lam);
    wr.vec(rb.trk_record); wr.vec(rb.trk_last_pos); wr.vec(rb.trk_last_val); wr.vec(rb.path);
    wr.vec(rb.frozen); wr.vec(rb.frozen_flag); wr.vec(rb.ir_frozen_snap); wr.vec(rb.ir_frozen_epoch); wr.vec(rb.ir_thaw_epoch);
    uint32_t n_conn = 0;
    for (const IrConn &c : w->conns) n_conn += c.other == robot ? 1u : 0u;
    wr.pod(n_conn); wr.pod((uint32_t)0);
    for (const IrConn &c : w->conns) {
        if (c.other != robot) continue;
        wr.pod((int32_t)c.owner); wr.pod((int32_t)c.node_first);
        wr.pod((uint64_t)c.first_number);
        for (const IrEdge &ed : c.edges) {
            for (double v : ed.fv_eta) wr.pod(v);
            for (double v : ed.fv_lam) wr.pod(v);
            for (double v : ed.bmu) wr.pod(v);
            wr.pod((uint32_t)ed.created); wr.pod((uint32_t)(ed.fresh ? 1 : 0));
        }
    }
    *bytes = (uint64_t)wr.b.size();
    if (!buf) return MGX_OK;
    if (capacity < wr.b.size()) return fail(MGX_ERR_INVALID, "the record of robot %d takes %zu bytes, %llu given", robot, wr.b.size(), (unsigned long long)capacity);
    memcpy(buf, wr.b.data(), wr.b.size());
    return MGX_OK;
}

// The robot — a ghost here so far — becomes this rank's: its graph and the factors attached to its variables take the
// state of the record.  The device state is pulled, the host mirror edited, and the next launch lays the world out again
// (locals first: device indices change, so every wiring that names them — exchange lists, direct / resident halo — is
// made again by the launcher, as after mgx_robot_add).  The replicated bookkeeping has to be in step with the exporting
// rank's: the record names its connections (owner, first robot number, first node slot) and a mismatch is refused.
int mgx_robot_import(mgx_world *w, int32_t robot, const void *buf, uint64_t bytes) {
    MGX_ENTER(w);
    if (!w || !buf || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    if (!w->robots[(size_t)robot].ghost) return fail(MGX_ERR_STATE, "robot %d is owned here already", robot);
    if ((size_t)robot < w->mission.has.size() && w->mission.has[(size_t)robot])
        return fail(MGX_ERR_STATE, "robot %d has a mission on this device (mgx_mission_set): missions do not migrate — routes, next waypoints "
                                   "and Transforms are state of unsharded worlds (include/mgx.h)", robot);
    int rc = check_device_error(w);
    if (rc != MGX_OK) return rc;
    if (w->dev_valid && (w->dirty || w->conns_dirty || w->flags_dirty)) {
        rc = commit(w);
        if (rc != MGX_OK) return rc;
    }
    rc = pull(w);
    if (rc != MGX_OK) return rc;
    flush_counts(w);
    MigReader rd{(const uint8_t *)buf, (const uint8_t *)buf + bytes};
    uint32_t magic = 0, version = 0, n_conn = 0, pad = 0;
    int32_t K = 0, id = 0, itf = 0, thaw = 0;
    uint64_t key = 0, cnt[4] = {0, 0, 0, 0};
    rd.pod(magic); rd.pod(version); rd.pod(K); rd.pod(id); rd.pod(key); rd.pod(itf); rd.pod(thaw);
    for (uint64_t &c : cnt) rd.pod(c);
    if (!rd.ok || magic != MIG_MAGIC || version != MIG_VERSION) return fail(MGX_ERR_INVALID, "not a robot record of this library version");
    Robot tmp = w->robots[(size_t)robot];  // (edited aside: a record that turns out malformed leaves the world untouched)
    if (K != tmp.K || id != robot || key != tmp.order_key)
        return fail(MGX_ERR_STATE, "the record is robot %d (K = %d, order key %llu): not robot %d of this world", id, K, (unsigned long long)key, robot);
    const size_t Ks = (size_t)K, E = (size_t)(4 * K - 6);
    rd.vec(tmp.prior_eta, 4 * Ks); rd.vec(tmp.prior_lam, 16 * Ks); rd.vec(tmp.bel_eta, 4 * Ks); rd.vec(tmp.bel_lam, 16 * Ks);
    rd.vec(tmp.bel_mu, 4 * Ks); rd.vec(tmp.bel_cov, 16 * Ks);
    rd.vec(tmp.valid, Ks); rd.vec(tmp.snap, 24 * Ks); rd.vec(tmp.epoch, Ks); rd.vec(tmp.fv_eta, 4 * E); rd.vec(tmp.fv_lam, 16 * E);
    rd.vec(tmp.trk_record, Ks - 2); rd.vec(tmp.trk_last_pos, 2 * (Ks - 2)); rd.vec(tmp.trk_last_val, Ks - 2); rd.vec(tmp.path);
    rd.vec(tmp.frozen); rd.vec(tmp.frozen_flag); rd.vec(tmp.ir_frozen_snap); rd.vec(tmp.ir_frozen_epoch); rd.vec(tmp.ir_thaw_epoch);
    rd.pod(n_conn); rd.pod(pad);
    if (!rd.ok || (tmp.path.size() & 1)) return fail(MGX_ERR_INVALID, "malformed robot record");
    std::vector<size_t> mine;
    for (size_t ci = 0; ci < w->conns.size(); ci++)
        if (w->conns[ci].other == robot) mine.push_back(ci);
    if (mine.size() != n_conn)
        return fail(MGX_ERR_STATE, "the record holds %u connections into robot %d, this rank's bookkeeping %zu: the ranks' topology passes are out of step",
                    n_conn, robot, mine.size());
    std::vector<std::vector<IrEdge>> edges(mine.size());
    for (size_t m = 0; m < mine.size(); m++) {
        const IrConn &c = w->conns[mine[m]];
        int32_t owner = 0, node_first = 0;
        uint64_t first_number = 0;
        rd.pod(owner); rd.pod(node_first); rd.pod(first_number);
        if (!rd.ok || owner != c.owner || node_first != c.node_first || first_number != c.first_number)
            return fail(MGX_ERR_STATE, "connection %zu into robot %d differs between the ranks (owner %d / %d): the replicated bookkeeping diverged",
                        m, robot, owner, c.owner);
        edges[m].resize(c.edges.size());
        for (IrEdge &ed : edges[m]) {
            uint32_t created = 0, fresh = 0;
            for (double &v : ed.fv_eta) rd.pod(v);
            for (double &v : ed.fv_lam) rd.pod(v);
            for (double &v : ed.bmu) rd.pod(v);
            rd.pod(created); rd.pod(fresh);
            ed.created = created;
            ed.fresh = fresh != 0;
        }
    }
    if (!rd.ok || rd.p != rd.end) return fail(MGX_ERR_INVALID, "malformed robot record (length)");
    tmp.ghost = false;
    tmp.iter_factor = itf;
    tmp.thaw = (uint8_t)thaw;
    for (int q = 0; q < 4; q++) tmp.cnt[q] = cnt[q];
    w->robots[(size_t)robot] = std::move(tmp);
    for (size_t m = 0; m < mine.size(); m++) {
        bool any_fresh = false;
        for (const IrEdge &ed : edges[m]) any_fresh = any_fresh || ed.fresh;
        w->conns[mine[m]].edges = std::move(edges[m]);
        w->conn_hot[mine[m]].has_fresh = any_fresh ? 1 : 0;
    }
    w->sets.ghost[(size_t)robot] = 0;
    w->obs.n_ghosts -= 1;
    w->dirty = w->relayout = true;
    w->dev_valid = false;  // the host mirror is the truth now (mgx_reset_variables does the same)
    w->conns_dirty = true;
    w->flags_dirty = true;
    return MGX_OK;
}

// The other half on the rank that gave the robot away (after mgx_robot_export): it stays in this world as a ghost — its
// records arrive by the exchange from now on, the factors attached to its variables are its new owner's.
int mgx_robot_release(mgx_world *w, int32_t robot) {
    MGX_ENTER(w);
    if (!w || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id");
    if (w->robots[(size_t)robot].ghost) return fail(MGX_ERR_STATE, "robot %d is a ghost here already", robot);
    if (w->sets.n_grouped) return fail(MGX_ERR_STATE, "a grouped world takes no ghosts");
    if ((size_t)robot < w->mission.has.size() && w->mission.has[(size_t)robot])
        return fail(MGX_ERR_STATE, "robot %d has a mission on this device (mgx_mission_set): missions do not migrate — routes, next waypoints "
                                   "and Transforms are state of unsharded worlds (include/mgx.h)", robot);
    int rc = check_device_error(w);
    if (rc != MGX_OK) return rc;
    if (w->dev_valid && (w->dirty || w->conns_dirty || w->flags_dirty)) {
        rc = commit(w);
        if (rc != MGX_OK) return rc;
    }
    rc = pull(w);
    if (rc != MGX_OK) return rc;
    flush_counts(w);
    Robot &rb = w->robots[(size_t)robot];
    rb.ghost = true;
    rb.path.clear();
    w->sets.ghost[(size_t)robot] = 1;
    w->obs.n_ghosts += 1;
    w->dirty = w->relayout = true;
    w->dev_valid = false;
    w->conns_dirty = true;
    w->flags_dirty = true;
    return MGX_OK;
}

static int halo_commit(mgx_world *w) {
    MGX_CONFIRM(w);
    // Changed connections alone (conns_dirty) are left to the next sweep: an exchange does not read the
    // edge tables, and the edges created by a topology pass must find the ghosts' records of the exchange
    // that follows the pass (their creation epoch is the owner's delivery count at that moment).
    if (w->dirty || !w->dev_valid) {
        int rc = commit(w);
        if (rc != MGX_OK) return rc;
    } else if (!device_ok()) {
        return fail(MGX_ERR_NO_DEVICE, "no usable HIP device");
    }
    if (!w->halo_dirty) return MGX_OK;
    std::vector<int32_t> a(w->halo_send.size()), b(w->halo_recv.size());
    for (size_t i = 0; i < a.size(); i++) a[i] = w->dev_of[(size_t)w->halo_send[i]];
    for (size_t i = 0; i < b.size(); i++) b[i] = w->dev_of[(size_t)w->halo_recv[i]];
    HIP_TRY(w->halo_send_dev.upload(a, w->stream));
    HIP_TRY(w->halo_recv_dev.upload(b, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->halo_dirty = false;
    return MGX_OK;
}

}  // extern "C" (helpers below have C++ linkage)

// The direct exchange is only as good as its last aim: the push walks dst[] by the send list's length and the wait indexes the
// receive area by ghost number, so lists or a device order newer than the aim — or more ghosts than slots — are an error here,
// not a store to wherever the old tables point.
static int direct_aim_ok(mgx_world *w) {
    const mgx_world::DirectHalo &dh = w->direct;
    const size_t NG = (size_t)(w->d.R_total - w->d.R_local);
    if (NG > dh.slot_cap)
        return fail(MGX_ERR_STATE, "%zu ghost robots but the direct exchange was wired with %zu slots: wire it again (mgx_halo_direct_setup_slots)", NG, dh.slot_cap);
    if (!dh.aimed)
        return fail(MGX_ERR_STATE, "the exchange lists or the robots' device order changed since the direct exchange was aimed: "
                                   "mgx_halo_direct_connect_slots again (robots joined: mgx_halo_direct_setup_slots on every rank first)");
    return MGX_OK;
}
// push: this rank's boundary records go to the consumers (exchange number push_seq + 1);
// wait: the ghosts are filled once every producer has published exchange seq + 1.
static int direct_push(mgx_world *w) {
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    mgx_world::DirectHalo &dh = w->direct;
    if ((rc = direct_aim_ok(w)) != MGX_OK) return rc;
    if (dh.push_seq != dh.seq) return fail(MGX_ERR_STATE, "exchange %llu is already pushed and not yet waited for", dh.push_seq);
    dh.push_seq += 1;
    const int par = (int)(dh.push_seq & 1ull);
    HIP_TRY(launch_halo_push(w->d, (int)w->halo_send.size(), w->halo_send_dev.p, dh.dst[par].p, dh.n_peers, dh.peer_flags.p, dh.push_seq,
                             dh.done.p, w->stream));
    return MGX_OK;
}
static int direct_wait(mgx_world *w) {
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    mgx_world::DirectHalo &dh = w->direct;
    if ((rc = direct_aim_ok(w)) != MGX_OK) return rc;
    if (dh.push_seq != dh.seq + 1) return fail(MGX_ERR_STATE, "nothing pushed for exchange %llu", dh.seq + 1);
    dh.seq += 1;
    const int par = (int)(dh.seq & 1ull);
    HIP_TRY(launch_halo_wait_unpack(w->d, (int)w->halo_recv.size(), w->halo_recv_dev.p, dh.recv + (size_t)par * dh.recv_words,
                                    dh.n_sources, dh.flags, dh.seq, dh.flags + dh.n_sources, dh.timeout_ticks, dh.ready.p, w->d.sweep_err,
                                    w->stream));
    return MGX_OK;
}
static int direct_exchange(mgx_world *w) {
    if (w->direct.push_seq == w->direct.seq) {  // not pushed ahead by the caller
        int rc = direct_push(w);
        if (rc != MGX_OK) return rc;
    }
    return direct_wait(w);
}

// pack -> grouped ncclSend / ncclRecv (the all-to-all-v of boundary snapshots, RCCL over xGMI) -> unpack,
// all enqueued on the world's stream
static int rccl_exchange(mgx_world *w) {
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    mgx_world::RcclHalo &rh = w->rccl;
    const size_t words = (size_t)mgx_halo_words((uint32_t)w->K);
    HIP_TRY(launch_halo_pack(w->d, (int)w->halo_send.size(), w->halo_send_dev.p, rh.send_buf.p, w->stream));
    int e = g_rccl.group_start();
    for (size_t p = 0; p < rh.peer_rank.size() && e == 0; p++) {
        const size_t ns = (size_t)(rh.send_first[p + 1] - rh.send_first[p]) * words, nr = (size_t)(rh.recv_first[p + 1] - rh.recv_first[p]) * words;
        if (ns) e = g_rccl.send(rh.send_buf.p + (size_t)rh.send_first[p] * words, ns, NCCL_FLOAT64, rh.peer_rank[p], rh.comm, w->stream);
        if (nr && e == 0) e = g_rccl.recv(rh.recv_buf.p + (size_t)rh.recv_first[p] * words, nr, NCCL_FLOAT64, rh.peer_rank[p], rh.comm, w->stream);
    }
    const int e2 = g_rccl.group_end();
    if (e || e2) return fail(MGX_ERR_HIP, "RCCL: %s", g_rccl.error_string ? g_rccl.error_string(e ? e : e2) : "error");
    HIP_TRY(launch_halo_unpack(w->d, (int)w->halo_recv.size(), w->halo_recv_dev.p, rh.recv_buf.p, w->stream));
    return MGX_OK;
}

extern "C" {

// ---- halo exchange through RCCL inside the library -----------------------------------------------------
int mgx_rccl_unique_id(uint8_t id[128]) {
    if (!id) return fail(MGX_ERR_INVALID, "null argument");
    if (!g_rccl.load()) return fail(MGX_ERR_STATE, "RCCL is not available in this process");
    const int e = g_rccl.get_unique_id(id);
    if (e) return fail(MGX_ERR_HIP, "ncclGetUniqueId: %s", g_rccl.error_string ? g_rccl.error_string(e) : "error");
    return MGX_OK;
}
int mgx_halo_rccl_connect(mgx_world *w, const uint8_t id[128], uint32_t n_ranks, uint32_t rank, uint32_t n_peers, const uint32_t *peer_rank,
                          const uint32_t *send_first, const uint32_t *recv_first) {
    MGX_ENTER(w);
    if (!w || !id || (n_peers && (!peer_rank || !send_first || !recv_first))) return fail(MGX_ERR_INVALID, "null argument");
    if (rank >= n_ranks) return fail(MGX_ERR_INVALID, "rank out of range");
    if (!g_rccl.load()) return fail(MGX_ERR_STATE, "RCCL is not available in this process");
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    mgx_world::RcclHalo &rh = w->rccl;
    if (n_peers && (send_first[0] != 0 || send_first[n_peers] != w->halo_send.size() || recv_first[0] != 0 || recv_first[n_peers] != w->halo_recv.size()))
        return fail(MGX_ERR_INVALID, "segments do not cover the send / receive lists");
    for (uint32_t p = 0; p < n_peers; p++)
        if (peer_rank[p] >= n_ranks || peer_rank[p] == rank) return fail(MGX_ERR_INVALID, "bad peer rank");
    if (!rh.comm) {
        RcclApi::Id128 uid;
        memcpy(uid.internal, id, 128);
        const int e = g_rccl.comm_init_rank(&rh.comm, (int)n_ranks, uid, (int)rank);  // collective: every rank calls it
        if (e) { rh.comm = nullptr; return fail(MGX_ERR_HIP, "ncclCommInitRank: %s", g_rccl.error_string ? g_rccl.error_string(e) : "error"); }
    }
    const size_t words = (size_t)mgx_halo_words((uint32_t)w->K);
    HIP_TRY(rh.send_buf.reserve(std::max<size_t>(w->halo_send.size() * words, 1)));
    HIP_TRY(rh.recv_buf.reserve(std::max<size_t>(w->halo_recv.size() * words, 1)));
    rh.peer_rank.assign(peer_rank, peer_rank + n_peers);
    rh.send_first.assign(send_first, send_first + n_peers + (n_peers ? 1 : 0));
    rh.recv_first.assign(recv_first, recv_first + n_peers + (n_peers ? 1 : 0));
    rh.connected = true;
    return MGX_OK;
}
int mgx_halo_rccl_disconnect(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->rccl.connected = false;
    return MGX_OK;
}

// ---- direct halo exchange (peer-mapped stores, SURVEY §8e) ---------------------------------------------
// The exchange is wired ONCE (include/mgx.h) and outlives changes of the exchange lists: the receive area holds `slot_capacity` record
// slots per parity, slot g = the g-th ghost robot of this rank in device order (mgx_halo_ghost_slots); its `n_sources` producers are
// the ranks it shares a boundary with (fixed lists) or every other rank (a world that follows its topology) — with or without
// records in a given exchange.
int mgx_halo_direct_setup_slots(mgx_world *w, uint32_t n_sources, uint32_t slot_capacity, void **recv_base, void **flag_base) {
    MGX_ENTER(w);
    if (!w || !recv_base || !flag_base) return fail(MGX_ERR_INVALID, "null argument");
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    const size_t NG = (size_t)(w->d.R_total - w->d.R_local);
    if ((size_t)slot_capacity < NG) return fail(MGX_ERR_INVALID, "%u slots for %zu ghost robots", slot_capacity, NG);
    mgx_world::DirectHalo &dh = w->direct;
    HIP_TRY(hipStreamSynchronize(w->stream));
    dh.connected = false;
    if (dh.recv) { (void)hipFree(dh.recv); dh.recv = nullptr; }
    if (dh.flags) { (void)hipFree(dh.flags); dh.flags = nullptr; }
    dh.aimed = false;
    dh.slot_cap = slot_capacity;
    dh.recv_words = (size_t)slot_capacity * (size_t)mgx_halo_words((uint32_t)w->K);
    dh.n_sources = (int)n_sources;
    const size_t rb = std::max<size_t>(2 * dh.recv_words, 1) * sizeof(double), fb = ((size_t)n_sources + 1) * sizeof(unsigned long long);
    // fine-grained: coherent with stores arriving from other GPUs / processes while kernels run
    HIP_TRY(hipExtMallocWithFlags((void **)&dh.recv, rb, hipDeviceMallocFinegrained));
    HIP_TRY(hipExtMallocWithFlags((void **)&dh.flags, fb, hipDeviceMallocFinegrained));
    HIP_TRY(hipMemsetAsync(dh.recv, 0, rb, w->stream));
    HIP_TRY(hipMemsetAsync(dh.flags, 0, fb, w->stream));
    {
        std::vector<unsigned long long> z(1, 0ull);
        HIP_TRY(dh.ready.upload(z, w->stream));
    }
    HIP_TRY(hipStreamSynchronize(w->stream));
    if (w->sweep_err_host) *w->sweep_err_host = 0ull;  // a freshly wired exchange starts clean
    dh.seq = dh.push_seq = 0;
    if (const char *ms = getenv("MGX_HALO_TIMEOUT_MS")) {
        const long long v = atoll(ms);
        if (v > 0) dh.timeout_ticks = v * 100000ll;
    }
    *recv_base = dh.recv;
    *flag_base = dh.flags;
    return MGX_OK;
}

// slot of every listed robot among this rank's ghosts (-1: not a ghost here) — what the robot's owner stores its record into
int mgx_halo_ghost_slots(mgx_world *w, uint32_t n, const int32_t *robots, int32_t *slots) {
    MGX_ENTER(w);
    if (!w || (n && (!robots || !slots))) return fail(MGX_ERR_INVALID, "null argument");
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    for (uint32_t i = 0; i < n; i++) {
        const int32_t g = robots[i];
        if (g < 0 || (size_t)g >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad robot id %d", g);
        slots[i] = w->robots[(size_t)g].ghost ? w->dev_of[(size_t)g] - w->d.R_local : -1;
    }
    return MGX_OK;
}

// (Re)aim the pushes after the exchange lists changed (mgx_halo_plan / mgx_halo_plan_from_connections): peers in the order of the
// send list's segments — an empty segment for a peer that takes nothing now — and for every entry of the send list the slot of
// that robot in its consumer's area.  The exchange numbers go on: both ends keep counting.
int mgx_halo_direct_connect_slots(mgx_world *w, uint32_t n_peers, const uint32_t *send_first, void *const *peer_recv_base,
                                  const uint64_t *peer_slot_capacity, const uint32_t *entry_slot, void *const *peer_flag_slot) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::DirectHalo &dh = w->direct;
    if (!dh.flags) return fail(MGX_ERR_STATE, "mgx_halo_direct_setup_slots first");
    if (n_peers && (!send_first || !peer_recv_base || !peer_slot_capacity || !peer_flag_slot)) return fail(MGX_ERR_INVALID, "null argument");
    if ((int)n_peers != dh.n_sources)
        return fail(MGX_ERR_INVALID, "%u consumers but %d producers: the exchange must be symmetric (every peer both sends and receives)",
                    n_peers, dh.n_sources);
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    const size_t n_send = w->halo_send.size(), words = (size_t)mgx_halo_words((uint32_t)w->K);
    if ((size_t)(w->d.R_total - w->d.R_local) > dh.slot_cap)
        return fail(MGX_ERR_STATE, "%d ghost robots but the receive area has %zu slots: mgx_halo_direct_setup_slots again (on every rank)",
                    w->d.R_total - w->d.R_local, dh.slot_cap);
    if (n_peers && (send_first[0] != 0 || send_first[n_peers] != n_send)) return fail(MGX_ERR_INVALID, "send_first does not cover the send list");
    if (n_send && !entry_slot) return fail(MGX_ERR_INVALID, "null argument");
    std::vector<unsigned long long> d0(std::max<size_t>(n_send, 1), 0ull), d1(std::max<size_t>(n_send, 1), 0ull), pf(std::max<size_t>(n_peers, 1), 0ull);
    for (uint32_t p = 0; p < n_peers; p++) {
        if (send_first[p + 1] < send_first[p]) return fail(MGX_ERR_INVALID, "send_first is not ascending");
        if (!peer_recv_base[p] || !peer_flag_slot[p]) return fail(MGX_ERR_INVALID, "peer %u: null address", p);
        const unsigned long long base = (unsigned long long)(uintptr_t)peer_recv_base[p];
        for (uint32_t i = send_first[p]; i < send_first[p + 1]; i++) {
            if ((uint64_t)entry_slot[i] >= peer_slot_capacity[p]) return fail(MGX_ERR_INVALID, "entry %u: slot %u beyond the peer's %llu", i, entry_slot[i], (unsigned long long)peer_slot_capacity[p]);
            d0[i] = base + (0ull * peer_slot_capacity[p] + entry_slot[i]) * words * sizeof(double);
            d1[i] = base + (1ull * peer_slot_capacity[p] + entry_slot[i]) * words * sizeof(double);
        }
        pf[p] = (unsigned long long)(uintptr_t)peer_flag_slot[p];
    }
    HIP_TRY(dh.dst[0].upload(d0, w->stream));
    HIP_TRY(dh.dst[1].upload(d1, w->stream));
    HIP_TRY(dh.peer_flags.upload(pf, w->stream));
    if (!dh.connected) {
        std::vector<unsigned int> zero(1, 0u);
        HIP_TRY(dh.done.upload(zero, w->stream));
    }
    HIP_TRY(hipStreamSynchronize(w->stream));
    dh.n_peers = (int)n_peers;
    dh.connected = true;
    dh.aimed = true;
    return MGX_OK;
}

int mgx_halo_direct_exchange(mgx_world *w, uint32_t what) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (!w->direct.connected) return fail(MGX_ERR_STATE, "direct halo exchange is not connected");
    if (what == MGX_HALO_PUSH) return direct_push(w);
    if (what == MGX_HALO_WAIT) return direct_wait(w);
    if (what == (MGX_HALO_PUSH | MGX_HALO_WAIT)) return direct_exchange(w);
    return fail(MGX_ERR_INVALID, "bad phase mask");
}

int mgx_halo_direct_status(mgx_world *w, uint64_t *exchanges, uint64_t *failed_exchange) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    mgx_world::DirectHalo &dh = w->direct;
    if (!dh.flags) return fail(MGX_ERR_STATE, "direct halo exchange is not set up");
    unsigned long long err = 0;
    HIP_TRY(hipStreamSynchronize(w->stream));
    HIP_TRY(hipMemcpy(&err, dh.flags + dh.n_sources, sizeof err, hipMemcpyDeviceToHost));
    if (exchanges) *exchanges = dh.seq;
    if (failed_exchange) *failed_exchange = err;
    if (err) return fail(MGX_ERR_STATE, "halo exchange %llu timed out waiting for a peer", err);
    return MGX_OK;
}

int mgx_halo_direct_disconnect(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->direct.connected = false;
    return MGX_OK;
}

// ---- resident schedule launches on sharded worlds (include/mgx.h) -----------------------------------------
// Layout of a ghost area for NG ghost slots of K variables: the agreement word's line, exchange records of parity 0, of parity 1
// (NG * K * XREC_BYTES each: mgx_dev.h), NG progress words.  Both ends compute it.
namespace {
struct GhostAreaLayout {
    static constexpr size_t agree = 0, HEAD = 64;  // the ranks' agreement word (used in rank 0's area only) has the first line to itself
    size_t xrec[2], flag, bytes;
    GhostAreaLayout(size_t ng, size_t K) {
        const size_t S = ng * K * (size_t)XREC_BYTES;
        xrec[0] = HEAD; xrec[1] = HEAD + S;
        flag = HEAD + 2 * S;
        bytes = flag + std::max<size_t>(ng, 1) * sizeof(unsigned long long);
    }
};
}  // namespace

int mgx_halo_resident_setup(mgx_world *w, void **area_base, uint32_t *n_ghost_slots, uint32_t *parity, uint64_t *segment_count,
                            int32_t *recv_slots, int32_t *eligible) {
    MGX_ENTER(w);
    if (!w || !area_base || !n_ghost_slots || !parity || !segment_count || !eligible) return fail(MGX_ERR_INVALID, "null argument");
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    if (w->conns_dirty || w->flags_dirty) { rc = commit(w); if (rc != MGX_OK) return rc; }
    if (!w->halo_recv.empty() && !recv_slots) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::ResidentHalo &xr = w->xres;
    HIP_TRY(hipStreamSynchronize(w->stream));
    // The area (rank 0's also holds the agreement word) may still be mapped by the peers, whose launches store into it: a layout
    // change only switches THIS rank's launches off (commit).  It is given back only after a disconnect — which every rank runs
    // behind a barrier, before any of them sets up again (include/mgx.h; sharded.rewire_resident).
    if (xr.area && xr.wired)
        return fail(MGX_ERR_STATE, "mgx_halo_resident_setup: the ghost area of the previous wiring is still connected; call "
                    "mgx_halo_resident_disconnect on every rank (behind a barrier) first");
    xr.connected = false;
    xr.agree = nullptr;
    w->d.agree = nullptr;
    if (xr.area) { (void)hipFree(xr.area); xr.area = nullptr; }
    const DevWorld &d = w->d;
    const int NG = d.R_total - d.R_local;
    // can this rank run its schedules as resident launches at all?
    const bool has_factors = d.ir_max_edges > 0 && !w->conns.empty();
    bool ok = resident_enabled() && (w->p.enable_mask & 2u) && sweep_lds_bytes(w->K, d.ir_max_edges, true) <= sweep_resident_lds_max();
    if (ok && has_factors) {
        ok = d.R_local + 1 <= w->res.capacity_for(d, true, SWEEP_F_ALL);  // (+ the launch's decider workgroup; every launch asks its own form again)
    }
    rc = ensure_resident_tables(w);  // settles this rank's segment count (progress words are created here)
    if (rc != MGX_OK) return rc;
    const GhostAreaLayout L((size_t)NG, (size_t)w->K);
    // fine-grained: coherent with stores arriving from other GPUs / processes while kernels run
    HIP_TRY(hipExtMallocWithFlags(&xr.area, L.bytes, hipDeviceMallocFinegrained));
    xr.bytes = L.bytes;
    xr.n_ghosts = NG;
    HIP_TRY(hipMemsetAsync(xr.area, 0, L.bytes, w->stream));
    {   // every ghost "has completed" what this rank's segment count says: nothing of an earlier launch is still being read
        std::vector<unsigned long long> f((size_t)std::max(NG, 1), w->res.flag_base);
        HIP_TRY(hipMemcpyAsync((char *)xr.area + L.flag, f.data(), sizeof(unsigned long long) * f.size(), hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    for (size_t i = 0; i < w->halo_recv.size(); i++) recv_slots[i] = w->dev_of[(size_t)w->halo_recv[i]] - d.R_local;
    *area_base = xr.area;
    *n_ghost_slots = (uint32_t)NG;
    *parity = (uint32_t)d.cur;
    *segment_count = w->res.flag_base;
    // 2: everything but inter-robot factors is there — a world that follows its topology may get them later (every schedule is then
    // decided where the ranks agree: a rank that cannot run one as a resident launch says so there)
    *eligible = ok ? (has_factors ? 1 : 2) : 0;
    return MGX_OK;
}

// The wiring outlives the exchange lists: the peers ONCE — every peer's ghost area, its number of ghost slots, its buffer parity and
// segment count as ITS setup returned them — and, after every change of the lists, which local robot's records go into which slot
// of which peer (mgx_halo_resident_aim).
int mgx_halo_resident_connect_peers(mgx_world *w, uint32_t n_peers, void *const *peer_area_base, const uint32_t *peer_ghost_slots,
                                    const uint32_t *peer_parity, const uint64_t *peer_segment_count, void *coordinator_area, uint32_t n_ranks) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (n_ranks > 0x3fffu) return fail(MGX_ERR_INVALID, "at most %u ranks", 0x3fffu);  // (the agreement word counts them in 14 bits)
    if (n_peers && (!peer_area_base || !peer_ghost_slots || !peer_parity || !peer_segment_count)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::ResidentHalo &xr = w->xres;
    if (!xr.area) return fail(MGX_ERR_STATE, "mgx_halo_resident_setup first");
    if (!w->dev_valid || w->dirty) return fail(MGX_ERR_STATE, "the world's layout changed since mgx_halo_resident_setup");
    DevWorld &d = w->d;
    xr.peers.assign(n_peers, mgx_world::ResidentHalo::Peer());
    for (uint32_t p = 0; p < n_peers; p++) {
        if (!peer_area_base[p] || peer_parity[p] > 1u) return fail(MGX_ERR_INVALID, "peer %u: bad area / parity", p);
        xr.peers[p].base = (unsigned long long)(uintptr_t)peer_area_base[p];
        xr.peers[p].n_slots = peer_ghost_slots[p];
        xr.peers[p].x = ((unsigned)d.cur ^ peer_parity[p]) & 1u;
        xr.peers[p].flag_delta = peer_segment_count[p] - w->res.flag_base;  // modulo 2^64
    }
    const GhostAreaLayout Lm((size_t)xr.n_ghosts, (size_t)w->K);
    for (int p = 0; p < 2; p++) d.gxrec[p] = (const unsigned char *)xr.area + Lm.xrec[p];
    d.gflag = (const unsigned long long *)((const char *)xr.area + Lm.flag);
    xr.agree = coordinator_area && n_ranks >= 2 ? (unsigned long long *)((char *)coordinator_area + GhostAreaLayout::agree) : nullptr;
    xr.n_ranks = xr.agree ? (int)n_ranks : 0;
    xr.agree_seq = 0;
    d.agree = xr.agree;
    d.n_ranks = xr.n_ranks;
    xr.connected = true;
    xr.wired = true;
    return mgx_halo_resident_aim(w, 0, nullptr, nullptr, nullptr);
}

// n_targets entries (local robot, index of the peer in mgx_halo_resident_connect_peers' order, the robot's ghost slot there).  Call
// on every rank after a change of the lists, with every rank's launches through (the callers synchronise and meet at a barrier):
// the progress words of this rank's ghosts start over at "through with everything so far" — a robot that becomes somebody's
// neighbour across ranks has never stored one here.
int mgx_halo_resident_aim(mgx_world *w, uint32_t n_targets, const int32_t *robots, const uint32_t *peer_index, const uint32_t *peer_slot) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    if (n_targets && (!robots || !peer_index || !peer_slot)) return fail(MGX_ERR_INVALID, "null argument");
    mgx_world::ResidentHalo &xr = w->xres;
    if (!xr.area || !xr.connected) return fail(MGX_ERR_STATE, "mgx_halo_resident_connect_peers first");
    MGX_CONFIRM(w);
    if (!w->dev_valid || w->dirty) return fail(MGX_ERR_STATE, "the world's layout changed since mgx_halo_resident_setup");
    const DevWorld &d = w->d;
    const size_t R = (size_t)d.R_local, K = (size_t)w->K;
    std::vector<std::pair<int, XPushRec>> recs;
    recs.reserve(n_targets);
    for (uint32_t t = 0; t < n_targets; t++) {
        if (robots[t] < 0 || (size_t)robots[t] >= w->robots.size() || w->robots[(size_t)robots[t]].ghost)
            return fail(MGX_ERR_INVALID, "target %u: robot %d is not a local robot", t, robots[t]);
        if ((size_t)peer_index[t] >= xr.peers.size()) return fail(MGX_ERR_INVALID, "target %u: peer %u of %zu", t, peer_index[t], xr.peers.size());
        const mgx_world::ResidentHalo::Peer &pr = xr.peers[(size_t)peer_index[t]];
        if ((size_t)peer_slot[t] >= pr.n_slots) return fail(MGX_ERR_INVALID, "target %u: slot %u of %zu", t, peer_slot[t], pr.n_slots);
        const GhostAreaLayout L(pr.n_slots, K);
        XPushRec r;
        for (unsigned p = 0; p < 2; p++) r.xrec[p] = pr.base + L.xrec[p ^ pr.x] + (size_t)peer_slot[t] * K * (size_t)XREC_BYTES;
        r.flag = pr.base + L.flag + (size_t)peer_slot[t] * sizeof(unsigned long long);
        r.flag_delta = pr.flag_delta;
        recs.emplace_back(w->dev_of[(size_t)robots[t]], r);
    }
    std::stable_sort(recs.begin(), recs.end(), [](const std::pair<int, XPushRec> &a, const std::pair<int, XPushRec> &b) { return a.first < b.first; });
    std::vector<int32_t> ptr(R + 1, 0);
    std::vector<XPushRec> flat(std::max<size_t>(recs.size(), 1));
    for (size_t i = 0; i < recs.size(); i++) { ptr[(size_t)recs[i].first + 1]++; flat[i] = recs[i].second; }
    for (size_t r = 0; r < R; r++) ptr[r + 1] += ptr[r];
    HIP_TRY(hipStreamSynchronize(w->stream));
    HIP_TRY(xr.xp_ptr.upload(ptr, w->stream));
    HIP_TRY(xr.xp_rec.upload(flat, w->stream));
    {
        const GhostAreaLayout Lm((size_t)xr.n_ghosts, K);
        std::vector<unsigned long long> f((size_t)std::max(xr.n_ghosts, 1), w->res.flag_base);
        HIP_TRY(hipMemcpyAsync((char *)xr.area + Lm.flag, f.data(), sizeof(unsigned long long) * f.size(), hipMemcpyHostToDevice, w->stream));
    }
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->d.xp_ptr = xr.xp_ptr.p;
    w->d.xp_rec = xr.xp_rec.p;
    return MGX_OK;
}

int mgx_halo_resident_disconnect(mgx_world *w) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    MGX_CONFIRM(w);
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->xres.connected = false;
    w->xres.wired = false;
    w->xres.peers.clear();
    w->xres.agree = nullptr;
    w->d.agree = nullptr;
    return MGX_OK;
}

int mgx_resident_outcome(mgx_world *w, int32_t *outcome) {
    MGX_ENTER_SCHEDULE(w);  // (a query: a launch that lingers stays — and its verdict is still there to be asked for)
    if (!w || !outcome) return fail(MGX_ERR_INVALID, "null argument");
    return confirm_resident(w, false, outcome);
}

int mgx_resident_ready(mgx_world *w, const uint8_t *steps, uint32_t n, int32_t *ready) {
    MGX_ENTER(w);
    if (!w || !ready || (!steps && n)) return fail(MGX_ERR_INVALID, "null argument");
    int rc = commit(w);
    if (rc != MGX_OK) return rc;
    *ready = resident_gate(w, plan_launches(steps, n)) ? 1 : 0;
    if (*ready && !(w->xres.connected && w->xres.agree)) {  // nobody to agree with: what this world's own launch needs
        *ready = resident_fits(w, w->xres.connected, resident_features(w, false)) == FITS ? 1 : 0;
    }
    return MGX_OK;
}

int mgx_resident_stats(mgx_world *w, uint64_t *launches, uint64_t *declined, uint32_t *backoff) {
    MGX_ENTER_SCHEDULE(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    MGX_CONFIRM(w);
    if (launches) *launches = w->res.launches;
    if (declined) *declined = w->res.aborts;
    if (backoff) *backoff = (uint32_t)w->res.backoff.left;
    return MGX_OK;
}

// hipIpc* wrappers so that a host language needs no HIP binding of its own to share the areas
int mgx_ipc_export(const void *dev_ptr, uint8_t handle[64]) {
    if (!dev_ptr || !handle) return fail(MGX_ERR_INVALID, "null argument");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "handle size");
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, const_cast<void *>(dev_ptr)));
    memcpy(handle, &h, 64);
    return MGX_OK;
}
int mgx_ipc_open(const uint8_t handle[64], void **dev_ptr) {
    if (!handle || !dev_ptr) return fail(MGX_ERR_INVALID, "null argument");
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, 64);
    HIP_TRY(hipIpcOpenMemHandle(dev_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return MGX_OK;
}
int mgx_ipc_close(void *dev_ptr) {
    if (!dev_ptr) return MGX_OK;
    HIP_TRY(hipIpcCloseMemHandle(dev_ptr));
    return MGX_OK;
}

int mgx_halo_pack(mgx_world *w, void *dev_buf) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    if (w->halo_send.empty()) return MGX_OK;
    if (!dev_buf) return fail(MGX_ERR_INVALID, "null buffer");
    HIP_TRY(launch_halo_pack(w->d, (int)w->halo_send.size(), w->halo_send_dev.p, (double *)dev_buf, w->stream));
    return MGX_OK;
}
int mgx_halo_unpack(mgx_world *w, const void *dev_buf) {
    MGX_ENTER(w);
    if (!w) return fail(MGX_ERR_INVALID, "null world");
    int rc = halo_commit(w);
    if (rc != MGX_OK) return rc;
    if (w->halo_recv.empty()) return MGX_OK;
    if (!dev_buf) return fail(MGX_ERR_INVALID, "null buffer");
    HIP_TRY(launch_halo_unpack(w->d, (int)w->halo_recv.size(), w->halo_recv_dev.p, (const double *)dev_buf, w->stream));
    return MGX_OK;
}

#ifdef MGX_STAMPS
// diagnostic build only: copy the per-wave phase cycle sums to the host
int mgx_debug_read_stamps(mgx_world *w, unsigned long long *out, uint32_t n) {
    MGX_ENTER(w);
    if (!w || !out) return fail(MGX_ERR_INVALID, "null argument");
    std::vector<unsigned long long> h;
    HIP_TRY(w->dbg.download(h, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    for (uint32_t i = 0; i < n && i < h.size(); i++) out[i] = h[i];
    return (int)h.size();
}
#endif

}  // extern "C"
