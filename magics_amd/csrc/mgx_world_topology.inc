// mgx_world_topology.inc — C ABI: dynamic inter-robot topology — neighbour search, delete / create_interrobot_factors.
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
extern "C" {
// ---- dynamic inter-robot topology (robot.rs:1362-1586) -----------------------------------------------

// The fine-grained calls keep robots_connected_with in step, as create_/delete_interrobot_factors
// do (robot.rs:1406-1408,1546), so that they can be mixed with mgx_update_topology.
int mgx_ir_connect(mgx_world *w, int32_t owner, int32_t other, uint64_t first_robot_number) {
    MGX_ENTER(w);
    int rc = ir_connect(w, owner, other, first_robot_number);
    if (rc != MGX_OK) return rc;
    w->search.sets_touched();
    if (!w->sets.has((size_t)owner, other)) w->sets.insert_sorted((size_t)owner, other);
    return MGX_OK;
}
int mgx_ir_disconnect(mgx_world *w, int32_t a, int32_t b) {
    MGX_ENTER(w);
    int rc = ir_disconnect(w, a, b);
    if (rc != MGX_OK) return rc;
    w->search.sets_touched();
    w->sets.erase((size_t)a, b);
    w->sets.erase((size_t)b, a);
    return MGX_OK;
}

// device neighbour search -> host CSR, rows ascending in order key
// pos == nullptr: the positions come from the device-resident Transforms of the missions (mgx_mission_tick)
// Two halves: everything that is enqueued (neighbours_enqueue) and, behind a synchronisation of the stream, the host side
// (neighbours_collect: once more with room if the rows outgrew it, ids and order).  Two strategies (mgx_search.h,
// search_kernel_for): the one-pass kernels read and write a mapped pinned block in place (rows_*), the two-pass count / scan /
// fill search works with device scratch and a guessed buffer (csr_*).
// mgx_mission_tick enqueues the search of the NEXT tick in front of this tick's GBP schedule — the Transforms it looks at are
// final once the prior updates have moved them — so its rows are on the host long before that tick's one synchronisation.
using PendingSearch = NeighbourSearch::PendingSearch;

// the positions of a mission's search: the Transforms of the robots in the query, on the device
static int mission_positions(mgx_world *w, PendingSearch &ps) {
    mgx_world::Mission &ms = w->mission;
    if (ms.alive_dirty || ms.alive_host.size() != ps.alive.size()) {
        ms.alive_host.assign(ps.alive.begin(), ps.alive.end());
        if (ms.alive_host.empty()) ms.alive_host.push_back(0);
        HIP_TRY(ms.alive_d.upload(ms.alive_host, ps.stream));
        HIP_TRY(hipStreamSynchronize(ps.stream));
        ms.alive_host.resize(ps.alive.size());
        ms.alive_dirty = false;
    }
    HIP_TRY(launch_mission_positions(ms.d, ps.n, ms.alive_d.p, w->search.pos.p, ps.stream));
    return MGX_OK;
}
// what both strategies start with: who is in the query, on which stream, ordered against the search before; the positions of
// a mission's search.  *pos: the caller's positions, compacted where robots have left the query
static int search_front(mgx_world *w, const float **pos, float radius, uint32_t method, PendingSearch &ps, const float *radii = nullptr,
                        uint32_t n_radii = 0) {
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    NeighbourSearch &S = w->search;
    S.mission.valid = false;  // the buffers below are shared: whatever was waiting in them is gone
    ps.valid = false;
    ps.n_all = (int)w->robots.size();
    ps.from_missions = *pos == nullptr;
    ps.radius = radius;
    if (radii) ps.radii.assign(radii, radii + n_radii);  // (may be the ones ps holds already: mgx_mission_tick_end's)
    else ps.radii.clear();
    ps.method = method;
    std::vector<int> &alive = ps.alive;  // removed robots are in no query: search the others, map back
    alive.clear();
    for (int r = 0; r < ps.n_all; r++) {
        // ghosts take part: a sharded world that follows a changing topology holds EVERY robot of the
        // scenario (its own ones and ghost copies of all others) and is handed all positions, so that
        // the connection bookkeeping below runs identically on every rank
        if (!w->sets.removed[(size_t)r]) alive.push_back(r);
    }
    const int n = ps.n = (int)alive.size();
    ps.compact = n != ps.n_all;
    if (ps.compact && !ps.from_missions) {
        S.packed.resize(3 * alive.size());
        for (size_t a = 0; a < alive.size(); a++) memcpy(&S.packed[3 * a], *pos + 3 * (size_t)alive[a], 3 * sizeof(float));
        *pos = S.packed.data();
    }
    S.last_launches = 0;
    S.last_changed = -1;  // (until flags reach a pass: topology_bookkeeping)
    // A search over positions the CALLER hands in reads nothing of the world's device state: it runs on a stream of its own,
    // next to whatever the world's stream is still busy with (the previous tick's GBP schedule), instead of behind it.
    // (The missions' search reads the device's Transforms, which the tick's kernels move: that one stays in stream order.)
    ps.stream = w->stream;
    if (!ps.from_missions) {
        // Never beside a resident launch that is still getting onto the device: the search's workgroups would take slots the
        // launch's last workgroups need — the census says no and a handful of ticks run launch by launch (a thousand robots
        // leave two or three free slots per XCD; enqueued at once "when both fit" the search still cost every third launch its
        // residency: tools/dynamic_tick_bench.py, 27 of 90 launches declined, 4.2 k ticks/s against 5.9 k behind the decision).
        // Behind a DECIDED launch the search finds the holes that launch leaves (mgx_topology.hip) and runs beside it.
        MGX_CONFIRM(w);
        if (!S.stream) HIP_TRY(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
        ps.stream = S.stream;
    }
    if (S.last_stream_set && S.last_stream != ps.stream) HIP_TRY(hipStreamSynchronize(S.last_stream));  // the scratch buffers are shared
    S.last_stream = ps.stream;
    S.last_stream_set = true;
    HIP_TRY(S.pos.reserve((size_t)3 * std::max(n, 1)));
    return ps.from_missions ? mission_positions(w, ps) : MGX_OK;
}

// ---- one pass: rows of a fixed capacity, written in place (small worlds, AUTO) --------------------------------------------------
// ONE launch of the kernel for rows of `cap` entries.  No copies at all: the kernel reads the callers' positions from the pinned
// block and writes counts and rows into it (a copy is a launch of its own — a blit kernel too big to find room beside a resident
// schedule launch).  host_pos (may be null): positions to put into the block first — null where they are in it already (a
// search that runs again: what the block holds moves along when it grows) or on the device (a mission's).
// prev (may be null): the kept rows, for the kernel to compare with and to overwrite
static int rows_launch(mgx_world *w, PendingSearch &ps, int cap, const float *host_pos, int32_t *prev, int prev_valid) {
    NeighbourSearch &S = w->search;
    const RowsLayout at = rows_layout(ps.n, cap);
    HIP_TRY(S.pin.reserve(at.bytes, host_pos || ps.from_missions ? 0 : at.off_cnt));
    if (host_pos) memcpy(S.pin.p, host_pos, at.off_cnt);
    void *dpin = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dpin, S.pin.p, 0));
    char *dp = static_cast<char *>(dpin);
    ps.rows.cap = cap;
    if (ps.grouped) {  // a grouped world: its one kernel, over the query listed by group (groups_prepare)
        const GroupTables &g = S.groups;
        ps.rows.has_chg = false;
        HIP_TRY(neighbours_rows_groups(ps.from_missions ? S.pos.p : reinterpret_cast<const float *>(dp), ps.n, S.groups_d.p, S.groups_d.p + g.off_seg(),
                                       S.groups_d.p + g.off_wg(), g.n_workgroups(), g.largest, reinterpret_cast<const float *>(S.groups_d.p + g.off_thr()),
                                       cap, reinterpret_cast<int32_t *>(dp + at.off_cnt),
                                       reinterpret_cast<int32_t *>(dp + at.off_rows), ps.stream, &S.last_kernel));
    } else {
        HIP_TRY(neighbours_rows(ps.from_missions ? S.pos.p : reinterpret_cast<const float *>(dp), ps.n, ps.radius, cap,
                                reinterpret_cast<int32_t *>(dp + at.off_cnt), reinterpret_cast<int32_t *>(dp + at.off_rows), ps.stream, prev,
                                prev_valid, &ps.rows.has_chg, &S.last_kernel));
    }
    S.last_cap = cap;
    S.last_launches++;
    return MGX_OK;
}
// keep_rows: the search of a topology pass over the caller's positions, by a kernel that can compare every robot's row with the
// one it got in the pass before (NeighbourSearch::prev) and say which ones changed
static int rows_enqueue(mgx_world *w, const float *pos, PendingSearch &ps, bool keep_rows) {
    NeighbourSearch &S = w->search;
    int prev_valid = 0;
    if (keep_rows) {
        const size_t words = (size_t)ps.n * (size_t)NEIGHBOURS_PREV_STRIDE;
        if (S.prev.cap < words || S.prev_n != (size_t)ps.n) {  // (the world's robots are not the ones of the last pass: nothing is kept)
            HIP_TRY(S.prev.reserve(words));
            S.prev_n = (size_t)ps.n;
            S.prev_valid = false;
        }
        prev_valid = S.prev_valid ? 1 : 0;
        S.prev_valid = false;  // (the kernel overwrites the kept rows: they are the sets again when the pass has gone through)
    }
    HIP_TRY(S.idx.reserve((size_t)ps.n * (size_t)S.row_cap));  // (a two-pass search behind this one fills into it on a guess)
    return rows_launch(w, ps, S.row_cap, pos, keep_rows ? S.prev.p : nullptr, prev_valid);
}
// chg (may be null): where to put the pointer to the rows-changed bytes of the search, or null if it has none — then only the rows
// of robots whose byte is set are copied into idx (the others' entries are not to be read)
static int rows_collect(mgx_world *w, PendingSearch &ps, std::vector<int32_t> &ptr, std::vector<int32_t> &idx, const uint8_t **chg) {
    NeighbourSearch &S = w->search;
    const int n = ps.n;
    RowsLayout at = rows_layout(n, ps.rows.cap);
    int32_t *cnt = reinterpret_cast<int32_t *>(static_cast<char *>(S.pin.p) + at.off_cnt);
    if (ps.rows.has_chg) {  // the flags out of the counts (the pinned block is the host's to write)
        S.chg.resize((size_t)n);
        strip_changed(cnt, n, S.chg.data());
    }
    int32_t longest = 0;
    for (int i = 0; i < n; i++) longest = std::max(longest, cnt[i]);
    if (longest > ps.rows.cap) {  // a row outgrew its capacity: once more with room (the world remembers)
        int cap = ps.rows.cap;
        while (cap < longest) cap *= 2;
        S.row_cap = cap;
        // (no kept rows, no flags: they were half written by the search that did not fit — everybody counts as changed)
        const int rc = rows_launch(w, ps, cap, nullptr, nullptr, 0);
        if (rc != MGX_OK) return rc;
        HIP_TRY(hipStreamSynchronize(ps.stream));
        at = rows_layout(n, ps.rows.cap);
        cnt = reinterpret_cast<int32_t *>(static_cast<char *>(S.pin.p) + at.off_cnt);
    }
    // flags reach the pass only where it can go by them: nobody left the query, and ids ascending == keys ascending (rows that are
    // sorted by key below are all needed)
    const uint8_t *changed = (chg && ps.rows.has_chg && !ps.compact && w->sets.monotone()) ? S.chg.data() : nullptr;
    static const bool check_index = getenv("MGX_CHECK_INDEX") != nullptr;  // (diagnostics: every row is there for the pass to verify)
    rows_to_csr(cnt, reinterpret_cast<const int32_t *>(static_cast<char *>(S.pin.p) + at.off_rows), n, ps.rows.cap, check_index ? nullptr : changed,
                ptr, idx);
    if (chg) *chg = changed;
    S.last_total = idx.size();
    return MGX_OK;
}

// ---- two passes: count, scan, fill ----------------------------------------------------------------------------------------------
static int csr_enqueue(mgx_world *w, const float *pos, PendingSearch &ps, bool grid) {
    NeighbourSearch &S = w->search;
    const int n = ps.n;
    uint32_t M = 64;  // buckets of the grid: a power of two, at least two per robot
    while (M < 2u * (uint32_t)std::max(n, 1)) M <<= 1;
    HIP_TRY(S.cnt.reserve((size_t)std::max(n, 1)));
    HIP_TRY(S.ptr.reserve((size_t)n + 1));
    HIP_TRY(S.members.reserve((size_t)std::max(n, 1)));
    HIP_TRY(S.special.reserve((size_t)std::max(n, 1)));
    HIP_TRY(S.nspecial.reserve(1));
    HIP_TRY(S.bucket_cnt.reserve(M));
    HIP_TRY(S.bucket_ptr.reserve((size_t)M + 1));
    HIP_TRY(S.cursor.reserve(M));
    const size_t guess = std::min(S.idx.cap, S.last_total + S.last_total / 4 + 64);  // (0 while there is no buffer)
    // pinned layout: [3 n floats: positions up] [n + 1 ints: row pointers down] [guess ints: rows down]
    const size_t off_ptr = sizeof(float) * 3 * (size_t)std::max(n, 1), off_idx = off_ptr + sizeof(int32_t) * ((size_t)n + 1);
    HIP_TRY(S.pin.reserve(off_idx + sizeof(int32_t) * guess));
    char *pin = static_cast<char *>(S.pin.p);
    if (!ps.from_missions && n) {
        memcpy(pin, pos, sizeof(float) * 3 * (size_t)n);
        HIP_TRY(hipMemcpyAsync(S.pos.p, pin, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ps.stream));
    }
    HIP_TRY(neighbours_count(S.pos.p, n, ps.radius, grid, M, S.scratch(), ps.stream));
    if (n > 0) {  // (an empty query launches nothing)
        S.last_kernel = grid ? MGX_SEARCH_TWO_PASS_GRID : MGX_SEARCH_TWO_PASS_PAIRS;
        S.last_cap = 0;
        S.last_launches++;
    }
    // The second pass needs the total to size its output — one more host round trip.  Instead it runs right
    // away into the buffer left from the last search (the kernels leave it alone if the rows do not fit), and
    // rows and counts come back together; only a total beyond the guess costs the second trip.
    if (guess > 0) HIP_TRY(neighbours_fill(S.pos.p, n, ps.radius, grid, M, S.scratch(), S.idx.p, (int32_t)guess, ps.stream));
    HIP_TRY(hipMemcpyAsync(pin + off_ptr, S.ptr.p, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ps.stream));
    if (guess > 0) HIP_TRY(hipMemcpyAsync(pin + off_idx, S.idx.p, sizeof(int32_t) * guess, hipMemcpyDeviceToHost, ps.stream));
    ps.csr = {guess, off_ptr, off_idx, M, grid};
    return MGX_OK;
}
static int csr_collect(mgx_world *w, PendingSearch &ps, std::vector<int32_t> &ptr, std::vector<int32_t> &idx) {
    NeighbourSearch &S = w->search;
    const int n = ps.n;
    const char *pin = static_cast<const char *>(S.pin.p);
    ptr.assign((size_t)n + 1, 0);
    memcpy(ptr.data(), pin + ps.csr.off_ptr, sizeof(int32_t) * ((size_t)n + 1));
    const size_t total = (size_t)ptr[(size_t)n];
    S.last_total = total;
    if (total <= ps.csr.guess || total == 0) {
        idx.resize(total);
        if (total) memcpy(idx.data(), pin + ps.csr.off_idx, sizeof(int32_t) * total);
        return MGX_OK;
    }
    idx.assign(total, 0);
    if (n > 0 && ps.csr.guess > 0) S.last_launches++;  // (the filling pass ran into the guessed buffer: once more)
    HIP_TRY(S.idx.reserve(total));
    HIP_TRY(neighbours_fill(S.pos.p, n, ps.radius, ps.csr.grid, ps.csr.M, S.scratch(), S.idx.p, (int32_t)total, ps.stream));
    HIP_TRY(hipMemcpyAsync(idx.data(), S.idx.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, ps.stream));
    HIP_TRY(hipStreamSynchronize(ps.stream));
    return MGX_OK;
}

// A grouped world's query listed by group (GroupTables, mgx_search.h), on the device: built again only when robots have joined or
// left the query, the segments' thresholds also when a group's radius is not the one of the search before — then uploaded and
// waited for (the kernels of an earlier search on this stream have read the old tables by then).  Not per search: a search with
// the robots and the radii of the one before uploads nothing
static int groups_prepare(mgx_world *w, PendingSearch &ps) {
    NeighbourSearch &S = w->search;
    const float *radii = ps.radii.empty() ? nullptr : ps.radii.data();
    if (S.groups_valid && S.groups_alive == ps.alive) {
        if (!group_thresholds(S.groups, radii, ps.radii.size(), ps.radius)) return MGX_OK;
    } else {
        S.groups_valid = false;
        std::vector<uint32_t> of_query((size_t)ps.n);
        for (int q = 0; q < ps.n; q++) of_query[(size_t)q] = w->sets.group[(size_t)ps.alive[(size_t)q]];
        if (!group_tables(of_query.data(), ps.n, S.groups))
            return fail(MGX_ERR_INVALID, "a group of %d robots: the grouped search holds one group's positions in a workgroup's LDS, %d at the most",
                        S.groups.largest, ROWS_MAX_N);
        group_thresholds(S.groups, radii, ps.radii.size(), ps.radius);
    }
    S.groups_valid = false;
    const GroupTables &g = S.groups;
    S.groups_host.clear();
    S.groups_host.insert(S.groups_host.end(), g.members.begin(), g.members.end());
    S.groups_host.insert(S.groups_host.end(), g.seg.begin(), g.seg.end());
    S.groups_host.insert(S.groups_host.end(), g.wg.begin(), g.wg.end());
    S.groups_host.resize(g.words_with_thr());  // (the thresholds' bits)
    if (!g.thr.empty()) memcpy(S.groups_host.data() + g.off_thr(), g.thr.data(), sizeof(float) * g.thr.size());
    HIP_TRY(hipStreamSynchronize(ps.stream));  // (nothing reads the old tables any more)
    HIP_TRY(S.groups_d.upload(S.groups_host, ps.stream));
    HIP_TRY(hipStreamSynchronize(ps.stream));
    S.groups_alive = ps.alive;
    S.groups_valid = true;
    return MGX_OK;
}
// track: the search of a topology pass over the caller's positions (see rows_enqueue)
// radii (may be null) [n_radii]: one radius per group, for a grouped world's search; an ungrouped world's search is the scalar one
// with radii[0] — `radius` is that one then
static int neighbours_enqueue(mgx_world *w, const float *pos, float radius, uint32_t method, PendingSearch &ps, bool track = false,
                              const float *radii = nullptr, uint32_t n_radii = 0) {
    if (w->sets.n_grouped == 0) radii = nullptr;
    int rc = search_front(w, &pos, radius, method, ps, radii, radii ? n_radii : 0);
    if (rc != MGX_OK) return rc;
    ps.grouped = w->sets.n_grouped != 0 && ps.n > 0;
    const int32_t kernel = search_kernel_for(ps.n, method, radius, w->search.row_cap, ps.grouped);
    if (ps.grouped && (rc = groups_prepare(w, ps)) != MGX_OK) return rc;
    ps.in_rows = search_in_rows(kernel);
    // (the kept rows: where robots left the query, or the positions are a mission's, nothing is kept)
    rc = ps.in_rows ? rows_enqueue(w, pos, ps, track && !ps.compact && !ps.from_missions && search_keeps_rows(kernel))
                    : csr_enqueue(w, pos, ps, kernel == MGX_SEARCH_TWO_PASS_GRID);
    ps.valid = rc == MGX_OK;
    return rc;
}
static int neighbours_collect(mgx_world *w, PendingSearch &ps, std::vector<int32_t> &ptr, std::vector<int32_t> &idx,
                              const uint8_t **chg = nullptr) {
    if (chg) *chg = nullptr;
    ps.valid = false;
    HIP_TRY(hipStreamSynchronize(ps.stream));
    const int rc = ps.in_rows ? rows_collect(w, ps, ptr, idx, chg) : csr_collect(w, ps, ptr, idx);
    if (rc != MGX_OK) return rc;
    if (ps.compact) compact_to_world(ps.alive, ps.n_all, ptr, idx);  // back to world robot ids, empty rows for the removed ones
    if (!w->sets.monotone())  // ids ascending == keys ascending: nothing to do (the keys' compact copies: fixed when a robot is added)
        for (int r = 0; r < ps.n_all; r++)
            std::sort(idx.begin() + ptr[(size_t)r], idx.begin() + ptr[(size_t)r + 1],
                      [&](int a, int b) { return w->robots[(size_t)a].order_key < w->robots[(size_t)b].order_key; });
    return MGX_OK;
}
static int neighbours(mgx_world *w, const float *pos, float radius, uint32_t method, std::vector<int32_t> &ptr,
                      std::vector<int32_t> &idx, const float *radii = nullptr, uint32_t n_radii = 0) {
    PendingSearch ps;
    const int rc = neighbours_enqueue(w, pos, radius, method, ps, false, radii, n_radii);
    return rc != MGX_OK ? rc : neighbours_collect(w, ps, ptr, idx);
}

static int groups_radii_arguments(mgx_world *w, const float *radii, uint32_t n_groups);
static int neighbours_to_caller(mgx_world *w, const float *positions_xyz, float radius, const float *radii, uint32_t n_groups, uint32_t method,
                          int32_t *row_ptr, int32_t *neighbours_out, uint64_t capacity, uint64_t *needed);
int mgx_neighbours(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, int32_t *row_ptr, int32_t *neighbours_out,
                   uint64_t capacity, uint64_t *needed) {
    MGX_ENTER(w);
    if (!w || !positions_xyz || !row_ptr) return fail(MGX_ERR_INVALID, "null argument");
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    return neighbours_to_caller(w, positions_xyz, radius, nullptr, 0, method, row_ptr, neighbours_out, capacity, needed);
}
int mgx_neighbours_groups(mgx_world *w, const float *positions_xyz, const float *radii, uint32_t n_groups, uint32_t method, int32_t *row_ptr,
                          int32_t *neighbours_out, uint64_t capacity, uint64_t *needed) {
    MGX_ENTER(w);
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    const int rc = groups_radii_arguments(w, radii, n_groups);
    if (rc != MGX_OK) return rc;
    if (!positions_xyz || !row_ptr) return fail(MGX_ERR_INVALID, "null argument");
    return neighbours_to_caller(w, positions_xyz, radii[0], radii, n_groups, method, row_ptr, neighbours_out, capacity, needed);
}
static int neighbours_to_caller(mgx_world *w, const float *positions_xyz, float radius, const float *radii, uint32_t n_groups, uint32_t method,
                          int32_t *row_ptr, int32_t *neighbours_out, uint64_t capacity, uint64_t *needed) {
    std::vector<int32_t> ptr, idx;
    int rc = neighbours(w, positions_xyz, radius, method, ptr, idx, radii, n_groups);
    if (rc != MGX_OK) return rc;
    memcpy(row_ptr, ptr.data(), sizeof(int32_t) * ptr.size());
    if (needed) *needed = idx.size();
    if (!neighbours_out) return MGX_OK;  // sizing call
    if (idx.size() > capacity) return fail(MGX_ERR_INVALID, "neighbour list needs %zu entries, capacity %llu", idx.size(), (unsigned long long)capacity);
    if (!idx.empty()) memcpy(neighbours_out, idx.data(), sizeof(int32_t) * idx.size());
    return MGX_OK;
}

int mgx_connections(mgx_world *w, int32_t robot, int32_t *others, uint32_t capacity, uint32_t *n) {
    MGX_ENTER(w);
    if (!w || !n || robot < 0 || (size_t)robot >= w->robots.size()) return fail(MGX_ERR_INVALID, "bad argument");
    const int32_t *c = w->sets.row((size_t)robot);
    const size_t nc = (size_t)w->sets.cnt[(size_t)robot];
    *n = (uint32_t)nc;
    if (!others) return MGX_OK;
    if (nc > capacity) return fail(MGX_ERR_INVALID, "capacity too small");
    for (size_t i = 0; i < nc; i++) others[i] = c[i];
    return MGX_OK;
}

// n_groups: 0 — ONE generator (*robot_number_next), stats {created, deleted}; otherwise one generator per group
// (robot_number_next[n_groups]) and stats [n_groups][stats_stride], {created, deleted, ..} per group (include/mgx.h, ROBOT GROUPS)
static int topology_bookkeeping(mgx_world *w, std::vector<int32_t> &ptr, std::vector<int32_t> &idx, uint64_t *robot_number_next,
                                uint32_t *stats, StageTimer &tm, const uint8_t *chg = nullptr, uint32_t n_groups = 0, uint32_t stats_stride = 2);
// what the per-group calls check before anything happens (no device needed; what the arguments alone say needs no world either)
static int groups_arguments(mgx_world *w, uint32_t n_groups, const uint64_t *number_next) {
    if (!number_next) return fail(MGX_ERR_INVALID, "null argument (number_next)");
    if (n_groups == 0 || n_groups > MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "n_groups %u is not in 1 .. MGX_GROUPS_MAX (%u)", n_groups, MGX_GROUPS_MAX);
    for (uint32_t g = 0; g < n_groups; g++)
        if (number_next[g] == 0) return fail(MGX_ERR_INVALID, "robot_number is NonZeroUsize (group %u)", g);
    if (!w) return fail(MGX_ERR_INVALID, "null argument");
    for (size_t r = 0; r < w->sets.group.size(); r++)
        if (w->sets.group[r] >= n_groups) return fail(MGX_ERR_INVALID, "robot %zu is in group %u: not below n_groups %u", r, w->sets.group[r], n_groups);
    return MGX_OK;
}
// ... and the calls with one radius per group: radii [n_groups] (any value: NaN, zero and negative radii mean what they mean as scalars)
static int groups_radii_arguments(mgx_world *w, const float *radii, uint32_t n_groups) {
    if (!radii) return fail(MGX_ERR_INVALID, "null argument (radii)");
    if (n_groups == 0 || n_groups > MGX_GROUPS_MAX) return fail(MGX_ERR_INVALID, "n_groups %u is not in 1 .. MGX_GROUPS_MAX (%u)", n_groups, MGX_GROUPS_MAX);
    if (!w) return fail(MGX_ERR_INVALID, "null argument");
    for (size_t r = 0; r < w->sets.group.size(); r++)
        if (w->sets.group[r] >= n_groups) return fail(MGX_ERR_INVALID, "robot %zu is in group %u: not below n_groups %u", r, w->sets.group[r], n_groups);
    return MGX_OK;
}
static int update_topology(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, uint64_t *robot_number_next, uint32_t *stats,
                           uint32_t n_groups, const float *radii = nullptr);
int mgx_update_topology(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, uint64_t *robot_number_next,
                        uint32_t *stats) {
    MGX_ENTER(w);
    if (!w || !positions_xyz || !robot_number_next) return fail(MGX_ERR_INVALID, "null argument");
    if (*robot_number_next == 0) return fail(MGX_ERR_INVALID, "robot_number is NonZeroUsize");
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    return update_topology(w, positions_xyz, radius, method, robot_number_next, stats, 0);
}
int mgx_update_topology_groups(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, uint32_t n_groups, uint64_t *number_next,
                               uint32_t *stats) {
    MGX_ENTER(w);
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    const int rc = groups_arguments(w, n_groups, number_next);
    if (rc != MGX_OK) return rc;
    if (!positions_xyz) return fail(MGX_ERR_INVALID, "null argument");
    const std::vector<float> radii((size_t)n_groups, radius);  // (the radii call with all radii equal)
    return update_topology(w, positions_xyz, radius, method, number_next, stats, n_groups, radii.data());
}
int mgx_update_topology_groups_radii(mgx_world *w, const float *positions_xyz, const float *radii, uint32_t method, uint32_t n_groups,
                                     uint64_t *number_next, uint32_t *stats) {
    MGX_ENTER(w);
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    if (!radii) return fail(MGX_ERR_INVALID, "null argument (radii)");
    const int rc = groups_arguments(w, n_groups, number_next);  // (n_groups, the generators, every robot's group)
    if (rc != MGX_OK) return rc;
    if (!positions_xyz) return fail(MGX_ERR_INVALID, "null argument");
    return update_topology(w, positions_xyz, radii[0], method, number_next, stats, n_groups, radii);
}
// radii (may be null): [n_groups], one radius per group (an ungrouped world: radii[0], which `radius` is)
static int update_topology(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, uint64_t *robot_number_next, uint32_t *stats,
                           uint32_t n_groups, const float *radii) {
    std::vector<int32_t> ptr, idx;
    StageTimer tm("update_topology");
    // update_robot_neighbours (robot.rs:1362-1384).  A small world's search runs BESIDE the GBP schedule of the tick before, on a
    // stream of its own — but it must not get onto the device before that schedule's resident launch has all its workgroups
    // there: enqueued a few microseconds behind the launch, its waves took slots the launch's last workgroups needed, the
    // residency census said no and the tick ran launch by launch (seen: three of sixty ticks, 0.8 ms each).  So the search is
    // enqueued only with the launch decided (microseconds after its start); the message counters are brought up to date
    // under it (the pass is about to change who sends to whom).  (Who owns which connection — what the deletions walk —
    // comes from the connection index, kept in step with the list: round 4 listed the connections by owner here, every tick.)
    PendingSearch ps;
    int rc = neighbours_enqueue(w, positions_xyz, radius, method, ps, true, radii, radii ? n_groups : 0);  // (waits for the launch to be decided first if it has to)
    if (rc != MGX_OK) return rc;
    tm.lap("search enqueued");
    flush_counts(w, true);  // (lazy: the robots' counters and cumulative counts; connections are settled when deleted or read)
    tm.lap("message counters (under the search)");
    const uint8_t *chg = nullptr;
    rc = neighbours_collect(w, ps, ptr, idx, &chg);
    if (rc != MGX_OK) return rc;
    tm.lap("neighbour search");
    return topology_bookkeeping(w, ptr, idx, robot_number_next, stats, tm, chg, n_groups);
}
// delete_interrobot_factors + create_interrobot_factors on the search's result (rows per robot id, ascending)
// chg (may be null): per robot, whether its row differs from the one of the pass before — which is its connection set (see
// NeighbourSearch::prev): a robot whose byte is 0 has nothing out of range and nobody new, and its row was not even copied
static int topology_bookkeeping(mgx_world *w, std::vector<int32_t> &ptr, std::vector<int32_t> &idx, uint64_t *robot_number_next,
                                uint32_t *stats, StageTimer &tm, const uint8_t *chg, uint32_t n_groups, uint32_t stats_stride) {
    int rc = MGX_OK;
    w->search.prev_valid = false;  // (until this pass has gone through)
    const int n = (int)w->robots.size();
    w->search.last_changed = -1;
    if (chg) {
        w->search.last_changed = 0;
        for (int r = 0; r < n; r++) w->search.last_changed += chg[r] ? 1 : 0;
    }
    uint32_t created = 0, deleted = 0;
    if (n_groups && stats)
        for (uint32_t g = 0; g < n_groups; g++) stats[(size_t)g * stats_stride] = stats[(size_t)g * stats_stride + 1] = 0;
    // a robot's row of the search and its connection set are both ascending in order key (BTreeSet<Entity>): merges
    ConnSets &cs = w->sets;
    auto key = [&](int x) { return cs.keys[(size_t)x]; };

    // delete_interrobot_factors (robot.rs:1386-1439).  The pairs pass through a
    // HashMap<RobotId, RobotId> filled with `extend` (:1391,1400-1404): one entry per robot, the
    // LAST out-of-range id (largest key) wins; every out-of-range id leaves robots_connected_with
    // (:1406-1408) whether or not its factors get deleted.  The map's iteration order is
    // unspecified in the reference; ascending robot id here.
    // (one merge per robot does both halves of the pass — a robot's row of the search and its connection set are ascending in
    // order key: what is in the set and not in the row is out of range; what is in the row and not in the set is a new
    // neighbour, create_interrobot_factors' snapshot (robot.rs:1449-1461: within range \ connected, taken for every robot
    // before anything is created; the deletions in between leave the sets alone).)
    std::vector<int> &victim = w->scratch_victim;  // (scratch kept with the world: a pass comes through here every tick)
    victim.assign((size_t)n, -1);
    std::vector<std::pair<int, int>> &fresh = w->scratch_fresh;  // (robot, new neighbour), robots ascending, neighbours in row order
    fresh.clear();
    static const bool check_rows = getenv("MGX_CHECK_INDEX") != nullptr;
    bool rows_ok = true;
    auto scan = [&](auto before) {  // before(a, b): robot a's order key is the smaller one
        for (int r = 0; r < n; r++) {
            int32_t *cw = cs.row((size_t)r);
            const int32_t n_cw = cs.cnt[(size_t)r];
            if (chg && !chg[r]) {
                if (check_rows) {  // (diagnostics: an unchanged row IS the set)
                    bool same = ptr[(size_t)r + 1] - ptr[(size_t)r] == n_cw;
                    for (int32_t q = 0; q < n_cw && same; q++) same = cw[q] == idx[(size_t)ptr[(size_t)r] + (size_t)q];
                    if (!same) rows_ok = false;
                }
                continue;
            }
            const bool gone = w->sets.removed[(size_t)r] != 0;  // not in the query any more: its set stays as it is
            int32_t kept = 0, q = 0;
            int32_t j = ptr[(size_t)r];
            const int32_t j1 = ptr[(size_t)r + 1];
            while (q < n_cw || j < j1) {
                if (j >= j1 || (q < n_cw && before(cw[q], idx[(size_t)j]))) {  // connected, not in range
                    if (gone) cw[kept++] = cw[q];
                    else victim[(size_t)r] = cw[q];
                    q++;
                } else if (q >= n_cw || before(idx[(size_t)j], cw[q])) {  // in range, not connected
                    fresh.emplace_back(r, idx[(size_t)j]);
                    j++;
                } else {  // both
                    cw[kept++] = cw[q];
                    q++;
                    j++;
                }
            }
            cs.cnt[(size_t)r] = kept;
        }
    };
    if (cs.monotone()) scan([](int a, int b) { return a < b; });  // (ids ascending == keys ascending: no key is looked up)
    else scan([&](int a, int b) { return key(a) < key(b); });
    if (!rows_ok) return fail(MGX_ERR_STATE, "internal: a row the search calls unchanged is not the robot's connection set (MGX_CHECK_INDEX)");
    tm.lap("range scan");
    {
        std::vector<std::pair<int, int>> pairs;
        for (int r = 0; r < n; r++)
            if (victim[(size_t)r] >= 0) pairs.emplace_back(r, victim[(size_t)r]);
        ir_disconnect_batch(w, pairs);
        deleted = (uint32_t)pairs.size();
        if (n_groups && stats)
            for (const auto &pr : pairs) stats[(size_t)cs.group[(size_t)pr.first] * stats_stride + 1] += 1;
        tm.lap("delete");
    }
    for (const auto &f : fresh) {
        const int r = f.first, o = f.second;
        // (one generator, or the one of the creating robot's group)
        uint64_t *number = n_groups ? robot_number_next + cs.group[(size_t)r] : robot_number_next;
        rc = ir_connect(w, r, o, *number);
        if (rc != MGX_OK) return rc;
        *number += (uint64_t)(w->K - 1);
        cs.insert_sorted((size_t)r, o);  // :1546
        created++;
        if (n_groups && stats) stats[(size_t)cs.group[(size_t)r] * stats_stride] += 1;
    }
    tm.lap("create");
    if (stats && !n_groups) { stats[0] = created; stats[1] = deleted; }
    w->search.prev_valid = chg != nullptr;  // (every robot's set is its row now — and where the search kept the rows, they are on the device)
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
