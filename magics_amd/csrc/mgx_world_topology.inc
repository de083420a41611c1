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
    w->nb_prev_valid = false;  // (the sets change outside a topology pass)
    if (!w->sets.has((size_t)owner, other)) w->sets.insert_sorted((size_t)owner, other);
    return MGX_OK;
}
int mgx_ir_disconnect(mgx_world *w, int32_t a, int32_t b) {
    MGX_ENTER(w);
    int rc = ir_disconnect(w, a, b);
    if (rc != MGX_OK) return rc;
    w->nb_prev_valid = false;
    w->sets.erase((size_t)a, b);
    w->sets.erase((size_t)b, a);
    return MGX_OK;
}

// device neighbour search -> host CSR, rows ascending in order key
// pos == nullptr: the positions come from the device-resident Transforms of the missions (mgx_mission_tick)
// Two halves: everything that is enqueued (positions up, the counting and filling kernels, rows down into pinned memory) and,
// behind a synchronisation of the stream, the host side (a second filling pass if the rows outgrew the guess, ids and order).
// mgx_mission_tick enqueues the search of the NEXT tick in front of this tick's GBP schedule — the Transforms it looks at are
// final once the prior updates have moved them — so its rows are on the host long before that tick's one synchronisation.
// track: the search of a topology pass over the caller's positions — the kernel compares every robot's row with the one it got in
// the pass before (mgx_world::nb_prev) and says which ones changed
static int neighbours_enqueue(mgx_world *w, const float *pos, float radius, uint32_t method, mgx_world::PendingSearch &ps, bool track = false) {
    if (!device_ok()) return fail(MGX_ERR_NO_DEVICE, "no HIP device");
    w->mission_search.valid = false;  // the buffers below are shared: whatever was waiting in them is gone
    ps.valid = false;
    const int n_all = (int)w->robots.size();
    const bool from_missions = pos == nullptr;
    std::vector<int> &alive = ps.alive;  // removed robots are in no query: search the others, map back
    alive.clear();
    std::vector<float> packed;
    for (int r = 0; r < n_all; r++) {
        // ghosts take part: a sharded world that follows a changing topology holds EVERY robot of the
        // scenario (its own ones and ghost copies of all others) and is handed all positions, so that
        // the connection bookkeeping below runs identically on every rank
        if (!w->sets.removed[(size_t)r]) alive.push_back(r);
    }
    const bool compact = (int)alive.size() != n_all;
    if (compact && !from_missions) {
        packed.resize(3 * alive.size());
        for (size_t a = 0; a < alive.size(); a++) memcpy(&packed[3 * a], pos + 3 * (size_t)alive[a], 3 * sizeof(float));
        pos = packed.data();
    }
    const int n = (int)alive.size();
    w->last_search_launches = 0;
    w->last_search_changed = -1;  // (until flags reach a pass: topology_bookkeeping)
    const bool usable_radius = std::isfinite(radius) && radius > 0.f;
    bool grid = method == MGX_NEIGHBOURS_GRID || (method == MGX_NEIGHBOURS_AUTO && n >= 512);
    if (!usable_radius) grid = false;  // radius <= 0 / NaN / inf: every pair has to see the predicate
    uint32_t M = 64;
    while (M < 2u * (uint32_t)std::max(n, 1)) M <<= 1;
    // A search over positions the CALLER hands in reads nothing of the world's device state: it runs on a stream of its own,
    // next to whatever the world's stream is still busy with (the previous tick's GBP schedule), instead of behind it.
    // (The missions' search reads the device's Transforms, which the tick's kernels move: that one stays in stream order.)
    hipStream_t s = w->stream;
    if (!from_missions) {
        // Never beside a resident launch that is still getting onto the device: the search's workgroups would take slots the
        // launch's last workgroups need — the census says no and a handful of ticks run launch by launch (a thousand robots
        // leave two or three free slots per XCD; enqueued at once "when both fit" the search still cost every third launch its
        // residency: tools/dynamic_tick_bench.py, 27 of 90 launches declined, 4.2 k ticks/s against 5.9 k behind the decision).
        // Behind a DECIDED launch the search finds the holes that launch leaves (mgx_topology.hip) and runs beside it.
        if (w->pending.active) { const int rcc = confirm_resident(w); if (rcc != MGX_OK) return rcc; }
        if (!w->search_stream) HIP_TRY(hipStreamCreateWithFlags(&w->search_stream, hipStreamNonBlocking));
        s = w->search_stream;
    }
    if (w->nb_last_stream_set && w->nb_last_stream != s) HIP_TRY(hipStreamSynchronize(w->nb_last_stream));  // the scratch buffers are shared
    w->nb_last_stream = s;
    w->nb_last_stream_set = true;
    ps.stream = s;
    HIP_TRY(w->nb_pos.reserve((size_t)3 * std::max(n, 1)));
    HIP_TRY(w->nb_cnt.reserve((size_t)std::max(n, 1)));
    HIP_TRY(w->nb_ptr.reserve((size_t)n + 1));
    HIP_TRY(w->nb_members.reserve((size_t)std::max(n, 1)));
    HIP_TRY(w->nb_special.reserve((size_t)std::max(n, 1)));
    HIP_TRY(w->nb_nspecial.reserve(1));
    HIP_TRY(w->nb_bucket_cnt.reserve(M));
    HIP_TRY(w->nb_bucket_ptr.reserve((size_t)M + 1));
    HIP_TRY(w->nb_cursor.reserve(M));
    if (from_missions) {
        mgx_world::Mission &ms = w->mission;
        if (ms.alive_dirty || ms.alive_host.size() != alive.size()) {
            ms.alive_host.assign(alive.begin(), alive.end());
            if (ms.alive_host.empty()) ms.alive_host.push_back(0);
            HIP_TRY(ms.alive_d.upload(ms.alive_host, s));
            HIP_TRY(hipStreamSynchronize(s));
            ms.alive_host.resize(alive.size());
            ms.alive_dirty = false;
        }
        HIP_TRY(launch_mission_positions(ms.d, n, ms.alive_d.p, w->nb_pos.p, s));
    }
    // small worlds (AUTO): ONE small kernel, rows of a fixed capacity written in place, no scans (mgx_topology.hip)
    const bool rows_mode = method == MGX_NEIGHBOURS_AUTO && n > 0 && n <= 4096;
    if (rows_mode) {
        const int cap = w->nb_row_cap;
        const size_t off_cnt = sizeof(float) * 3 * (size_t)n, off_rows = off_cnt + sizeof(int32_t) * (size_t)n;
        HIP_TRY(w->nb_pin.reserve(off_rows + sizeof(int32_t) * (size_t)n * (size_t)cap));
        // (the kept rows: where robots left the query, or the world's robots are not the ones of the last pass, nothing is kept)
        const bool keep_rows = track && !compact && !from_missions && cap <= 32;
        int prev_valid = 0;
        if (keep_rows) {
            const size_t words = (size_t)n * (size_t)neighbours_prev_stride();
            if (w->nb_prev.cap < words || w->nb_prev_n != (size_t)n) {
                HIP_TRY(w->nb_prev.reserve(words));
                w->nb_prev_n = (size_t)n;
                w->nb_prev_valid = false;
            }
            prev_valid = w->nb_prev_valid ? 1 : 0;
            w->nb_prev_valid = false;  // (the kernel overwrites the kept rows: they are the sets again when the pass has gone through)
        }
        HIP_TRY(w->nb_idx.reserve((size_t)n * (size_t)cap));
        char *pin = static_cast<char *>(w->nb_pin.p);
        // no copies at all: the kernel reads the callers' positions from the pinned block and writes counts and rows into it
        // (a copy is a launch of its own — a blit kernel too big to find room beside a resident schedule launch)
        void *dpin = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dpin, pin, 0));
        char *dp = static_cast<char *>(dpin);
        if (!from_missions) memcpy(pin, pos, sizeof(float) * 3 * (size_t)n);
        bool chg_written = false;
        HIP_TRY(neighbours_rows(from_missions ? w->nb_pos.p : reinterpret_cast<const float *>(dp), n, radius, cap,
                                reinterpret_cast<int32_t *>(dp + off_cnt), reinterpret_cast<int32_t *>(dp + off_rows), s, nullptr,
                                keep_rows ? w->nb_prev.p : nullptr, prev_valid, &chg_written, &w->last_search_kernel));
        w->last_search_cap = cap;
        w->last_search_launches++;
        ps.has_chg = chg_written;
        ps.n = n; ps.n_all = n_all; ps.compact = compact; ps.guess = 0; ps.off_ptr = off_cnt; ps.off_idx = off_rows;
        ps.radius = radius; ps.method = method; ps.grid = false; ps.M = M; ps.rows = true; ps.row_cap = cap; ps.from_missions = from_missions;
        ps.valid = true;
        return MGX_OK;
    }
    ps.rows = false;
    const size_t guess = std::min(w->nb_idx.cap, w->nb_last_total + w->nb_last_total / 4 + 64);
    // pinned layout: [3 n floats: positions up] [n + 1 ints: row pointers down] [guess ints: rows down]
    const size_t off_ptr = sizeof(float) * 3 * (size_t)std::max(n, 1), off_idx = off_ptr + sizeof(int32_t) * ((size_t)n + 1);
    HIP_TRY(w->nb_pin.reserve(off_idx + sizeof(int32_t) * guess));
    char *pin = static_cast<char *>(w->nb_pin.p);
    if (!from_missions && n) {
        memcpy(pin, pos, sizeof(float) * 3 * (size_t)n);
        HIP_TRY(hipMemcpyAsync(w->nb_pos.p, pin, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(neighbours_count(w->nb_pos.p, n, radius, grid, M, w->nb_cnt.p, w->nb_bucket_cnt.p, w->nb_bucket_ptr.p, w->nb_cursor.p,
                             w->nb_members.p, w->nb_special.p, w->nb_nspecial.p, w->nb_ptr.p, s));
    if (n > 0) {  // (an empty query launches nothing)
        w->last_search_kernel = grid ? MGX_SEARCH_TWO_PASS_GRID : MGX_SEARCH_TWO_PASS_PAIRS;
        w->last_search_cap = 0;
        w->last_search_launches++;
    }
    // The second pass needs the total to size its output — one more host round trip.  Instead it runs right
    // away into the buffer left from the last search (the kernels leave it alone if the rows do not fit), and
    // rows and counts come back together; only a total beyond the guess costs the second trip.
    if (guess > 0 && w->nb_idx.p)
        HIP_TRY(neighbours_fill(w->nb_pos.p, n, radius, grid, M, w->nb_bucket_ptr.p, w->nb_members.p, w->nb_special.p,
                                w->nb_nspecial.p, w->nb_ptr.p, w->nb_idx.p, (int32_t)guess, s));
    HIP_TRY(hipMemcpyAsync(pin + off_ptr, w->nb_ptr.p, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
    if (guess > 0 && w->nb_idx.p) HIP_TRY(hipMemcpyAsync(pin + off_idx, w->nb_idx.p, sizeof(int32_t) * guess, hipMemcpyDeviceToHost, s));
    ps.n = n; ps.n_all = n_all; ps.compact = compact; ps.guess = guess; ps.off_ptr = off_ptr; ps.off_idx = off_idx;
    ps.radius = radius; ps.method = method; ps.grid = grid; ps.M = M;
    ps.valid = true;
    return MGX_OK;
}
// chg (may be null): where to put the pointer to the rows-changed bytes of the search, or null if it has none — then only the rows
// of robots whose byte is set are copied into idx (the others' entries are not to be read)
static int neighbours_collect(mgx_world *w, mgx_world::PendingSearch &ps, std::vector<int32_t> &ptr, std::vector<int32_t> &idx,
                              const uint8_t **chg = nullptr) {
    if (chg) *chg = nullptr;
    hipStream_t s = ps.stream;
    const int n = ps.n, n_all = ps.n_all;
    const std::vector<int> &alive = ps.alive;
    const size_t guess = ps.guess;
    char *pin = static_cast<char *>(w->nb_pin.p);
    ps.valid = false;
    HIP_TRY(hipStreamSynchronize(s));
    if (ps.rows) {
        int cap = ps.row_cap;
        const int32_t *cnt = reinterpret_cast<const int32_t *>(pin + ps.off_ptr);
        if (ps.has_chg) {  // the flags out of the counts (the pinned block is the host's to write)
            int32_t *c = reinterpret_cast<int32_t *>(pin + ps.off_ptr);
            const int32_t bit = neighbours_changed_bit();
            w->scratch_chg.resize((size_t)n);
            for (int i = 0; i < n; i++) { w->scratch_chg[(size_t)i] = (c[i] & bit) ? 1 : 0; c[i] &= ~bit; }
        }
        int32_t longest = 0;
        for (int i = 0; i < n; i++) longest = std::max(longest, cnt[i]);
        if (longest > cap) {  // a row outgrew its capacity: once more with room (the world remembers)
            while (cap < longest) cap *= 2;
            w->nb_row_cap = cap;
            const size_t off_rows = ps.off_ptr + sizeof(int32_t) * (size_t)n;
            ps.has_chg = false;  // (the kept rows were half written by the search that did not fit: everybody counts as changed)
            // the pinned block grows: the callers' positions it holds move along (a mission's are on the device)
            std::vector<float> keep;
            if (!ps.from_missions) keep.assign(reinterpret_cast<const float *>(pin), reinterpret_cast<const float *>(pin) + 3 * (size_t)n);
            HIP_TRY(w->nb_pin.reserve(off_rows + sizeof(int32_t) * (size_t)n * (size_t)cap));
            pin = static_cast<char *>(w->nb_pin.p);
            if (!ps.from_missions) memcpy(pin, keep.data(), sizeof(float) * keep.size());
            void *dpin = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&dpin, pin, 0));
            char *dp = static_cast<char *>(dpin);
            HIP_TRY(neighbours_rows(ps.from_missions ? w->nb_pos.p : reinterpret_cast<const float *>(dp), n, ps.radius, cap,
                                    reinterpret_cast<int32_t *>(dp + ps.off_ptr), reinterpret_cast<int32_t *>(dp + off_rows), s, nullptr,
                                    nullptr, 0, nullptr, &w->last_search_kernel));
            w->last_search_cap = cap;
            w->last_search_launches++;
            HIP_TRY(hipStreamSynchronize(s));
            cnt = reinterpret_cast<const int32_t *>(pin + ps.off_ptr);
        }
        const int32_t *rows = reinterpret_cast<const int32_t *>(pin + ps.off_ptr + sizeof(int32_t) * (size_t)n);
        ptr.assign((size_t)n + 1, 0);
        for (int i = 0; i < n; i++) ptr[(size_t)i + 1] = ptr[(size_t)i] + cnt[i];
        idx.resize((size_t)ptr[(size_t)n]);
        static const bool check_index = getenv("MGX_CHECK_INDEX") != nullptr;  // (diagnostics: every row is there for the pass to verify)
        const uint8_t *changed = (chg && ps.has_chg && !ps.compact) ? w->scratch_chg.data() : nullptr;
        for (int i = 0; i < n; i++)
            if (cnt[i] && (!changed || changed[i] || check_index)) memcpy(idx.data() + ptr[(size_t)i], rows + (size_t)i * (size_t)cap, sizeof(int32_t) * (size_t)cnt[i]);
        if (chg) *chg = changed;
        w->nb_last_total = idx.size();
    } else {
    ptr.assign((size_t)n + 1, 0);
    memcpy(ptr.data(), pin + ps.off_ptr, sizeof(int32_t) * ((size_t)n + 1));
    const size_t total = (size_t)ptr[(size_t)n];
    w->nb_last_total = total;
    if (total <= guess && (w->nb_idx.p || total == 0)) {
        idx.resize(total);
        if (total) memcpy(idx.data(), pin + ps.off_idx, sizeof(int32_t) * total);
    } else {
        idx.assign(total, 0);
        if (n > 0 && guess > 0 && w->nb_idx.p) w->last_search_launches++;  // (the filling pass ran into the guessed buffer: once more)
        HIP_TRY(w->nb_idx.reserve(total));
        HIP_TRY(neighbours_fill(w->nb_pos.p, n, ps.radius, ps.grid, ps.M, w->nb_bucket_ptr.p, w->nb_members.p, w->nb_special.p,
                                w->nb_nspecial.p, w->nb_ptr.p, w->nb_idx.p, (int32_t)total, s));
        HIP_TRY(hipMemcpyAsync(idx.data(), w->nb_idx.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    }
    if (ps.compact) {  // back to world robot ids, empty rows for the removed ones
        for (int32_t &j : idx) j = alive[(size_t)j];
        std::vector<int32_t> full((size_t)n_all + 1, 0);
        for (int a = 0; a < n; a++) full[(size_t)alive[(size_t)a] + 1] = ptr[(size_t)a + 1] - ptr[(size_t)a];
        for (int r = 0; r < n_all; r++) full[(size_t)r + 1] += full[(size_t)r];
        ptr.swap(full);
    }
    if (chg && *chg && !w->sets.monotone()) {  // (rows are re-sorted by key below: every row is needed)
        const int32_t *cnt = reinterpret_cast<const int32_t *>(pin + ps.off_ptr);
        const int32_t *rows = reinterpret_cast<const int32_t *>(pin + ps.off_ptr + sizeof(int32_t) * (size_t)n);
        for (int i = 0; i < n; i++)
            if (cnt[i]) memcpy(idx.data() + ptr[(size_t)i], rows + (size_t)i * (size_t)ps.row_cap, sizeof(int32_t) * (size_t)cnt[i]);
        *chg = nullptr;
    }
    if (!w->sets.monotone())  // ids ascending == keys ascending: nothing to do (the keys' compact copies: fixed when a robot is added)
        for (int r = 0; r < n_all; r++)
            std::sort(idx.begin() + ptr[(size_t)r], idx.begin() + ptr[(size_t)r + 1],
                      [&](int a, int b) { return w->robots[(size_t)a].order_key < w->robots[(size_t)b].order_key; });
    return MGX_OK;
}
static int neighbours(mgx_world *w, const float *pos, float radius, uint32_t method, std::vector<int32_t> &ptr,
                      std::vector<int32_t> &idx) {
    mgx_world::PendingSearch ps;
    const int rc = neighbours_enqueue(w, pos, radius, method, ps);
    return rc != MGX_OK ? rc : neighbours_collect(w, ps, ptr, idx);
}

int mgx_neighbours(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, int32_t *row_ptr, int32_t *neighbours_out,
                   uint64_t capacity, uint64_t *needed) {
    MGX_ENTER(w);
    if (!w || !positions_xyz || !row_ptr) return fail(MGX_ERR_INVALID, "null argument");
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    std::vector<int32_t> ptr, idx;
    int rc = neighbours(w, positions_xyz, radius, method, ptr, idx);
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

static int topology_bookkeeping(mgx_world *w, std::vector<int32_t> &ptr, std::vector<int32_t> &idx, uint64_t *robot_number_next,
                                uint32_t *stats, StageTimer &tm, const uint8_t *chg = nullptr);
int mgx_update_topology(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, uint64_t *robot_number_next,
                        uint32_t *stats) {
    MGX_ENTER(w);
    if (!w || !positions_xyz || !robot_number_next) return fail(MGX_ERR_INVALID, "null argument");
    if (*robot_number_next == 0) return fail(MGX_ERR_INVALID, "robot_number is NonZeroUsize");
    if (method > MGX_NEIGHBOURS_GRID) return fail(MGX_ERR_INVALID, "bad method");
    std::vector<int32_t> ptr, idx;
    StageTimer tm("update_topology");
    // update_robot_neighbours (robot.rs:1362-1384).  A small world's search runs BESIDE the GBP schedule of the tick before, on a
    // stream of its own — but it must not get onto the device before that schedule's resident launch has all its workgroups
    // there: enqueued a few microseconds behind the launch, its waves took slots the launch's last workgroups needed, the
    // residency census said no and the tick ran launch by launch (seen: three of sixty ticks, 0.8 ms each).  So the search is
    // enqueued only with the launch decided (microseconds after its start); the message counters are brought up to date
    // under it (the pass is about to change who sends to whom).  (Who owns which connection — what the deletions walk —
    // comes from the connection index, kept in step with the list: round 4 listed the connections by owner here, every tick.)
    mgx_world::PendingSearch ps;
    int rc = neighbours_enqueue(w, positions_xyz, radius, method, ps, true);  // (waits for the launch to be decided first if it has to)
    if (rc != MGX_OK) return rc;
    tm.lap("search enqueued");
    flush_counts(w, true);  // (lazy: the robots' counters and cumulative counts; connections are settled when deleted or read)
    tm.lap("message counters (under the search)");
    const uint8_t *chg = nullptr;
    rc = neighbours_collect(w, ps, ptr, idx, &chg);
    if (rc != MGX_OK) return rc;
    tm.lap("neighbour search");
    return topology_bookkeeping(w, ptr, idx, robot_number_next, stats, tm, chg);
}
// delete_interrobot_factors + create_interrobot_factors on the search's result (rows per robot id, ascending)
// chg (may be null): per robot, whether its row differs from the one of the pass before — which is its connection set (see
// mgx_world::nb_prev): a robot whose byte is 0 has nothing out of range and nobody new, and its row was not even copied
static int topology_bookkeeping(mgx_world *w, std::vector<int32_t> &ptr, std::vector<int32_t> &idx, uint64_t *robot_number_next,
                                uint32_t *stats, StageTimer &tm, const uint8_t *chg) {
    int rc = MGX_OK;
    w->nb_prev_valid = false;  // (until this pass has gone through)
    const int n = (int)w->robots.size();
    w->last_search_changed = -1;
    if (chg) {
        w->last_search_changed = 0;
        for (int r = 0; r < n; r++) w->last_search_changed += chg[r] ? 1 : 0;
    }
    uint32_t created = 0, deleted = 0;
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
        tm.lap("delete");
    }
    for (const auto &f : fresh) {
        const int r = f.first, o = f.second;
        rc = ir_connect(w, r, o, *robot_number_next);
        if (rc != MGX_OK) return rc;
        *robot_number_next += (uint64_t)(w->K - 1);
        cs.insert_sorted((size_t)r, o);  // :1546
        created++;
    }
    tm.lap("create");
    if (stats) { stats[0] = created; stats[1] = deleted; }
    w->nb_prev_valid = chg != nullptr;  // (every robot's set is its row now — and where the search kept the rows, they are on the device)
    return MGX_OK;
}

}  // extern "C" (continued in the next part)
