// mgx_world_counters.inc — message counters (MessageCount): the launch log, lazy settling of the connections, flush_counts.
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// ---- message counters (factorgraph/mod.rs:29-137, factorgraph.rs:876-890) ----------------------------
// Every count is structural: who sends to whom is fixed by the topology, the enabled kinds, the
// antenna / idle flags and (for tracking factors) iteration_count.factor — never by message
// contents (a skipped factor still "sends" its empty messages, factor/mod.rs:353-367).  So the
// launches are only logged, and the counters are brought up to date whenever one of those inputs
// is about to change or a count is asked for.

// A connection's counters brought up to date against its robots' cumulative counts (IrConn::base; the flags and the enabled kinds
// have not changed since it was settled last: whoever changes them settles everything first — flush_counts in full).
static void settle_conn(mgx_world *w, IrConn &c) {
    const size_t o = (size_t)c.owner, t = (size_t)c.other;
    const mgx_world::Cum &cu = w->cum;
    const uint64_t now[5] = {cu.nIv[o], cu.nEv[t], cu.nEf[o], cu.on_ir[o], cu.on_ir[t]};
    uint64_t d[5];
    for (int q = 0; q < 5; q++) { d[q] = now[q] - c.base[q]; c.base[q] = now[q]; }
    if (!(w->p.enable_mask & 2u)) return;
    const uint64_t K1 = (uint64_t)(w->K - 1);
    const Robot &ra = w->robots[o], &rb = w->robots[t];
    const bool radio_a = ra.antenna && !ra.idle, radio_b = rb.antenna && !rb.idle;
    c.cnt[2] += d[3];                          // the owner's own variable delivers to its factor (change_prior)
    c.cnt[3] += d[4];                          // the foreign variable delivers to it
    c.cnt[2] += d[0] * K1;                     // own variables' responses (internal sweeps)
    if (radio_a) c.cnt[3] += d[1] * K1;        // the foreign variables' responses (robot.rs:1842-1858)
    const uint64_t sent = d[2] * c.updates_per_sweep;  // external factor sweeps: one message per key
    c.cnt[0] += sent;
    c.cnt[1] += sent;
    if (radio_b) w->robots[t].cnt[3] += sent;  // delivered (robot.rs:1813-1831)
}

// lazy: the robots' own counters and cumulative counts only — the connections stay as they are until somebody needs them settled
// (the per-tick topology pass: what it deletes it settles itself).  Not while factors still lack inbox keys (their counting
// replays the log per connection).
static void flush_counts(mgx_world *w, bool lazy) {
    const int rcc = confirm_resident(w);  // the pending launch's entries join the log once it is known to have run
    if (rcc != MGX_OK && w->sticky_rc == MGX_OK) w->sticky_rc = rcc;  // (a re-run that failed: reported by whatever runs or reads next)
    const size_t n = w->robots.size();
    mgx_world::Cum &cu = w->cum;
    if (cu.nIv.size() < n) { cu.nIv.resize(n, 0); cu.nEv.resize(n, 0); cu.nEf.resize(n, 0); cu.on_ir.resize(n, 0); }
    const bool keyless = w->n_keyless > 0;
    if (keyless) lazy = false;
    if (w->clog.empty() && w->cp_dirty.empty()) {
        if (!lazy && w->conns_unsettled) {
            for (IrConn &c : w->conns) settle_conn(w, c);
            w->conns_unsettled = false;
        }
        return;
    }
    const int K = w->K;
    // (the enabled kinds are the robot's GROUP's where the world is masked — mgx_set_group_enabled; the inter-robot bit is the world's)
    const uint32_t en_ir = w->p.enable_mask & 2u;
    // The robots (what each one's sweeps were, from the log: their own counters, and the cumulative counts the connections are
    // settled against), then — in full — the connections.  What the passes need of a robot sits in compact arrays: a Robot is a
    // dozen vectors wide.
    std::vector<uint64_t> nIv(n, 0), nEf(n, 0), nEv(n, 0), nIfv(n, 0), trkv(n, 0);
    std::vector<uint8_t> flags(n, 0);  // bit 0: on air (antenna and not idle), bit 1: idle
    std::vector<int64_t> itf0(n, 0);   // the robots' factor iteration counts in front of this log
    // Past a robot's tracking gate (ten factor sweeps) every entry of the log only ADDS, and a world-wide entry adds the same to
    // every robot with the same flags: the log is summed once per class of robots — on air / silent / idle — as suffix sums, and
    // a robot walks the log itself only as far as its gate is still closed.  (A driver that iterates without reading fills the log
    // at three entries per schedule; walked per robot, four thousand entries times a thousand robots were a 6.8 ms stall of the
    // host every 1365 schedules — 6 % of a sustained run, and the lingering launch it starved ended each time:
    // tools/iterate_stalls.py.)
    struct Sum { uint64_t nEf = 0, nEv = 0, nIv = 0, nIf = 0, trk = 0; int64_t itf = 0; };
    // one entry applied to a robot's running sums (one repetition = [external factor][external variable] n_int x ([internal
    // factor][internal variable]))
    auto apply = [](const mgx_world::CountEntry &e, bool radio, bool idle, Sum &a) {
        const uint64_t fac_per_rep = ((e.ext & 1u) && radio ? 1u : 0u) + ((e.in & 1u) && !idle ? (uint64_t)e.n_int : 0u);
        uint64_t rep = 0;
        for (; rep < e.times && a.itf < 10 && fac_per_rep; rep++) {  // tracking gate still closed: step by step
            if ((e.ext & 1u) && radio) { a.nEf++; a.itf++; }
            if ((e.ext & 2u) && radio) a.nEv++;
            if (!idle)
                for (int q = 0; q < e.n_int; q++) {
                    if (e.in & 1u) { a.nIf++; if (a.itf >= 10) a.trk++; a.itf++; }
                    if (e.in & 2u) a.nIv++;
                }
        }
        const uint64_t left = e.times - rep;
        if ((e.ext & 1u) && radio) { a.nEf += left; a.itf += (int64_t)left; }
        if ((e.ext & 2u) && radio) a.nEv += left;
        if (!idle) {
            if (e.in & 1u) { const uint64_t k = left * (uint64_t)e.n_int; a.nIf += k; if (fac_per_rep) a.trk += k; a.itf += (int64_t)k; }
            if (e.in & 2u) a.nIv += left * (uint64_t)e.n_int;
        }
    };
    const size_t n_log = w->clog.size();
    // an entry's scope (CountEntry::robot): a robot's id; -1: every robot; -2 - g: the robots of group g (a launch of a mixed
    // mgx_iterate_groups call, whose phases are per group)
    auto out_of_scope = [w](const mgx_world::CountEntry &e, size_t r) {
        return e.robot >= 0 ? (size_t)e.robot != r : (e.robot <= -2 && w->sets.group[r] != (uint32_t)(-2 - e.robot));
    };
    bool world_wide_only = true;
    for (const mgx_world::CountEntry &e : w->clog) world_wide_only = world_wide_only && e.robot == -1;
    std::vector<Sum> suffix[3];  // [class: 0 on air, 1 silent, 2 idle][j]: entries j .. end applied with the gate open
    if (world_wide_only)
        for (int c = 0; c < 3; c++) {
            const bool radio = c == 0, idle = c == 2;
            suffix[c].assign(n_log + 1, Sum{});
            for (size_t j = n_log; j-- > 0;) {
                Sum one;
                one.itf = 10;  // (gate open)
                apply(w->clog[j], radio, idle, one);
                Sum &d = suffix[c][j];
                const Sum &nx = suffix[c][j + 1];
                d.nEf = nx.nEf + one.nEf; d.nEv = nx.nEv + one.nEv; d.nIv = nx.nIv + one.nIv; d.nIf = nx.nIf + one.nIf; d.trk = nx.trk + one.trk;
                d.itf = nx.itf + (one.itf - 10);
            }
        }
    for (size_t r = 0; r < n; r++) {
        Robot &rb = w->robots[r];
        // ghosts too: on a sharded world every rank sees the same launches and holds every robot's flags, so the sweeps a
        // ghost has run (what its variables answered to the factors local robots own) are known here; only the totals of
        // the ghost's own graph are its owner's business
        const bool idle = rb.idle != 0, radio = rb.antenna && !idle;
        flags[r] = (uint8_t)((radio ? 1 : 0) | (idle ? 2 : 0));
        Sum a;
        a.itf = rb.cnt_itf;
        itf0[r] = rb.cnt_itf;
        if (world_wide_only) {
            size_t j = 0;
            while (j < n_log && a.itf < 10 && !idle) apply(w->clog[j++], radio, idle, a);  // (its gate: entry by entry; an idle robot's never moves)
            const Sum &t = suffix[radio ? 0 : (idle ? 2 : 1)][j];
            a.nEf += t.nEf; a.nEv += t.nEv; a.nIv += t.nIv; a.nIf += t.nIf; a.trk += t.trk; a.itf += t.itf;
        } else {
            for (const mgx_world::CountEntry &e : w->clog) {
                if (out_of_scope(e, r)) continue;
                apply(e, radio, idle, a);
            }
        }
        nEf[r] = a.nEf; nEv[r] = a.nEv; nIv[r] = a.nIv;
        const uint64_t nIf = a.nIf, trk = a.trk;
        const int64_t itf = a.itf;
        rb.cnt_itf = itf;
        nIfv[r] = nIf;
        trkv[r] = trk;
    }
    // change_prior (variable.rs:203-230): its sends stay in a local counter; the connected factors receive
    if (!w->cp_dirty.empty()) {
        for (uint32_t key : w->cp_dirty) {
            const size_t r = key / (uint32_t)K;
            const int i = (int)(key % (uint32_t)K);
            const uint64_t c = w->cp_pending[key];
            w->cp_pending[key] = 0;
            Robot &rb = w->robots[r];
            const uint32_t en = w->kinds_of_robot(r);
            const uint64_t dyn_here = (uint64_t)((i >= 1) + (i <= K - 2));
            rb.cnt[2] += c * (((en & 1u) ? dyn_here : 0) + ((i >= 1 && i <= K - 2) ? (uint64_t)(((en & 4u) != 0) + ((en & 8u) != 0)) : 0));
            if (i >= 1) cu.on_ir[r] += c;  // one inter-robot factor per connection hangs on this variable
        }
        w->cp_dirty.clear();
    }
    const bool log_any = !w->clog.empty();
    if (keyless) {
        // Some factors still lack inbox keys: what they send follows the log in order, per connection (the connections WITH all
        // their keys are settled as ever, against the cumulative counts BEFORE this log joins them — their share of it is added here).
        for (IrConn &c : w->conns) {
            settle_conn(w, c);  // (prior changes up to now; sweeps up to the last flush)
            if (!en_ir || !log_any) continue;
            const size_t o = (size_t)c.owner, t = (size_t)c.other;
            const bool radio_a = (flags[o] & 1u) != 0, radio_b = (flags[t] & 1u) != 0;
            c.cnt[2] += nIv[o] * (uint64_t)(K - 1);
            if (radio_a) c.cnt[3] += nEv[t] * (uint64_t)(K - 1);
            uint64_t to_own = nEf[o] * c.updates_per_sweep, to_foreign = to_own;
            if (!c.keys.empty()) {  // some keys are still missing: replay the log in order until they are all there
                const bool a_idle = (flags[o] & 2u) != 0;
                to_own = to_foreign = 0;
                for (const mgx_world::CountEntry &e : w->clog) {
                    if (out_of_scope(e, (size_t)c.owner)) continue;  // per-robot launches run internal sweeps only
                    for (uint64_t rep = 0; rep < e.times; rep++) {
                        if (e.robot < 0 && (e.ext & 1u) && radio_a)
                            for (size_t f = 0; f < c.keys.size(); f++) { to_own += c.uses[f] * (c.keys[f] & 1u); to_foreign += c.uses[f] * ((c.keys[f] >> 1) & 1u); }
                        if (e.robot < 0 && (e.ext & 2u) && radio_a && radio_b)
                            for (uint8_t &k : c.keys) k |= 2u;
                        if ((e.in & 2u) && e.n_int > 0 && !a_idle)
                            for (uint8_t &k : c.keys) k |= 1u;
                    }
                }
                bool all = true;
                for (uint8_t k : c.keys) all = all && k == 3u;
                if (all) { c.keys.clear(); c.uses.clear(); w->n_keyless--; }
            }
            c.cnt[0] += to_own;
            c.cnt[1] += to_foreign;
            if (radio_b) w->robots[t].cnt[3] += to_foreign;  // delivered (robot.rs:1813-1831)
        }
    }
    if (log_any) {
        conn_index_ensure(w);  // (how many connections a robot owns / is the target of: the index' lists)
        for (size_t r = 0; r < n; r++) {
            cu.nIv[r] += nIv[r]; cu.nEv[r] += nEv[r]; cu.nEf[r] += nEf[r];
            Robot &rb = w->robots[r];
            if (rb.ghost) continue;
            const uint64_t own = w->cidx.out[r].size(), foreign = w->cidx.in[r].size();
            const uint32_t en = w->kinds_of_robot(r);
            const uint64_t dynf = (en & 1u) ? 2ull * (K - 1) : 0, obsf = (en & 4u) ? (uint64_t)(K - 2) : 0, trkf = (en & 8u) ? (uint64_t)(K - 2) : 0;
            const uint64_t s_int = 2ull * (K - 1) + 2ull * (K - 2) + (uint64_t)(K - 1) * own, s_ext = (uint64_t)(K - 1) * foreign;
            // internal factor sweeps: one message per inbox key of every updated factor, received by the variables
            rb.cnt[0] += nIfv[r] * (dynf + obsf) + trkv[r] * trkf;
            rb.cnt[2] += nIfv[r] * (dynf + obsf) + trkv[r] * trkf;
            // variable sweeps answer every inbox key; only own-graph, enabled factors receive (internal sweeps)
            rb.cnt[0] += (nIv[r] + nEv[r]) * s_int;
            rb.cnt[1] += (nIv[r] + nEv[r]) * s_ext;
            rb.cnt[2] += nIv[r] * (dynf + obsf + trkf);
            // factors without inbox keys (created switched off, Robot::nokey) send nothing: the internal factor sweeps in front
            // of the robot's first internal variable sweep under the kind — the log in order — were counted above and are taken back
            const uint32_t nk = (uint32_t)rb.nokey & en & 13u;
            if (nk && !(flags[r] & 2u)) {
                const bool radio = (flags[r] & 1u) != 0;
                int64_t itf = itf0[r];
                uint64_t missed = 0, missed_open = 0;  // sweeps without keys; those of them behind the tracking gate
                bool filled = false;
                for (const mgx_world::CountEntry &e : w->clog) {
                    if (filled) break;
                    if (out_of_scope(e, r)) continue;
                    for (uint64_t rep = 0; rep < e.times && !filled; rep++) {
                        if ((e.ext & 1u) && radio) itf++;
                        for (int q = 0; q < e.n_int && !filled; q++) {
                            if (e.in & 1u) { missed++; if (itf >= 10) missed_open++; itf++; }
                            if (e.in & 2u) filled = true;
                        }
                    }
                }
                const uint64_t back = missed * (((nk & 1u) ? 2ull * (K - 1) : 0) + ((nk & 4u) ? (uint64_t)(K - 2) : 0)) + missed_open * ((nk & 8u) ? (uint64_t)(K - 2) : 0);
                rb.cnt[0] -= back;
                rb.cnt[2] -= back;
                if (filled) rb.nokey &= (uint8_t)~en;
            }
        }
    }
    if (keyless) {  // (their share of this log was added by hand above: the bases move with the cumulative counts)
        for (IrConn &c : w->conns) {
            const size_t o = (size_t)c.owner, t = (size_t)c.other;
            c.base[0] = cu.nIv[o]; c.base[1] = cu.nEv[t]; c.base[2] = cu.nEf[o];
        }
        w->conns_unsettled = false;
    } else if (!lazy) {
        for (IrConn &c : w->conns) settle_conn(w, c);
        w->conns_unsettled = false;
    } else {
        w->conns_unsettled = true;
    }
    w->clog.clear();
}
static void log_launch(mgx_world *w, int robot, uint32_t ext_mask, uint32_t int_mask, int n_int) {
    const uint8_t ext = (uint8_t)((ext_mask & PH_EXT_FACTOR ? 1 : 0) | (ext_mask & PH_EXT_VARIABLE ? 2 : 0));
    const uint8_t in = (uint8_t)((int_mask & PH_INT_FACTOR ? 1 : 0) | (int_mask & PH_INT_VARIABLE ? 2 : 0));
    if (!ext && (!in || n_int <= 0)) return;
    if (!w->clog.empty()) {
        mgx_world::CountEntry &b = w->clog.back();
        if (b.ext == ext && b.in == in && b.n_int == n_int && b.robot == robot) { b.times++; return; }
    }
    w->clog.push_back({ext, in, in ? n_int : 0, robot, 1});
    if (w->clog.size() > 4096) flush_counts(w, true);  // (lazy: the robots' sums; the connections are settled when somebody needs their numbers)
}
static void log_change_prior(mgx_world *w, int robot, int var) {
    if (w->n_keyless > 0 && var >= 1 && (w->p.enable_mask & 2u)) {  // the delivery fills inbox keys of factors that lack them
        flush_counts(w);                                           // (what was logged so far saw them missing)
        for (IrConn &c : w->conns) {
            if (c.keys.empty()) continue;
            if (c.owner == robot) c.keys[(size_t)var - 1] |= 1u;
            if (c.other == robot) c.keys[(size_t)var - 1] |= 2u;
        }
    }
    const size_t key = (size_t)robot * (size_t)w->K + (size_t)var;
    if (w->cp_pending.size() <= key) w->cp_pending.resize(w->robots.size() * (size_t)w->K, 0);
    if (w->cp_pending[key]++ == 0) w->cp_dirty.push_back((uint32_t)key);
}
