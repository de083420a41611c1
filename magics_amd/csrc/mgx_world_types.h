// mgx_world_types.h — what the host side is made of: launcher prototypes of the kernel files, error text, device buffers, the pinned argument ring, the neighbour search's state, the resident launches' state, the host mirror's records (Robot, IrConn), connection sets and index, the world itself, the entry hooks of the C ABI (MGX_ENTER).
// Part of ONE translation unit (mgx_world.hip includes its parts in order); not a stand-alone header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mgx.h"
#include "gbp_math.h"
#include "mgx_dev.h"
#include "mgx_grid.h"
#include "mgx_search.h"  // the neighbour search: its dispatch, its pure helpers, the launchers of mgx_topology.hip
#include "mgx_plan_pool.h"  // the global planner's pool of pending requests: slots, tickets, the order they are handed out in
#include "mgx_resident.h"  // resident launches, the host's arithmetic: segments, plan bytes, parity and segment count, back-off, riding updates

namespace mgx {
size_t sweep_lds_bytes(int K, int ir_edges);
size_t sweep_lds_bytes(int K, int ir_edges, bool resident);
int blob_words(int K);
bool sweep_supports(int K);
hipError_t launch_robot_sweep(const DevWorld &w, int robot0, int n_robots, uint32_t ext_mask, uint32_t int_mask, int n_int,
                              int snap_out, uint32_t hints, hipStream_t stream, SweepRan *ran);
int sweep_resident_capacity(const DevWorld &w, bool sharded, uint32_t features);
uint32_t sweep_resident_form(int K, uint32_t features);
size_t sweep_resident_lds_max();
hipError_t launch_robot_schedule(const DevWorld &w, int n_robots, const SegPlan &plan, bool sharded, uint32_t features, bool cooperative,
                                 hipStream_t stream, SweepRan *ran);
hipError_t launch_agree_abort(const DevWorld &w, const SegPlan &plan, hipStream_t stream);
hipError_t launch_change_prior(const DevWorld &w, int n, const int32_t *robots, const uint32_t *vars, const double *means,
                               hipStream_t stream);
hipError_t launch_update_priors(const DevWorld &w, int n, const int32_t *robots, const double *waypoints, const double *time_scale,
                                const uint8_t *what, double max_speed, double delta_t, hipStream_t stream);
hipError_t launch_global_paths(const DevWorld &w, int n, const int32_t *robots, const double *means, double first_last_sigma,
                               double inbetween_sigma, bool reset_tracking, int32_t *mission_target, int n_edges, IrEdgeRec *recs,
                               const uint8_t *selected, hipStream_t stream);
hipError_t launch_halo_pack(const DevWorld &w, int n, const int32_t *robots, double *buf, hipStream_t stream);
hipError_t launch_halo_unpack(const DevWorld &w, int n, const int32_t *ghosts, const double *buf, hipStream_t stream);
hipError_t launch_copy_bytes(uint8_t *dst, const uint8_t *src, size_t n, hipStream_t stream);
hipError_t launch_freeze(const DevWorld &w, uint32_t kinds, hipStream_t stream);
hipError_t launch_ir_freeze(const DevWorld &w, double *frozen_snap, uint32_t *frozen_epoch, hipStream_t stream);
hipError_t launch_thaw_ir(const DevWorld &w, uint8_t *gate, hipStream_t stream);
hipError_t launch_keyless_ir(const DevWorld &w, uint8_t *gate, int n, const KeylessRec *recs, hipStream_t stream);
hipError_t launch_or_bytes(uint8_t *p, int n, uint8_t keep, uint8_t set, hipStream_t stream);
hipError_t launch_thaw(const DevWorld &w, int robot0, int n_robots, uint32_t ext_mask, hipStream_t stream);
hipError_t launch_thaw_done(const DevWorld &w, int robot0, int n_robots, int clear, hipStream_t stream);
hipError_t launch_gather_variable_means(const DevWorld &w, int var, double *out, hipStream_t stream);
hipError_t launch_mission_reached(const DevWorld &w, const DevMission &m, int n, long long tick, unsigned int *ev, hipStream_t stream);
hipError_t launch_mission_positions(const DevMission &m, int n, const int32_t *alive, float *out, hipStream_t stream);
hipError_t launch_mission_prepare(const DevWorld &w, const DevMission &m, int n, const uint8_t *moving, double *rec, int32_t *robots,
                                  double *waypoints, double *time_scale, uint8_t *what, hipStream_t stream);
hipError_t launch_retopo_robots(const DevWorld &w, const RetopoBlock &b, const int32_t *in_old, const IrSlotRec *slots_old, const int32_t *peers_old,
                                int32_t *in_dst, IrSlotRec *slots_new, int32_t *peers_dst, int32_t *var_ptr, int32_t *var_mid, int stride_new,
                                IrEdgeRec *recs, double *fv_eta, double *fv_lam, double *bmu, uint8_t *gate, hipStream_t stream);
hipError_t launch_append_robots(const DevWorld &w, const AppendLayout &l, const AppendTargets &t, hipStream_t stream);
hipError_t launch_var_tables(int R, int K, const int32_t *in_ptr, const int32_t *in_mid, int32_t *var_ptr, int32_t *var_mid,
                             hipStream_t stream);
hipError_t launch_edge_gates(int n, const IrEdgeRec *recs, const uint8_t *antenna, const uint8_t *idle, uint8_t *gate, hipStream_t stream);
hipError_t launch_set_safety(int n_edges, IrEdgeRec *recs, int n_slots, IrSlotRec *slots, int n_robots, const double *radius,
                             double multiplier, hipStream_t stream);
hipError_t launch_halo_push(const DevWorld &w, int n, const int32_t *robots, const unsigned long long *dst, int n_peers,
                            const unsigned long long *peer_flags, unsigned long long seq, unsigned int *done, hipStream_t stream);
hipError_t launch_halo_wait_unpack(const DevWorld &w, int n, const int32_t *ghosts, const double *recv, int n_sources,
                                   const unsigned long long *flags, unsigned long long seq, unsigned long long *err,
                                   long long timeout_ticks, unsigned long long *ready, unsigned long long *host_err, hipStream_t stream);
int env_red_plane(const mgx_env_desc *d, uint32_t resolution, float expansion, float blur_percent, bool with_blur, hipStream_t s,
                  std::vector<uint8_t> &red, uint32_t &W, uint32_t &H);  // mgx_env.hip
// mgx_collisions.hip
hipError_t launch_collisions_pass(const CollDev &c, bool grid, double cell, uint32_t n_buckets, hipStream_t s);
hipError_t launch_collisions_rebits(const CollDev &c, hipStream_t s);
hipError_t launch_env_collisions_pass(const EnvCollDev &c, hipStream_t s);
// mgx_tracks.hip
hipError_t launch_tracks_pass(const TrackDev &t, hipStream_t s);
hipError_t launch_track_metrics_read(int n, const TrackMetricsState *state, TrackMetricsOut *out, hipStream_t s);
// mgx_goal_areas.hip
hipError_t launch_goal_areas_pass(const GoalAreasDev &g, hipStream_t s);
// mgx_planner.hip
hipError_t launch_plan_pool(const PlanDev &c, const PlanPoolDev &pool, int n_active, hipStream_t s);
}  // namespace mgx

using namespace mgx;

static thread_local std::string g_err;
// MGX_TIMING=1: host-side stage times of the topology pass and the table rebuild on stderr (diagnostic); MGX_TIMING=2: the same
// times kept in memory and summed up per stage when the process ends (printing every lap shifts the very phases being looked at)
struct StageTimer {
    struct Sum { const char *what, *stage; double total = 0.0; long n = 0; };
    struct Book {
        std::vector<Sum> rows;
        ~Book() { for (const Sum &r : rows) fprintf(stderr, "[mgx timing] %s: %s n=%ld mean %.1f us\n", r.what, r.stage, r.n, r.total / (double)std::max(r.n, 1L)); }
        void add(const char *what, const char *stage, double dt) {
            for (Sum &r : rows) if (r.what == what && r.stage == stage) { if (++r.n > 0) r.total += dt; return; }
            rows.push_back(Sum{what, stage, 0.0, -7});  // (the first eight of every stage size tables and warm caches: not counted)
        }
    };
    int on;
    double t0;
    const char *what;
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
    explicit StageTimer(const char *w) : what(w) { static const int e = [] { const char *v = getenv("MGX_TIMING"); return v ? (v[0] == '2' ? 2 : 1) : 0; }(); on = e; t0 = on ? now() : 0.0; }
    void lap(const char *stage) {
        if (!on) return;
        const double t = now();
        if (on == 2) { static Book book; book.add(what, stage, t - t0); }
        else fprintf(stderr, "[mgx timing] %s: %s %.1f us\n", what, stage, t - t0);
        t0 = on == 2 ? now() : t;
    }
};
static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(MGX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));    \
    } while (0)

namespace {

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0, cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;  // owns its allocation
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void swap(DevBuf &o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(cap, o.cap);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = cap = 0;
    }
    // (re)allocates only when growing; the copy is enqueued on `s` from pageable memory, so the
    // caller synchronises before `h` dies.  room: elements the allocation holds at least (head-room behind the upload: what a
    // reserved world appends into, mgx_world_reserve)
    hipError_t upload(const std::vector<T> &h, hipStream_t s, size_t room = 0) {
        const size_t want = std::max<size_t>(std::max(h.size(), room), 1);
        if (want > cap) {
            release();
            hipError_t e = hipMalloc((void **)&p, sizeof(T) * want);
            if (e != hipSuccess) return e;
            cap = want;
        }
        n = h.size();
        if (n) return hipMemcpyAsync(p, h.data(), sizeof(T) * n, hipMemcpyHostToDevice, s);
        return hipSuccess;
    }
    hipError_t reserve(size_t want) {  // contents undefined afterwards
        if (want < 1) want = 1;
        if (want > cap) {  // grow with headroom: tables that follow a churning topology would otherwise be
            release();     // re-allocated (a device-wide synchronisation) at every new maximum
            const size_t room = want + want / 4 + 64;
            hipError_t e = hipMalloc((void **)&p, sizeof(T) * room);
            if (e != hipSuccess) return e;
            cap = room;
        }
        n = want;
        return hipSuccess;
    }
    hipError_t download(std::vector<T> &h, hipStream_t s) const {
        h.resize(n);
        if (!n) return hipSuccess;
        return hipMemcpyAsync(h.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost, s);
    }
};

// Pinned, device-mapped host staging for the small per-tick argument lists: the kernels read them
// in place over the host link (tens of KB), so a tick enqueues no copy and never synchronises host
// and device.  A ring of slots, each guarded by an event recorded after the kernel that reads it.
struct StageRing {
    static constexpr int SLOTS = 8;
    void *host[SLOTS] = {};
    size_t cap[SLOTS] = {};
    hipEvent_t ev[SLOTS] = {};
    bool pending[SLOTS] = {};
    int next = 0;
    ~StageRing() {
        for (int i = 0; i < SLOTS; i++) {
            if (ev[i]) { (void)hipEventSynchronize(ev[i]); (void)hipEventDestroy(ev[i]); }
            if (host[i]) (void)hipHostFree(host[i]);
        }
    }
    hipError_t acquire(size_t bytes, void **p, int *slot) {
        const int i = next;
        next = (next + 1) % SLOTS;
        hipError_t e;
        if (!ev[i] && (e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) return e;
        if (pending[i]) {
            if ((e = hipEventSynchronize(ev[i])) != hipSuccess) return e;
            pending[i] = false;
        }
        if (bytes > cap[i] || !host[i]) {  // also for a request of zero bytes (a rank that holds ghosts only): callers map the slot
            if (host[i]) (void)hipHostFree(host[i]);
            host[i] = nullptr;
            cap[i] = 0;
            const size_t want = std::max<size_t>(bytes + bytes / 2, 4096);
            if ((e = hipHostMalloc(&host[i], want, hipHostMallocMapped)) != hipSuccess) return e;
            cap[i] = want;
        }
        *p = host[i];
        *slot = i;
        return hipSuccess;
    }
    hipError_t release(int slot, hipStream_t s) {
        pending[slot] = true;
        return hipEventRecord(ev[slot], s);
    }
};

// mutable state of one robot, item-major (AoS) on the host
struct Robot {
    int K = 0;
    bool ghost = false;
    double radius = 1.0;
    uint64_t order_key = 0;
    uint8_t antenna = 1, idle = 0;
    bool removed = false;  // despawned: never iterated, nothing delivered, invisible to the neighbour search
    std::vector<double> prior_eta, prior_lam, bel_eta, bel_lam, bel_mu, bel_cov;  // [K][4|16]
    std::vector<int32_t> valid;                                                   // [K]
    std::vector<double> snap;                                                     // [K][24]
    std::vector<uint32_t> epoch;                                                  // [K]
    std::vector<double> fv_eta, fv_lam;                                           // [E][4|16]
    std::vector<double> dyn_m;                                                    // [K-1][16]
    std::vector<int32_t> trk_record;                                              // [K-2]
    std::vector<float> trk_last_pos;                                              // [K-2][2]
    std::vector<double> trk_last_val;                                             // [K-2]
    std::vector<float> path;                                                      // [n_path][2]
    int32_t iter_factor = 0;
    // petgraph StableGraph node slots of this robot's graph: K variables, K-1 dynamic, K-2 obstacle
    // and K-2 tracking factors first (robot.rs:1179-1334), inter-robot factors after; vacated slots
    // are reused last-freed-first.  Only the ORDER of the indices matters (inbox key order).
    int n_nodes = 0;
    std::vector<int> free_nodes;
    int alloc_node() {
        if (!free_nodes.empty()) { const int ix = free_nodes.back(); free_nodes.pop_back(); return ix; }
        return n_nodes++;
    }
    // MessageCount of the graph's permanent nodes (variables, dynamic / obstacle / tracking factors):
    // sent internal, sent external, received internal, received external (factorgraph/mod.rs:29-137)
    uint64_t cnt[4] = {0, 0, 0, 0};
    int64_t cnt_itf = 0;  // iteration_count.factor as far as the counters have been advanced
    std::vector<uint32_t> slot_uses;  // per node slot: entries of interrobot_factor_indices naming it
    // run-time switching of factor kinds (mgx_set_enabled): the inbox the internal factors froze with, whether each
    // entry is present, and the kinds still to take their first update from it (empty until the world needs them)
    std::vector<double> frozen;
    std::vector<uint8_t> frozen_flag;
    uint8_t thaw = 0;
    // internal kinds that were switched off when the robot joined and whose factors have not been delivered to since: a factor
    // created switched off takes no message, not even the empty one that gives its inbox its keys (factorgraph.rs:304-330,
    // factor/mod.rs:307-310) — until its variables deliver it sends nothing (frozen_flag 2 on the device, NO_KEY)
    uint8_t nokey = 0;
    std::vector<double> ir_frozen_snap;                   // [K][24] what the variables had sent when inter-robot factors went off
    std::vector<uint32_t> ir_frozen_epoch, ir_thaw_epoch;  // [K]
};
// frozen_flag [E] of a robot that has no frozen inbox yet: empty entries, and NO key at all for the kinds in `nokey`
static inline void nokey_flags(uint8_t nokey, int K, uint8_t *fl) {
    const int n_dyn = 2 * (K - 1), E = 4 * K - 6;
    for (int e = 0; e < E; e++) {
        const uint8_t bit = e < n_dyn ? 1u : (e < n_dyn + (K - 2) ? 4u : 8u);
        fl[e] = (nokey & bit) ? 2 : 0;
    }
}

struct IrEdge {  // one InterRobotFactor, kept at its target variable
    double fv_eta[4] = {0, 0, 0, 0}, fv_lam[16] = {0}, bmu[4] = {0, 0, 0, 0};
    uint32_t created = 0;
    bool fresh = true;  // created since the last commit: state is initialised at commit
};
struct IrConn {  // K-1 factors owner -> other
    // (what the per-tick host passes over ALL connections read — counters, table rebuild — sits in the first cache line)
    int owner, other;
    // (its slot in the target's incoming list on the device and "some edge is still fresh" live in mgx_world::conn_hot)
    uint64_t first_number;
    uint64_t cnt[4] = {0, 0, 0, 0};  // MessageCount summed over the K-1 factors
    // Sum over the factors of how often each one's node slot occurs in the owner's
    // interrobot_factor_indices: that list is never pruned (factorgraph.rs:729-733), so a factor in a
    // re-used slot is updated once per occurrence in every external sweep — same message, but every
    // update counts as sent / received.
    uint64_t updates_per_sweep = 0;
    int node_first = 0, node_last = 0;  // node[0], node.back(): what orders two connections of one owner in an inbox
    // Everything `cnt` counts is a function of what its two robots have run since the counters were last brought up to date
    // (internal / external variable sweeps, external factor sweeps, prior changes of variables that carry inter-robot factors:
    // mgx_world::cum) under flags that do not change in between — so a connection is SETTLED (settle_conn) only when somebody
    // needs its numbers: a read, a switch of flags or kinds, its deletion; the per-tick topology pass no longer walks every
    // connection for it.  base: the robots' cumulative counts when the connection was settled last.
    uint64_t base[5] = {0, 0, 0, 0, 0};  // owner's nIv, target's nEv, owner's nEf, owner's / target's prior changes
    std::vector<IrEdge> edges;  // index i-1 for variable i
    std::vector<int> node;      // node slot of each factor in the owner's graph
    // Factors created while their kind is switched off drop the two messages that would have filled their inbox
    // (factor/mod.rs:307-310), and FactorNode::update answers inbox KEYS: once enabled, such a factor sends nothing to
    // a variable that has not delivered to it yet.  The messages themselves are handled on the device (delivery
    // counts); this is the same knowledge for the counters: per factor, bit 0 = the own variable's key is there,
    // bit 1 = the foreign variable's; `uses` = the factor's share of updates_per_sweep.  Empty: every key is there.
    std::vector<uint8_t> keys;
    std::vector<uint32_t> uses;
};

// RobotConnections::robots_connected_with of every robot (robot.rs:515-531), ascending order key — ONE contiguous pool, rows of a
// fixed capacity: the topology pass walks every robot's set every tick, and a thousand separately allocated vectors are a
// thousand cache misses.  `keys`: the robots' order keys, compact, for the merges of that pass.
struct ConnSets {
    int cap = 16;
    std::vector<int32_t> ids, cnt;
    std::vector<uint64_t> keys;
    std::vector<uint8_t> ghost;   // the robots' ghost flags and radii, compact like the keys (fixed when a robot is added): the
    std::vector<double> radius;   // per-tick passes over all connections read them instead of the robots themselves
    std::vector<uint8_t> removed; // ... and Robot::removed (mgx_robot_remove)
    std::vector<uint32_t> group;  // mgx_robot_desc::group of every robot (include/mgx.h, ROBOT GROUPS), fixed when it is added
    size_t n_grouped = 0;         // robots of a non-zero group: the world is GROUPED when there are any
    // ids ascending == order keys ascending?  (the rule: robots get their keys in the order they are added.)  Looked at once per
    // robot count: the per-tick merges then compare ids instead of looking two keys up per comparison.
    size_t mono_n = 0;
    bool mono = true;
    bool monotone() {
        if (mono_n != keys.size()) {
            mono = true;
            for (size_t r = 1; r < keys.size() && mono; r++) mono = keys[r - 1] < keys[r];
            mono_n = keys.size();
        }
        return mono;
    }
    void ensure(size_t n) {
        if (cnt.size() < n) { cnt.resize(n, 0); ids.resize(n * (size_t)cap, 0); }
    }
    int32_t *row(size_t r) { return ids.data() + r * (size_t)cap; }
    const int32_t *row(size_t r) const { return ids.data() + r * (size_t)cap; }
    void grow() {
        const int nc = cap * 2;
        std::vector<int32_t> ni(cnt.size() * (size_t)nc, 0);
        for (size_t r = 0; r < cnt.size(); r++) std::copy(row(r), row(r) + cnt[r], ni.begin() + (long)(r * (size_t)nc));
        ids.swap(ni);
        cap = nc;
    }
    bool has(size_t r, int id) const { return std::find(row(r), row(r) + cnt[r], id) != row(r) + cnt[r]; }
    void insert_sorted(size_t r, int id) {  // keeps the row ascending in order key
        if (cnt[r] == cap) grow();
        int32_t *b = row(r), *e = b + cnt[r];
        int32_t *at = std::upper_bound(b, e, id, [&](int x, int y) { return keys[(size_t)x] < keys[(size_t)y]; });
        std::copy_backward(at, e, e + 1);
        *at = id;
        cnt[r]++;
    }
    void erase(size_t r, int id) {
        int32_t *b = row(r), *e = b + cnt[r];
        cnt[r] = (int32_t)(std::remove(b, e, id) - b);
    }
};

// RCCL, resolved at run time (no link-time dependency): the copy already in the process (a host that
// runs torch.distributed has one) or the system library.  Only what the halo exchange needs.
struct RcclApi {
    typedef int (*get_unique_id_t)(void *);
    struct Id128 { char internal[128]; };
    typedef int (*comm_destroy_t)(void *);
    typedef int (*group_t)(void);
    typedef int (*sendrecv_t)(void *, size_t, int, int, void *, hipStream_t);
    typedef const char *(*error_string_t)(int);
    get_unique_id_t get_unique_id = nullptr;
    int (*comm_init_rank)(void **, int, Id128, int) = nullptr;
    comm_destroy_t comm_destroy = nullptr;
    group_t group_start = nullptr, group_end = nullptr;
    sendrecv_t send = nullptr, recv = nullptr;
    error_string_t error_string = nullptr;
    bool tried = false, ok = false;
    bool load() {
        if (tried) return ok;
        tried = true;
        void *h = dlopen(nullptr, RTLD_NOW);  // symbols already in the process
        if (!h || !dlsym(h, "ncclCommInitRank")) {
            h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        }
        if (!h) return false;
        get_unique_id = (get_unique_id_t)dlsym(h, "ncclGetUniqueId");
        comm_init_rank = (int (*)(void **, int, Id128, int))dlsym(h, "ncclCommInitRank");
        comm_destroy = (comm_destroy_t)dlsym(h, "ncclCommDestroy");
        group_start = (group_t)dlsym(h, "ncclGroupStart");
        group_end = (group_t)dlsym(h, "ncclGroupEnd");
        send = (sendrecv_t)dlsym(h, "ncclSend");
        recv = (sendrecv_t)dlsym(h, "ncclRecv");
        error_string = (error_string_t)dlsym(h, "ncclGetErrorString");
        ok = get_unique_id && comm_init_rank && comm_destroy && group_start && group_end && send && recv;
        return ok;
    }
};
static RcclApi g_rccl;
constexpr int NCCL_FLOAT64 = 8;  // ncclFloat64 (rccl.h)

// Pinned, device-mapped host memory the search's positions go up from and its rows come back into: copies to and from pageable
// memory (std::vector) are staged by the runtime, tens of microseconds each
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    // keep: the first bytes of the block that move along when it grows (the rest is undefined afterwards)
    hipError_t reserve(size_t bytes, size_t keep = 0) {
        if (bytes <= cap) return hipSuccess;
        void *q = nullptr;
        const size_t want = bytes + bytes / 2 + 4096;
        const hipError_t e = hipHostMalloc(&q, want, hipHostMallocMapped);  // the one-pass search reads and writes it in place
        if (e != hipSuccess) return e;
        if (p) {
            memcpy(q, p, std::min(keep, cap));
            (void)hipHostFree(p);
        }
        p = q;
        cap = want;
        return hipSuccess;
    }
};

// The comms-range neighbour search of a world: everything it owns between calls.  mgx_world_topology.inc drives it
// (neighbours_enqueue / neighbours_collect), mgx_search.h says which kernel of mgx_topology.hip answers which query.
struct NeighbourSearch {
    DevBuf<float> pos;  // the query's positions on the device (the two-pass search's copy, a mission's Transforms)
    DevBuf<int32_t> cnt, bucket_cnt, bucket_ptr, cursor, members, special, nspecial, ptr, idx;  // the two-pass search's scratch and rows
    SearchScratch scratch() const { return {cnt.p, bucket_cnt.p, bucket_ptr.p, cursor.p, members.p, special.p, nspecial.p, ptr.p}; }
    size_t last_total = 0;  // rows of the last search: sizes the speculative second pass of the next one
    int row_cap = 16;       // one-pass searches: capacity of a row (grown to what the largest row needed)
    // The rows of the last topology pass's search, kept on the device: after a pass a robot's connection set IS its row, so the
    // next search can say which robots' rows changed (k_grid_rows) and the host's pass looks at those only.  prev_valid: the
    // kept rows are the sets — false whenever the sets were touched by anything but a pass that compared against them.
    DevBuf<int32_t> prev;
    bool prev_valid = false;
    size_t prev_n = 0;
    void sets_touched() { prev_valid = false; }  // the connection sets change outside a topology pass
    hipStream_t stream = nullptr, last_stream = nullptr;  // searches over host-supplied positions run beside the world's stream
    bool last_stream_set = false;                         // (last_stream: the one that last used the shared buffers)
    PinBuf pin;
    std::vector<float> packed;  // the callers' positions without the removed robots' (scratch)
    std::vector<uint8_t> chg;   // the rows-changed flags taken out of the counts (scratch; what mgx_last_search copies)
    // a grouped world's search (k_group_rows): the query listed by group, on the host and on the device (members, seg, wg behind one
    // another) — built again only when the robots of the query are not the ones it was built for
    GroupTables groups;
    std::vector<int> groups_alive;
    bool groups_valid = false;
    DevBuf<int32_t> groups_d;
    std::vector<int32_t> groups_host;  // (scratch of the upload)
    // the last search (mgx_last_search): the kernel it launched last, written by the branch that launched it, with which row
    // capacity, in how many launches — and how many robots' changed-row flags reached the pass behind it (-1: none did)
    int32_t last_kernel = MGX_SEARCH_NONE, last_cap = 0, last_launches = 0, last_changed = -1;
    // a search that has been enqueued and not collected yet: what both strategies need, then one part per strategy
    struct PendingSearch {
        bool valid = false;
        hipStream_t stream = nullptr;  // where it was enqueued
        int n = 0, n_all = 0;          // robots in the query, robots of the world
        std::vector<int> alive;        // the world ids of the robots in the query
        bool compact = false, from_missions = false;
        float radius = 0.f;
        std::vector<float> radii;  // a grouped search's radius per GROUP id (empty: `radius` for every group)
        uint32_t method = 0;
        bool grouped = false;  // a grouped world's search: k_group_rows over NeighbourSearch::groups
        bool in_rows = false;  // the one-pass kernel with rows of a fixed capacity (`rows`), else count / scan / fill (`csr`)
        struct { int cap = 0; bool has_chg = false; } rows;  // has_chg: the counts carry "this robot's row changed" (see prev)
        struct Csr { size_t guess, off_ptr, off_idx; uint32_t M; bool grid; } csr{};  // the guessed buffer, where the pinned block holds what
    } mission;  // the coming tick's search, enqueued by mgx_mission_tick_end
};

// A block of host-mapped words the device writes and the host polls (a launch's verdict, a lingering launch's box): zeroed when
// it is made, freed with its owner
struct MappedBlock {
    void *p = nullptr;
    MappedBlock() = default;
    MappedBlock(const MappedBlock &) = delete;
    MappedBlock &operator=(const MappedBlock &) = delete;
    ~MappedBlock() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; }
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped);
        if (e == hipSuccess) memset(p, 0, bytes);
        return e;
    }
};

// A schedule (or the part of one that fits a launch) handed to the device that may have to be taken back: the resident launch
// whose census verdict the host has not seen, and the post a lingering launch has not taken yet.  Everything needed to undo the
// host's bookkeeping and run the same segments again launch by launch.
struct Submitted {
    bool active = false;
    unsigned long long number = 0;  // the world's launch number it went out under
    std::vector<Launch> plan;       // its segments
    Standing before;                // where the world stood when it went out
    bool partial = false;           // a launch that is not the first of its schedule (more than MAX_SEGS segments)
    uint32_t schedules = 1;         // a post: the schedules merged into its plan (mgx_set_post_merge)
    // the prior updates that ride in it.  A launch: where the kernel read them, and the ring slot a re-run guards again (the event
    // behind a declined launch completed at once).  A post: host = its slot of records in the box, nothing else.
    RidingUpdates upd;
    void take_back(mgx_world *w);   // the world stands where it stood before; nothing of the schedule counts as launched
};

// The resident and lingering schedule launches of a world (SegPlan, LingerBox: mgx_dev.h): everything their host side owns
// between calls.  mgx_world_launch.inc drives it (run_resident, confirm_resident, the linger_* functions); the entry points
// of the C ABI come through MGX_ENTER, commit and confirm_resident, and the table builds of mgx_world_commit.inc tell it what
// they changed through the methods below.  mgx_resident.h holds its arithmetic.
struct ResidentLaunches {
    // progress words, the abort word, the census' per-group counts and decision word (with its host-mapped copy), the exchange
    // records of the local robots' variables in two parities
    DevBuf<unsigned long long> sweep_flag_buf, sweep_abort_buf, census_buf, decision_buf;
    DevBuf<unsigned char> xrec_buf;
    MappedBlock decision_mem;
    unsigned long long *decision_host() const { return (unsigned long long *)decision_mem.p; }
    // the peer table: [R + 1 row pointers | entries] (current / being built by a topology change)
    DevBuf<int32_t> peer_ptr_dev, peer_ptr_dev_b;
    size_t peer_idx_off = 0;
    std::vector<int32_t> peer_fill;
    bool peers_valid = false;
    unsigned long long flag_base = 0;   // the segment count: every progress word is below or at this value between launches
    unsigned long long launch_seq = 0;  // the number of the last launch or post
    enum Mode : int32_t { OFF = 0, ON = 1, DECLINE = 2 } mode = ON;  // mgx_set_resident_launches
    Backoff backoff;
    // workgroups of the resident kernel the device holds at once, per flavour (unsharded, sharded) and form (SWEEP_F_* mask): asked
    // of the instantiation that will run; -1: not asked yet
    int cap[2][8] = {{-1, -1, -1, -1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1, -1, -1}};
    void forget_capacity() { for (auto &f : cap) for (int &c : f) c = -1; }
    int capacity_for(const DevWorld &d, bool sharded, uint32_t form) {  // (asked of the runtime once per topology)
        int &c = cap[sharded ? 1 : 0][form & 7u];
        if (c < 0) c = sweep_resident_capacity(d, sharded, form);
        return c;
    }
    // The form the world's resident launches take (mgx_dev.h, SWEEP_F_*).  specialize: 1 = the smallest form that covers the launch,
    // 0 = always the full one (mgx_set_specialize, MGX_SPECIALIZE; -1: not asked yet).  upd_seen: a schedule with prior updates has
    // come this way — from then on every launch can take them, so a caller who alternates mgx_iterate and mgx_tick ends a
    // lingering launch for it once, not at every tick.
    int32_t specialize = -1;
    bool upd_seen = false;
    uint64_t aborts = 0, launches = 0;
    Submitted pending;      // the launch the host has enqueued but not yet seen decided (go / abort)
    RidingUpdates riding;   // the prior updates of the schedule being submitted (run_schedule sets and clears them)
    // LINGERING resident launches (mgx_dev.h): the host's side of the box.  `open`: a launch that lingers is in flight — every
    // entry point but mgx_iterate / mgx_tick (and the pure queries) ends it first (MGX_ENTER, commit); those two POST their schedule
    // into it when it qualifies (run_resident).  At most one post is outstanding without the launch's word for it (`un`): what
    // is needed to take it back and run it as a launch of its own if the launch ended first.
    struct Linger {
        long long ticks = -1;  // wall-clock ticks (100 MHz) a robot's workgroup waits for the next post; -1: not asked yet, 0: off
        MappedBlock box_mem;   // the box, then two blocks of prior-update records
        LingerBox *box() const { return (LingerBox *)box_mem.p; }
        size_t upd_stride = 0;  // f64 words per slot of prior-update records behind the box
        DevBuf<unsigned long long> go;
        DevBuf<unsigned char> dev;  // the launch's device-side slots (the postman's copies of the posts): [2][dev_stride]
        size_t dev_stride = 0;
        bool open = false, hold = false;
        unsigned long long seq0 = 0;       // number of the open launch's own plan
        SweepRan ran;                      // the open launch's instantiation (what a post runs in)
        uint32_t taken_in_launch = 0;      // posts the open launch has taken
        int useless = 0;                   // lingering launches in a row that ended without having taken a post
        uint32_t streak = 0;               // schedules issued back to back, this one included (no other call on the world in between)
        Submitted un;
        uint64_t launches = 0, posts = 0, reruns = 0, ended_by_device = 0;  // (posts, reruns: SCHEDULES, however they were grouped)
        // merging back-to-back schedules into one post (post_merge_decide, mgx_resident.h): the switch, the schedules in the plan
        // being submitted (linger_post takes the number; 1 outside submit_batch), and what was posted as how many plans
        int32_t merge_mode = -1;  // PostMergeMode; -1: not asked yet (MGX_POST_MERGE)
        uint32_t coming = 1;
        uint64_t plans_posted = 0, schedules_in_plans = 0, largest_plan = 0;
    } linger;
    // ---- what the rest of the host tells it ----
    void arrays_rebuilt() {  // commit laid the device arrays out again: progress words are re-created (zero), the count starts over
        peers_valid = false;
        sweep_flag_buf.n = 0;
        flag_base = 0;
        forget_capacity();
    }
    // commit appended robots behind the ones on the device (append_robots): progress words and exchange records are re-created
    // for the new count (a launch's first segment reads snapshots, not records) and the peer table is built again — row pointers
    // and entries share one array whose split moves with the count; the capacity asked of the runtime stays: it follows the
    // LDS footprint, which a robot without connections does not change
    void robots_appended() {
        peers_valid = false;
        sweep_flag_buf.n = 0;
        flag_base = 0;
    }
    // the resident kernel's LDS per workgroup (hence workgroups per CU) follows the largest number of edges on one robot: a
    // capacity asked for a sparser topology says nothing about this one
    void lds_footprint_changed() { forget_capacity(); }
    // retopo built the peer table of the new topology beside the edge tables (or could not: no resident launches on this world now)
    void peers_rebuilt(bool built, size_t R, DevWorld &d) {
        if (built) {
            peer_ptr_dev.swap(peer_ptr_dev_b);
            peer_idx_off = R + 1;
            d.peer_ptr = peer_ptr_dev.p;
            d.peer_idx = peer_ptr_dev.p + peer_idx_off;
        }
        peers_valid = built;
    }
    void set_mode(int32_t enabled) { mode = enabled == 0 ? OFF : enabled == 2 ? DECLINE : ON; }
    void set_linger(int32_t microseconds) {  // negative: as the environment says (asked again at the next launch)
        linger.ticks = microseconds >= 0 ? (long long)std::min(microseconds, 1000000) * 100ll : -1;
        linger.useless = 0;
    }
    void schedule_issued() { linger.streak++; }  // mgx_iterate / mgx_tick
    void other_call() { linger.streak = 0; }     // every other entry point (MGX_ENTER)
};

}  // namespace

// Incoming inter-robot connections of every local robot in inbox key order (graph key, node index
// — message.rs / id.rs:19-117), and the split between lower-key and higher-key owners.  Each
// connection hangs one factor on every variable 1..K-1 of its target, and the order is the same for
// all of them: by owner key, and for two connections of one owner by node slot — a connection's K-1
// slots are one block of consecutive indices (fresh, or a whole vacated block: alloc_node), so
// comparing the first slots orders the whole blocks.  Edge (variable i, list position q) of robot r
// lives at  (K-1) * in_ptr[r] + (i-1) * n_in(r) + q.
struct Incoming {
    std::vector<int32_t> in_ptr, in_list, mid;
    // on request: the resident kernel's peer table (ensure_resident_tables) from the same two passes over the connections —
    // [R + 1 row pointers | entries]: for every local robot the owners of its incoming and the targets of its outgoing connections
    std::vector<int32_t> peers;
    std::vector<int32_t> fill, pfill;  // scratch of build_incoming
    int ir_max_edges = 0;
    bool blocks_ok = true;
};

// Who points at whom, kept IN STEP with the connection list (ir_connect, ir_disconnect_batch) instead of being derived from it in
// two passes over every connection whenever a topology pass has changed something: per robot id the connections it is the TARGET
// of — in the order of its variables' inboxes (owner's order key, then node slot: build_incoming) — and the ones it OWNS (no
// order).  Entries are indices into the connection list, which closes its holes by moving the last survivors into them: a move
// rewrites the mover's two entries.  Anything the index is not told about (ir_disconnect, a robot that changes sides) just
// invalidates it: the next use builds it again from the list.
struct ConnIndex {
    bool valid = false;
    bool interleaved = false;  // node slots of two connections of one owner towards one target interleave (never: reported)
    std::vector<std::vector<int32_t>> in, out;
};

struct mgx_world {
    mgx_params p{};
    std::vector<Robot> robots;  // ids = indices; ghosts may interleave on the host, device order below
    std::vector<IrConn> conns;
    ConnSets sets;  // robots_connected_with of every robot
    std::vector<uint8_t> sdf_red;
    uint32_t sdf_w = 0, sdf_h = 0;
    double world_w = 1.0, world_h = 1.0;
    // the reciprocal of the obstacle factors' jacobian_delta the kernels may divide with, and the delta it was checked for
    // (gbp_math.h, obstacle_inv_delta: 65 536 quotients, so once per delta and not once per commit)
    double obs_delta_checked = 0.0, obs_inv_delta = 0.0;
    int K = 0;

    hipStream_t stream = nullptr;
    bool dirty = true;       // robots / image changed since the device arrays were built: commit() has robots to bring onto the device
    bool relayout = true;    // ... and not only robots were added (image, shard calls, edits of the host mirror): full rebuild.  relayout implies dirty
    // mgx_world_reserve: the robots the world expects to hold (0: never asked), the robots the per-robot device arrays of the
    // layout there now have room for (== d.R_local on a world that never asked: today's arrays), and what mgx_append_stats counts
    uint32_t reserve_want = 0;
    int R_cap = 0;
    uint64_t n_appends = 0, n_robots_appended = 0, n_append_fallbacks = 0;
    bool conns_dirty = false;  // only inter-robot connections changed: edge tables are rebuilt in place
    bool flags_dirty = true;
    bool dev_valid = false;  // device arrays hold live state
    uint64_t n_layouts = 0, n_pulls = 0;  // full rebuilds of the device arrays in commit(), pull()s that downloaded (mgx_layout_stats)
    bool frozen_live = false;     // the frozen-inbox arrays exist (a kind has been switched at run time)
    uint32_t thaw_kinds = 0;      // kinds some robot may still be thawing: k_thaw runs before sweeps with a factor phase
    DevBuf<double> frozen_buf;
    DevBuf<uint8_t> frozen_flag_buf, thaw_buf, skip0_buf;
    bool ir_frozen_live = false;  // ir_frozen_* hold what the variables had sent when inter-robot factors were switched off
    bool ir_thaw_active = false;  // inter-robot factors are back and some owner may not have delivered since
    DevBuf<double> ir_frozen_snap_buf;
    DevBuf<uint32_t> ir_frozen_epoch_buf, ir_thaw_epoch_buf;
    bool trk_ever_on = false;  // tracking factors were enabled at some point: their message columns may be non-zero
    uint32_t stale_kinds = 0;  // disabled factor kinds whose inboxes have missed a delivery (mgx_set_enabled)
    DevWorld d{};
    std::vector<int> dev_of;     // robot id -> device robot index (locals first, then ghosts)
    std::vector<int> robot_of;   // device robot index -> robot id

    DevBuf<double> blob, snap0, snap1, dyn_m, trk_last_val, ir_fv_eta, ir_fv_lam, ir_bmu;
    DevBuf<IrEdgeRec> ir_rec;
    DevBuf<double> ir_fv_eta_b, ir_fv_lam_b, ir_bmu_b;  // second set: the edge tables are rebuilt out of place
    DevBuf<IrEdgeRec> ir_rec_b;
    DevBuf<int32_t> in_ptr_dev, in_ptr_dev_b, in_mid_dev;  // per-robot slot ranges (current / being built), split index
    DevBuf<IrSlotRec> slot_recs, slot_recs_b;  // slot records of the layout on the device (current / being built): what a robot whose incoming list did not change keeps
    std::vector<int32_t> dev_in_ptr;  // [R_local + 1] incoming-slot ranges of the tables now on the device
    DevBuf<int32_t> trk_record, path_ptr, iter_factor, ir_var_ptr, ir_var_mid;
    DevBuf<uint32_t> epoch0, epoch1;
    DevBuf<float> trk_last_pos, path_xy;
    DevBuf<uint8_t> ir_gate, antenna, idle, sdf;
    DevBuf<double> radius_dev;  // [R_total] the robots' radii by device index (laid out by commit): what mgx_set_safety_multiplier rewrites d_safe from
    StageRing stage;  // packed per-tick arguments
    unsigned long long *sweep_err_host = nullptr;  // host-mapped; non-zero once a wait inside a resident launch (or the direct halo's) gave up
    // mgx_batch_begin .. mgx_batch_end: the schedules mgx_iterate was handed since the last submission, one after the other (what
    // iterate(a); iterate(b) computes is what iterate(a ++ b) computes), the launches they were submitted as and how many of them
    struct Batch {
        bool open = false;
        std::vector<uint8_t> steps;
        uint32_t schedules = 0, submissions = 0, launches = 0;
        uint32_t implicit = 0;  // schedules in `steps` that mgx_iterate recorded by itself, outside a batch (post merging)
    } batch;
    // One schedule per robot group (mgx_iterate_groups): the robots' groups by device index as they were uploaded last (again only
    // when the layout has changed them), the segment records of a mixed call's launches, and what mgx_group_schedule_stats reports
    struct GroupSchedules {
        std::vector<uint32_t> group_of;  // [R_local] what group_of_d holds
        DevBuf<uint32_t> group_of_d;
        DevBuf<GroupSeg> seg_d;          // [launches of the call][groups]
        uint64_t mixed_calls = 0, mixed_launches = 0, sat_out = 0;
    } gsched;
    // Enabled factor kinds per robot group (mgx_set_group_enabled).  A group has a mask of its own only where it was given one that
    // differs from the world's in an INTERNAL kind (bits 1, 4, 8); every other group follows w->p.enable_mask.  The world is MASKED
    // while there is such a group: its schedules all run as group plans (run_group_plan), whose launches read the table.
    struct GroupKinds {
        std::vector<uint8_t> has;       // [groups given a mask] 1: `mask` holds the group's own
        std::vector<uint32_t> mask;
        std::vector<uint8_t> populated; // [groups] a robot of the group has been added at some point: the kinds are fixed
        uint32_t n_masked = 0;          // groups with a mask of their own: the world is masked when there are any
        DevBuf<uint32_t> table_d;       // [groups of the last upload] the kinds by group id
        std::vector<uint32_t> table;    // what table_d holds
        uint64_t masked_plans = 0, masked_launches = 0;  // mgx_group_enabled_stats
        // mgx_set_group_resident: the world's equal schedules take the resident kernel's masked form (SWEEP_F_GRP) — launches of
        // that form, schedules posted into one, schedules that ran as group plans all the same (mgx_group_resident_stats)
        bool resident = false;
        uint64_t res_launches = 0, res_posts = 0, res_fallbacks = 0;
        // Factor sigmas per robot group (mgx_set_group_sigmas): a group has sigmas of its own only where it was given a set that
        // differs from the world's.  Fixed before the group's first robot, as the kinds are (`populated`); a world with such a
        // group counts as masked — ONE predicate for "the groups differ, in kinds or in sigmas" — and its launches read a second
        // table beside the kinds': {inv_s2_obs, inv_s2_ir, inv_s2_trk} by group id (sigma_dynamics is baked into the robots' dyn_m)
        std::vector<uint8_t> sig_has;   // [groups given sigmas] 1: `sig` holds the group's own
        std::vector<mgx_group_sigmas> sig;
        uint32_t n_sigma = 0;           // groups with sigmas of their own
        DevBuf<double> sig_d;           // [groups of the last upload][GROUP_SIGMA_W]
        std::vector<double> sig_table;  // what sig_d holds
        bool masked() const { return n_masked != 0 || n_sigma != 0; }
    } gkinds;
    // the factor sigmas of group g: the group's own, else the world's
    mgx_group_sigmas sigmas_of_group(uint32_t g) const {
        if (g < gkinds.sig_has.size() && gkinds.sig_has[g]) return gkinds.sig[g];
        return mgx_group_sigmas{p.sigma_dynamics, p.sigma_interrobot, p.sigma_obstacle, p.sigma_tracking};
    }
    // the enabled kinds of group g / of robot r (an id): the group's own internal kinds, the world's inter-robot bit
    uint32_t kinds_of_group(uint32_t g) const { return g < gkinds.has.size() && gkinds.has[g] ? ((gkinds.mask[g] & 13u) | (p.enable_mask & 2u)) : p.enable_mask; }
    uint32_t kinds_of_robot(size_t r) const { return gkinds.n_masked ? kinds_of_group(sets.group[r]) : p.enable_mask; }
    ResidentLaunches res;// resident and lingering schedule launches: their words and tables, the launch not yet decided, the open launch and its post
    int sticky_rc = 0;       // a declined launch whose re-run failed inside a call that cannot report it (flush_counts): every
                             // later sweep, read-back and mgx_synchronize reports it (check_device_error)
    // what the per-tick table rebuild reads of EVERY connection, 16 bytes apiece beside the connections themselves (168 bytes and
    // four vectors each): kept in step wherever the list changes (ir_connect, ir_disconnect, ir_disconnect_batch)
    struct ConnHot {
        int32_t owner, other, node_first, node_last;
        uint64_t first_number;
        int32_t dev_q;      // position of this connection in its target's incoming list ON THE DEVICE (-1: not there; its slot is dev_in_ptr[target] + dev_q) — kept HERE only
        uint8_t has_fresh;  // some edge still carries `fresh` (created since the device tables were last laid out) — kept HERE only
    };
    std::vector<ConnHot> conn_hot;
    ConnIndex cidx;
    // per robot, cumulative since the world began: internal variable sweeps run, external variable sweeps, external factor sweeps,
    // prior changes of variables that carry inter-robot factors — what the connections' counters are settled against (IrConn::base)
    struct Cum { std::vector<uint64_t> nIv, nEv, nEf, on_ir; } cum;
    bool conns_unsettled = false;  // some flush since the last full one left the connections' counters behind (lazy)
    std::vector<uint8_t> scratch_dead;    // ir_disconnect_batch's scratch
    std::vector<int32_t> scratch_dead_list;
    std::vector<int> scratch_gone;
    std::vector<int> scratch_victim;      // topology_bookkeeping's scratch
    // storage of deleted connections' edge and node lists, handed to the connections created next (a topology pass deletes and
    // creates dozens per tick: 3 KB from the allocator and back for each was a third of the pass's bookkeeping)
    std::vector<std::vector<IrEdge>> pool_edges;
    std::vector<std::vector<int>> pool_nodes;
    std::vector<std::pair<int, int>> scratch_fresh;
    Incoming retopo_tables;               // scratch of the full table builds (MGX_CHECK_INDEX, ensure_resident_tables)
    // retopo as DIFFERENCES (a world that follows its topology changes a few dozen of its thousands of connections per tick): which
    // robots' incoming lists / peer lists changed since the device tables were laid out (marked where the connection index is
    // edited), and what stays from tick to tick on the host — the lower / higher key split of every local robot.  `all`: every
    // robot counts as changed (after commit(), after the index was rebuilt from the list, before the first retopo).
    struct RetopoInc {
        bool all = true;
        std::vector<uint8_t> in_mark, peer_mark;     // [robot ids]
        std::vector<int32_t> in_changed, peer_changed;  // the ids marked
        std::vector<int32_t> mid;                    // [R_local] the lower / higher key split of every robot's list on the device
        std::vector<int32_t> in_ptr;                 // per-retopo scratch (storage kept)
        std::vector<uint8_t> mark;                   // [R_local] this pass sends the robot's piece
        void mark_in(int32_t id) {
            if ((size_t)id >= in_mark.size()) in_mark.resize((size_t)id + 1, 0);
            if (!in_mark[(size_t)id]) { in_mark[(size_t)id] = 1; in_changed.push_back(id); }
        }
        void mark_peer(int32_t id) {
            if ((size_t)id >= peer_mark.size()) peer_mark.resize((size_t)id + 1, 0);
            if (!peer_mark[(size_t)id]) { peer_mark[(size_t)id] = 1; peer_changed.push_back(id); }
        }
        void clear_marks() {
            for (int32_t id : in_changed) in_mark[(size_t)id] = 0;
            for (int32_t id : peer_changed) peer_mark[(size_t)id] = 0;
            in_changed.clear();
            peer_changed.clear();
        }
    } rinc;
    // missions on the device (mgx_mission_*): host copies of what mgx_mission_set gave, the device arrays, the
    // host-mapped event list of robots that reached their last waypoint, and the tick counter
    struct Mission {
        bool any = false, dirty = false, uploaded = false;
        std::vector<std::vector<double>> wp;  // per robot: [n][2]
        std::vector<int32_t> target;
        std::vector<int32_t> legs_left;       // further legs behind the route (mgx_mission_desc.legs_after; the device counts it down)
        std::vector<uint32_t> vars;           // [R][2]
        std::vector<float> dist2, translation;  // [R][2], [R][3]
        std::vector<double> time_scale;
        std::vector<uint8_t> has;
        std::vector<long long> finished_tick;
        DevBuf<int32_t> wp_ptr_d, target_d, alive_d, robots_d, legs_d;
        DevBuf<double> wp_xy_d, time_scale_d, rec_d, waypoints_d, ts_list_d;
        DevBuf<uint32_t> vars_d;
        DevBuf<float> dist2_d, translation_d;
        DevBuf<uint8_t> has_d, moving_d, what_d;
        DevBuf<long long> finished_d;
        unsigned int *ev_host = nullptr;  // mapped: [0] count, [1 ..] robot ids
        size_t ev_cap = 0;
        std::vector<int32_t> alive_host;  // the robots the search of the coming tick looks at
        bool alive_dirty = true;
        long long tick_no = 0;
        bool in_tick = false;                // between mgx_mission_tick_begin and _end
        std::vector<int32_t> last_finished;  // robots whose mission completed in the last begin, ascending
        std::vector<int32_t> last_leg_ended; // robots that ended a leg with legs left in the last begin, ascending (Idle since)
        float search_radius = 0.f;           // what the last tick's topology pass searched with: the coming tick's search is enqueued
        uint32_t search_method = 0;          //   with the same (mgx_mission_tick_end), used if the next begin asks for the same
        std::vector<float> search_radii;     // ... per group where the last begin had one radius per group (else empty)
        bool search_known = false;
        float *tr_host = nullptr;            // pinned: Transforms after the last tick's move (valid after the next synchronisation)
        size_t tr_cap = 0, tr_n = 0;
        DevMission d{};
    } mission;
    // What the observers — the passes mgx_mission_tick_end enqueues beside the GBP schedule: the contact books, the trackers, the
    // goal areas — read of the robots, kept ONCE (mgx_world_observers.inc) and keyed by robot id, so a relayout moves nothing.
    // robots.size() never shrinks: every array that follows the robots, here and in the observers, is sized again when R > n_sized,
    // with room for observers_room(R) robots when it is outgrown.  Lifetime: switching an observer off releases its own state only;
    // these inputs live until mgx_world_destroy.  The radii never change after mgx_robot_add, so the first n_sized are complete
    // whoever sized them: an observer switched on later uploads nothing.  `radius` moves only when robots have joined, and every
    // observer sizes itself again then: the pointers kept in the passes' argument structs stay good.  `pos` and `flags` are written
    // by every _update call, on the world's stream: the copy of one call is ordered behind the pass of the call before, so each
    // pass reads its own; where they have to grow, DevBuf::reserve frees them with hipFree, which waits for the device.
    struct RobotInputs {
        DevBuf<float> radius;    // [robot id] (float)Robot::radius
        size_t n_sized = 0;      // robots whose radii are up
        DevBuf<float> pos;       // positions the caller of the last _update handed in
        DevBuf<uint8_t> flags;   // ... and who was looked at then: not removed, not a ghost, and moved where the caller said who did
        uint32_t n_ghosts = 0;   // ghosts among the robots (mgx_robot_add, _import, _release): collisions_sharded
        DevBuf<uint32_t> group;  // [robot id] the robots' groups — of a grouped world only (observers_groups), what the robot-robot pass compares
        size_t group_sized = 0;  // robots whose groups are up
    } obs;
    // collision bookkeeping on the device (mgx_world_collisions.inc, mgx_collisions.hip): what its two kinds share
    struct ContactBook {
        bool enabled = false;
        size_t n_sized = 0;      // robots the per-robot arrays were last sized for
        DevBuf<ContactEvent> log;
        DevBuf<unsigned long long> words;
        DevBuf<uint32_t> per_robot;  // contacts, by robot id
        uint64_t log_cap = 0, pass = 0;
        std::vector<ContactEvent> host_log;  // the events fetched so far, in (pass, a, b) order
    };
    // robot-robot (mgx_collisions_*): the pair bits (whose stride grows with the robots), the pair lists, the hash grid's links
    struct Collisions : ContactBook {
        uint32_t method = 0;
        uint32_t stride = 0;     // of the pair bits
        DevBuf<uint32_t> bits, cnt;
        DevBuf<int2> list[2];
        DevBuf<unsigned long long> head;
        DevBuf<int32_t> next;
        uint32_t n_buckets = 0;
        CollDev d{};
    } coll;
    // robot-environment (mgx_env_collisions_*): the map's side, uploaded once by _enable, and the colliders every robot touches
    // the map as the device reads it: the collider table, the polygons' vertices and the per-tile grid (env_map_upload,
    // mgx_world_collisions.inc).  The robot-environment pass and the global planner each hold one
    struct EnvMap {
        DevBuf<EnvCollider> colliders;
        DevBuf<float> verts;
        DevBuf<uint32_t> cell_ptr;
        DevBuf<int32_t> cell_idx;
        EnvMapDev d{};
        void release() { colliders.release(); verts.release(); cell_ptr.release(); cell_idx.release(); d = EnvMapDev{}; }
    };
    struct EnvCollisions : ContactBook {
        EnvMap map;
        DevBuf<int32_t> touching;
        EnvCollDev d{};
    } envcoll;
    // trackers on the device (mgx_tracks_*, mgx_world_tracks.inc, mgx_tracks.hip): per-robot state keyed by robot id (robots that
    // join only make the array grow, zeroed), the sample log and the world's clock
    struct Tracks {
        bool enabled = false;
        size_t n_sized = 0;      // robots the state array (and the metrics' arrays, while they are on) has been sized for
        DevBuf<TrackState> state;
        DevBuf<TrackSample> log;
        DevBuf<unsigned long long> cursor;
        uint64_t log_cap = 0, period_ns = 0, tick_ns = 0;
        uint64_t clock = 0;      // the simulated tick index of the coming tick
        uint64_t dropped = 0;    // samples that found the log full, up to the last time it was emptied
        bool logging = true;     // mgx_tracks_set_logging
        // the run metrics (mgx_track_metrics_*): state per robot id beside `state`, under the same rules; every robot's route has
        // max_route_points places of the flat table, at robot * max_route_points
        bool metrics = false;
        uint32_t max_route_points = 0;
        DevBuf<TrackMetricsState> mstate;
        DevBuf<double> route_xy;
        DevBuf<TrackRoute> routes;
        DevBuf<TrackMetricsOut> mout;    // what mgx_track_metrics_read finalises into
    } tracks;
    // goal areas on the device (mgx_goal_areas_*, mgx_world_goal_areas.inc, mgx_goal_areas.hip): the table of first arrivals keyed
    // by (area, robot id), its rows with room for `stride` robots (observers_room: an append does not move it), and a clock of its own
    struct GoalAreas {
        bool enabled = false;
        uint32_t n_areas = 0;
        uint32_t stride = 0;     // robots a row of `first` has room for
        size_t n_sized = 0;      // robots the table was last sized for
        uint64_t clock = 0;      // the simulated tick index of the coming tick
        DevBuf<GoalAreaRec> recs;
        DevBuf<uint32_t> first;  // [n_areas][stride] tick + 1, 0: never
    } goals;
    // the global planner (mgx_planner_enable, mgx_world_planner.inc): the map and two pools of requests.  `pool`: the requests that
    // ride the stream (mgx_plan_submit / _advance / _collect), 256 blocks of 16 slots.  `call`: the requests of one mgx_plan_paths,
    // which gives its slots up before it returns — one block, sized by the largest call so far; the arrays of given-up slots are
    // the trees of the last call (mgx_plan_tree) until the next call takes them
    struct Planner {
        bool enabled = false;
        mgx_plan_params params{};  // defaults filled in
        EnvMap map;
        uint32_t tick_budget = 0;  // mgx_planner_set_tick_budget (a setting of the world: mgx_planner_enable keeps it)
        // the groups' parameter sets (mgx_planner_set_group_params): a group that has ever had one keeps its row of the device
        // table; set_of[group] is the index its requests carry (row + 1), 0 while it runs under the world's parameters
        struct Sets {
            std::vector<uint32_t> set_of;           // [MGX_GROUPS_MAX] once a set exists; empty: no group has one
            std::vector<uint32_t> row_of;           // [MGX_GROUPS_MAX] the group's row + 1, kept when its set is taken back
            std::vector<mgx_plan_params> params;    // per row, defaults filled in
            PlanSetDev *dev = nullptr;              // device memory, [dev_cap] rows
            size_t dev_cap = 0;
            Sets() = default;
            Sets(const Sets &) = delete;
            Sets &operator=(const Sets &) = delete;
            ~Sets() { release(); }
            void release() {  // (the caller has synchronised the stream)
                if (dev) (void)hipFree(dev);
                dev = nullptr; dev_cap = 0;
                set_of.clear(); row_of.clear(); params.clear();
            }
            uint32_t of(uint32_t group) const { return group < set_of.size() ? set_of[group] : 0u; }
        } sets;
        // a pool: bookkeeping in `book` (mgx_plan_pool.h), the slots' arrays a block at a time — trees and node paths in device
        // memory, states and points host-mapped — so that nothing a pending request uses ever moves; the table of blocks, the
        // completion log and the launches' active lists are host-mapped
        struct Pool {
            PlanPoolBook book;
            struct Block { void *dev = nullptr; PlanState *state = nullptr; float *out = nullptr; };  // state, out: one host allocation
            std::vector<Block> blocks;
            PlanBlockDev *table = nullptr;   // [book.max_blocks]
            uint32_t log_cap = 0;            // a power of two, at least 2 * book.max_slots() (more than can be unread)
            PlanLogEntry *log = nullptr;     // [log_cap]
            unsigned int *log_count = nullptr;  // device memory: entries claimed so far (the host never reads it)
            uint64_t log_taken = 0;
            struct List { PlanActive *p = nullptr; size_t cap = 0; uint64_t last_seq = 0; };  // last_seq: the last advance that reads it
            std::vector<List> lists;
            int cur = -1;                    // the list the running slots were last written to
            uint32_t cur_n = 0;
            bool cur_sets = false;           // a slot of that list names a parameter set: its launches take the table of sets
            std::vector<uint32_t> slot_group, slot_set;  // per slot: the group its request was submitted under (mgx_plan_done::group),
                                                         // and the parameter set it names (PlanState::set)
            hipEvent_t ev = nullptr;         // behind the last slice
            uint64_t ev_seq = 0;
            Pool(uint32_t slots_per_block, uint32_t max_blocks) : book(slots_per_block, max_blocks) {}
            Pool(const Pool &) = delete;
            Pool &operator=(const Pool &) = delete;
            ~Pool() { release(); }
            void release() {  // (the caller has synchronised the stream)
                for (Block &b : blocks) { if (b.dev) (void)hipFree(b.dev); if (b.state) (void)hipHostFree(b.state); }
                blocks.clear();
                for (List &l : lists) if (l.p) (void)hipHostFree(l.p);
                lists.clear();
                if (table) (void)hipHostFree(table);
                if (log) (void)hipHostFree(log);
                if (log_count) (void)hipFree(log_count);
                if (ev) (void)hipEventDestroy(ev);
                table = nullptr; log = nullptr; log_count = nullptr; ev = nullptr;
                log_cap = 0; log_taken = 0; cur = -1; cur_n = 0; ev_seq = 0; cur_sets = false;
                slot_group.clear(); slot_set.clear();
                book.drop();
            }
        };
        Pool pool{16, 256}, call{1, 1};
        std::vector<uint32_t> call_slots;  // slot of request i of the last mgx_plan_paths (mgx_plan_tree reads by it)
    } planner;
    uint32_t last_sweep_launches = 0;  // sweep-kernel launches of the last mgx_iterate / mgx_tick call (mgx_last_launch_count)
    SweepRan last_sweep;               // the sweep instantiation it launched last (mgx_last_sweep) ...
    int32_t last_sweep_form = -1;      // ... and in which form (MGX_SWEEP_FORM_*; -1: none)
    // message counters are advanced lazily: launches and prior changes are only logged here
    struct CountEntry { uint8_t ext, in; int n_int, robot; uint64_t times; };  // robot: an id; -1: every robot; -2 - g: the robots of group g
    std::vector<CountEntry> clog;
    int n_keyless = 0;  // connections whose factors still lack inbox keys (IrConn::keys)
    std::vector<uint32_t> cp_pending;  // [robot * K + variable] change_prior calls not yet counted
    std::vector<uint32_t> cp_dirty;
    DevBuf<unsigned long long> dbg;  // diagnostic builds only
    // halo plan: local robots whose snapshots are sent / ghost robots that receive, in buffer order
    std::vector<int32_t> halo_send, halo_recv;
    DevBuf<int32_t> halo_send_dev, halo_recv_dev;
    bool halo_dirty = false;
    // direct halo exchange (peer-mapped stores): this rank's receive area and arrival counters are
    // fine-grained device memory that the producers write; `dst` / `peer_flags` are addresses inside
    // the consumers' areas
    struct DirectHalo {
        double *recv = nullptr;               // [2][recv_words]
        unsigned long long *flags = nullptr;  // [n_sources] arrival counters, then one error word
        size_t recv_words = 0;
        int n_sources = 0, n_peers = 0;
        bool connected = false;
        // a wiring that survives changes of the exchange lists (mgx_halo_direct_setup_slots): one record slot per ghost robot —
        // slot = the robot's place among this rank's ghosts
        size_t slot_cap = 0;
        // ... whose push destinations (dst[], one per entry of the send list, in the consumers' slot numbering) are only as good as
        // the lists and the robots' device order they were made for: any change of either (mgx_halo_plan*, a robot added, imported
        // or released) takes the aim away until mgx_halo_direct_connect_slots has run again — an exchange in between is refused,
        // not run against tables of another length
        bool aimed = false;
        unsigned long long seq = 0, push_seq = 0;  // exchanges waited for / pushed
        long long timeout_ticks = 500000000ll;  // 5 s of the 100 MHz wall clock
        DevBuf<unsigned long long> dst[2], peer_flags, ready;  // ready: the exchange workgroup 0 of the wait kernel has announced
        DevBuf<unsigned int> done;
    } direct;
    // resident schedule launches of a sharded world (mgx_halo_resident_*): this rank's ghost area (fine-grained; the ghosts'
    // owner ranks store into it from inside their launches) and where the records of this rank's boundary robots go
    struct ResidentHalo {
        void *area = nullptr;
        size_t bytes = 0;
        int n_ghosts = 0;
        bool connected = false;
        bool wired = false;  // connect has run and disconnect has not: the peers may hold `area` mapped and store into it
        // a wiring that outlives the exchange lists (mgx_halo_resident_connect_peers / _aim): what translates this rank's parity and
        // segment count into each peer's, settled once when the ranks connect
        struct Peer { unsigned long long base = 0; size_t n_slots = 0; unsigned x = 0; unsigned long long flag_delta = 0; };
        std::vector<Peer> peers;
        DevBuf<int32_t> xp_ptr;
        DevBuf<XPushRec> xp_rec;
        // the ranks' agreement on every schedule's launches (SegPlan::agree_seq): the word (in rank 0's area), the number of
        // ranks that sign in on it, and the number of the last schedule this rank took there — the same on every rank
        unsigned long long *agree = nullptr;
        int n_ranks = 0;
        unsigned long long agree_seq = 0;
    } xres;
    // halo exchange through RCCL inside the library (grouped ncclSend / ncclRecv on the world's stream)
    struct RcclHalo {
        void *comm = nullptr;
        bool connected = false;
        std::vector<int> peer_rank;
        std::vector<uint32_t> send_first, recv_first;  // [n_peers + 1] into halo_send / halo_recv
        DevBuf<double> send_buf, recv_buf;
    } rccl;
    NeighbourSearch search;  // the comms-range neighbour search: its buffers, what it keeps between passes, what the last one did
};

static size_t edge_index(const std::vector<int32_t> &in_ptr, int K, int r, int j, int slot);
// slot of connection ci in the tables ON THE DEVICE (-1: not there — created since they were laid out, or its target is another rank's)
static inline int32_t dev_slot_of(const mgx_world *w, size_t ci) {
    const mgx_world::ConnHot &h = w->conn_hot[ci];
    return h.dev_q < 0 ? -1 : w->dev_in_ptr[(size_t)w->dev_of[(size_t)h.other]] + h.dev_q;
}
static void flush_counts(mgx_world *w, bool lazy = false);
static void conn_index_ensure(mgx_world *w);

// mgx_batch_begin .. mgx_batch_end (below, in front of mgx_iterate): every other call on the world first submits the schedules
// recorded so far, so that it finds the world as if each one had run when it was issued
static int iterate_now(mgx_world *w, const uint8_t *steps, uint32_t n);
static int submit_batch(mgx_world *w);
static int linger_close(mgx_world *w);
// the verdict of the resident launch not yet decided, if there is one (mgx_world_launch.inc): whoever enqueues work behind it or
// reads what it wrote comes through here first
static int confirm_resident(mgx_world *w, bool rerun = true, int32_t *outcome = nullptr);
#define MGX_CONFIRM(w)                                                  \
    do {                                                                \
        const int rc_confirm_ = confirm_resident(w);                    \
        if (rc_confirm_ != MGX_OK) return rc_confirm_;                  \
    } while (0)
// MGX_ENTER_SCHEDULE: mgx_tick (mgx_iterate has the batch's own logic) and the pure queries — recorded schedules are submitted,
// a lingering launch stays open.  MGX_ENTER: everything else — it also ends a lingering launch (what the call does would sit
// behind it in the stream, or read what it has not written back) and breaks the streak of back-to-back schedules.
#define MGX_ENTER_SCHEDULE(w)                                           \
    do {                                                                \
        if ((w) && !(w)->batch.steps.empty()) {                         \
            const int rc_enter_ = submit_batch(w);                      \
            if (rc_enter_ != MGX_OK) return rc_enter_;                  \
        }                                                               \
    } while (0)
#define MGX_ENTER(w)                                                    \
    do {                                                                \
        MGX_ENTER_SCHEDULE(w);                                          \
        if (w) {                                                        \
            (w)->res.other_call();                                      \
            if ((w)->res.linger.open) {                                 \
                const int rc_enter_ = linger_close(w);                  \
                if (rc_enter_ != MGX_OK) return rc_enter_;              \
            }                                                           \
        }                                                               \
    } while (0)

static bool device_ok() {
    static int state = 0;  // 0 unknown, 1 ok, -1 none
    if (state == 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        state = (e == hipSuccess && n > 0) ? 1 : -1;
    }
    return state == 1;
}
