// mgx_planner.hip — the global planner on the device: batched RRT* over the map's colliders (what crates/gbp_global_planner does
// per robot, rrtstar.rs:15-83, started from progress_missions, robot.rs:578-633).  include/mgx.h ("global planner") holds the
// specification; magics_amd/global_planner.py restates it on the host and is the checker of this file.
//
// ONE WORKGROUP PER REQUEST, 256 lanes, many requests per launch.  The tree is SoA: the positions (two f64 arrays of max_nodes)
// live in LDS for the length of a launch — every iteration reads all of them twice (nearest node, neighbourhood) — and are
// written through to global memory as nodes are appended; parents and costs stay in global memory (L2-resident: a request's
// whole tree is at most 224 KiB), because the neighbourhood pass reads only the costs of the few nodes inside the radius.
// A node k is always read and rewired by lane k % 256, so the only cross-lane traffic through global memory is the appended
// node (lane 0 writes, a workgroup barrier follows).
// Every strided loop ends in a reduction of the pair (key, index) to its lexicographic minimum — order-independent, so the
// result is the serial restatement's bit for bit: in-lane strict '<' over ascending indices, xor-shuffles across the wave,
// four partial results through LDS.
// feasible(p) spreads the colliders of the cells the ball overlaps over the lanes and combines with a workgroup OR; a smoothing
// chord spreads its POINTS over the lanes (each lane walks its points' cells alone) and combines the same way.
// A launch runs at most `budget` iterations per request (growth and smoothing iterations count alike) and leaves everything in
// global memory — tree, counters, stream state, phase — so the host launches again until every request is done, and where the
// slices fall does not show in the result.  One kernel runs the slice (plan_slice): k_plan_pool, over the active slots of a pool
// of requests — the pool whose requests ride the world's stream (mgx_plan_submit / _advance / _collect), or the pool that
// mgx_plan_paths fills, drives to the end and empties within one call.  A request may run under its robot group's own parameter set
// (mgx_planner_set_group_params): a row of one device table, read once per launch; k_plan_pool<true> is the launch that carries
// the table, k_plan_pool<false> the launch none of whose requests names a set.
// All planner arithmetic is f64 with every operation rounded on its own: contraction is switched off for this file whatever
// the command line says, so libmgx.so and libmgx_fma.so hold the same code here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "../../include/mgx.h"
#include "mgx_dev.h"
#include "mgx_env_contact.h"
#include "mgx_grid.h"

namespace mgx {

constexpr int PLAN_BLOCK = 256, PLAN_WAVES = PLAN_BLOCK / 64;

// -- the random stream: wyrand, advanced exactly as magics_amd/prng.py:WyRand ------------------------------------------------------
__device__ __forceinline__ unsigned long long wy_next(unsigned long long &s) {
    s += 0xA0761D6478BD642Full;
    const unsigned long long b = s ^ 0xE7037ED1A0B428DBull;
    return __umul64hi(s, b) ^ (s * b);
}
__device__ __forceinline__ double wy_uniform(unsigned long long &s, double h) {
    const unsigned long long u = wy_next(s);
    const double v = __longlong_as_double((long long)((u >> 12) | 0x3FF0000000000000ull)) - 1.0;
    return v * (2.0 * h) + (-h);
}
// rand 0.8.5 UniformInt::<u32>::sample_single(0, ubound)
__device__ __forceinline__ uint32_t wy_index(unsigned long long &s, uint32_t range) {
    if (range == 0) return (uint32_t)wy_next(s);
    const uint32_t zone = (range << __clz((int)range)) - 1u;
    for (;;) {
        const unsigned long long m = (unsigned long long)(uint32_t)wy_next(s) * range;
        if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
    }
}

// -- (key, index) -> its lexicographic minimum over the workgroup, in every lane -----------------------------------------------------
struct PlanScratch {
    double key[PLAN_WAVES];
    int idx[PLAN_WAVES];
};
__device__ __forceinline__ bool lex_less(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }
__device__ __forceinline__ void block_min(double &key, int &idx, PlanScratch &sc) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ok = __shfl_xor(key, off);
        const int oi = __shfl_xor(idx, off);
        if (lex_less(ok, oi, key, idx)) { key = ok; idx = oi; }
    }
    const int tid = (int)threadIdx.x;
    if ((tid & 63) == 0) { sc.key[tid >> 6] = key; sc.idx[tid >> 6] = idx; }
    __syncthreads();
    key = sc.key[0]; idx = sc.idx[0];
#pragma unroll
    for (int w = 1; w < PLAN_WAVES; w++)
        if (lex_less(sc.key[w], sc.idx[w], key, idx)) { key = sc.key[w]; idx = sc.idx[w]; }
    __syncthreads();  // (the scratch is free again)
}

// a collider touches the ball of radius r at ((float)px, (float)py): the colliders of the cells it overlaps, `lane` of `lanes`
__device__ __forceinline__ bool ball_hits(const EnvMapDev &m, double px, double py, float r, int lane, int lanes) {
    const float x = (float)px, z = (float)py;
    if (m.n_colliders <= 0 || !isfinite(x) || !isfinite(z)) return false;
    const EnvCellRange c = env_cells_of_ball(m, x, z, r);
    bool hit = false;
    for (int cz = c.z0; cz <= c.z1; cz++)
        for (int cx = c.x0; cx <= c.x1; cx++) {
            const uint32_t cell = (uint32_t)cz * (uint32_t)m.n_cx + (uint32_t)cx;
            for (uint32_t q = m.cell_ptr[cell] + (uint32_t)lane, q1 = m.cell_ptr[cell + 1]; q < q1; q += (uint32_t)lanes)
                hit = hit || env_touches(m.colliders[m.cell_idx[q]], m.verts, x, z, r);
        }
    return hit;
}

__device__ __forceinline__ double dist2(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}

// One request's arrays: a slot of a pool (k_plan_pool).
struct PlanSlot {
    PlanState *state;
    double *x, *y, *cost;  // [max_nodes]
    int32_t *parent;       // [max_nodes]
    int32_t *path;         // [max_nodes + 1]
    float *out;            // [max_nodes + 1][2]
};

// One slice of one request by one workgroup.  True (in every lane) when the request ENDED in this slice.
// `sets`: the groups' parameter sets (mgx_planner_set_group_params), NULL when no request of the launch names one.  A request
// that names one (PlanState::set) reads its row once and runs under a copy of the launch's constants with the row's fields in
// place: every value is the same in all lanes, as the launch's own are.
__device__ __forceinline__ bool plan_slice(const PlanDev &launch, const PlanSetDev *__restrict__ sets, const PlanSlot &slot) {
    extern __shared__ double plan_lds[];  // X [max_nodes], Y [max_nodes]
    __shared__ PlanScratch sc;
    __shared__ uint32_t s_len;
    const int tid = (int)threadIdx.x;
    PlanState st = *slot.state;  // (the same in every lane, and kept so)
    if (st.phase == PLAN_PHASE_DONE) return false;
    PlanDev c = launch;
    if (sets && st.set) {
        const PlanSetDev g = sets[st.set - 1u];
        c.step = g.step; c.radius2 = g.radius2; c.half_extent = g.half_extent; c.smoothing_step = g.smoothing_step;
        c.collision_radius = g.collision_radius;
        c.max_iterations = g.max_iterations; c.smoothing_max = g.smoothing_max; c.smoothing = g.smoothing;
    }
    const uint32_t cap = c.max_nodes;
    double *const X = plan_lds, *const Y = plan_lds + cap;
    double *const gx = slot.x, *const gy = slot.y, *const gcost = slot.cost;
    int32_t *const gparent = slot.parent, *const gpath = slot.path;
    const double ex = (double)st.end[0], ey = (double)st.end[1];
    if (st.phase == PLAN_PHASE_INIT) {
        if (tid == 0) {
            gx[0] = (double)st.start[0]; gy[0] = (double)st.start[1];
            gcost[0] = 0.0; gparent[0] = -1;
        }
        st.n_nodes = 1; st.iterations = 0; st.path_len = 0; st.smooth_done = 0; st.goal = -1; st.cost = 0.0;
        st.phase = PLAN_PHASE_GROW;
        __syncthreads();
    }
    for (uint32_t k = (uint32_t)tid; k < st.n_nodes && k < cap; k += PLAN_BLOCK) { X[k] = gx[k]; Y[k] = gy[k]; }
    __syncthreads();
    uint32_t budget = c.budget;

    while (st.phase == PLAN_PHASE_GROW && budget > 0) {
        if (st.iterations >= c.max_iterations) { st.status = MGX_PLAN_MAX_ITERATIONS; st.phase = PLAN_PHASE_DONE; break; }
        st.iterations += 1;
        budget -= 1;
        const int n = (int)st.n_nodes;
        const double qx = wy_uniform(st.rng, c.half_extent);
        const double qy = wy_uniform(st.rng, c.half_extent);
        // 2. the nearest node
        double bk = INFINITY;
        int bi = 0x7fffffff;
        for (int k = tid; k < n; k += PLAN_BLOCK) {
            const double d2 = dist2(X[k], Y[k], qx, qy);
            if (d2 < bk) { bk = d2; bi = k; }
        }
        block_min(bk, bi, sc);
        const int ns = bi;
        if (ns < 0 || ns >= n) continue;  // (no finite distance: nothing to grow from)
        // 3. steer
        const double d = __dsqrt_rn(bk);
        if (d == 0.0) continue;
        double px = qx, py = qy;
        if (!(d <= c.step)) {
            const double t = c.step / d, nx = X[ns], ny = Y[ns];
            px = nx + t * (qx - nx);
            py = ny + t * (qy - ny);
        }
        // 4. feasible
        if (__syncthreads_or(ball_hits(c.map, px, py, c.collision_radius, tid, PLAN_BLOCK) ? 1 : 0)) continue;
        // 5. + 6. the neighbourhood and the parent in it
        bk = INFINITY;
        bi = 0x7fffffff;
        for (int k = tid; k < n; k += PLAN_BLOCK) {
            const double d2 = dist2(X[k], Y[k], px, py);
            if (d2 <= c.radius2 || k == ns) {
                const double cand = gcost[k] + __dsqrt_rn(d2);
                if (cand < bk) { bk = cand; bi = k; }
            }
        }
        block_min(bk, bi, sc);
        const int parent = bi;
        const double cost_new = bk;
        // 7. append
        if ((uint32_t)n >= cap) { st.status = MGX_PLAN_TREE_FULL; st.phase = PLAN_PHASE_DONE; break; }
        const int m = n;
        // 8. rewire (node k is this lane's alone)
        for (int k = tid; k < n; k += PLAN_BLOCK) {
            if (k == parent) continue;
            const double d2 = dist2(X[k], Y[k], px, py);
            if (d2 <= c.radius2) {
                const double cnew = cost_new + __dsqrt_rn(d2);
                if (cnew < gcost[k]) { gparent[k] = m; gcost[k] = cnew; }
            }
        }
        if (tid == 0) {
            X[m] = px; Y[m] = py;
            gx[m] = px; gy[m] = py; gcost[m] = cost_new; gparent[m] = parent;
        }
        st.n_nodes = (uint32_t)(m + 1);
        __syncthreads();
        // 9. the goal
        const double dg = __dsqrt_rn(dist2(px, py, ex, ey));
        if (dg <= c.step) {
            st.goal = m;
            st.cost = cost_new + dg;
            if (tid == 0) {  // the parent chain from m to node 0, reversed, then `end`
                uint32_t len = 0;
                int k = m;
                while (k >= 0 && (uint32_t)k < cap && len < st.n_nodes) { len++; k = gparent[k]; }
                gpath[len] = -1;
                k = m;
                for (uint32_t i = len; i-- > 0;) { gpath[i] = k; k = gparent[k]; }
                s_len = len + 1;
            }
            __syncthreads();
            st.path_len = s_len;
            st.phase = c.smoothing ? PLAN_PHASE_SMOOTH : PLAN_PHASE_FINISH;
        }
    }

    while (st.phase == PLAN_PHASE_SMOOTH) {
        if (st.path_len < 3 || st.smooth_done >= c.smoothing_max) { st.phase = PLAN_PHASE_FINISH; break; }
        if (budget == 0) break;
        budget -= 1;
        const uint32_t len = st.path_len;
        const uint32_t a = wy_index(st.rng, len - 2);
        const uint32_t b = a + 2 + wy_index(st.rng, len - 2 - a);
        const int ia = gpath[a], ib = gpath[b];
        const double ax = X[ia], ay = Y[ia];  // (a <= len - 3: never `end`)
        const double bx = ib < 0 ? ex : X[ib], by = ib < 0 ? ey : Y[ib];
        const double dx = bx - ax, dy = by - ay;
        const double L = __dsqrt_rn(dx * dx + dy * dy), h = c.smoothing_step;
        const double fcnt = floor(L / h);
        const long long cnt = fcnt < 9.0e15 ? (long long)fcnt : 9000000000000000ll;
        bool hit = false;
        for (long long j = 1 + tid; j <= cnt && !hit; j += PLAN_BLOCK) {
            const double f = ((double)j * h) / L;
            hit = ball_hits(c.map, ax + dx * f, ay + dy * f, c.collision_radius, 0, 1);
        }
        const bool blocked = __syncthreads_or(hit ? 1 : 0) != 0;
        if (!blocked) {  // P[a+1 .. b-1] go: what follows moves down, a block of lanes at a time (reads before writes)
            const uint32_t shift = b - a - 1;
            for (uint32_t base = b; base < len; base += PLAN_BLOCK) {
                const uint32_t i = base + (uint32_t)tid;
                const int v = i < len ? gpath[i] : 0;
                __syncthreads();
                if (i < len) gpath[i - shift] = v;
                __syncthreads();
            }
            st.path_len = len - shift;
        }
        st.smooth_done += 1;
    }

    if (st.phase == PLAN_PHASE_FINISH) {
        float *const out = slot.out;
        for (uint32_t i = (uint32_t)tid; i < st.path_len && i <= cap; i += PLAN_BLOCK) {
            const int k = gpath[i];
            out[2 * i] = (float)(k < 0 ? ex : X[k]);
            out[2 * i + 1] = (float)(k < 0 ? ey : Y[k]);
        }
        st.status = MGX_PLAN_OK;
        st.phase = PLAN_PHASE_DONE;
    }
    if (tid == 0) *slot.state = st;
    return st.phase == PLAN_PHASE_DONE;
}

// One slice of a pool (mgx_plan_advance, a mission tick's budget, mgx_plan_paths): workgroup = entry of the compact list of
// active slots; a slot's arrays are found through its block's base pointers (blocks never move while the pool lives).  State and
// points of a slot are in host-mapped memory, and so is the completion log: a request that ends here makes its state and points
// visible to the host, then claims the next log entry (the one atomic, on a counter in device memory: the host never reads it)
// and fills it with one 16-byte store.  The host takes an entry once its ticket is not 0 (tickets count from 1) and zeroes it
// again, so a counter that is ahead of an entry's store only delays that entry to the next look.
// SETS: the launch carries the table of parameter sets.  A launch without one runs the instantiation that knows nothing of sets.
template <bool SETS>
__global__ void __launch_bounds__(PLAN_BLOCK) k_plan_pool(PlanDev c, PlanPoolDev pool) {
    const PlanActive a = pool.active[blockIdx.x];
    const PlanBlockDev b = pool.blocks[a.slot / pool.slots_per_block];
    const size_t i = a.slot % pool.slots_per_block, cap = c.max_nodes;
    PlanSlot slot;
    slot.state = b.state + i;
    slot.x = b.x + i * cap; slot.y = b.y + i * cap; slot.cost = b.cost + i * cap;
    slot.parent = b.parent + i * cap;
    slot.path = b.path + i * (cap + 1);
    slot.out = b.out + 2 * i * (cap + 1);
    if (!plan_slice(c, SETS ? pool.sets : nullptr, slot)) return;
    __threadfence_system();  // every lane: its points; lane 0: the state
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the fence's own wait is not relied on)
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int at = atomicAdd_system(pool.log_count, 1u);
        PlanLogEntry e;
        e.ticket = a.ticket;
        e.slices = pool.seq - a.first_seq;
        e.slot = a.slot;
        pool.log[at % pool.log_cap] = e;
    }
}

template <bool SETS>
static hipError_t launch_plan_pool_as(const PlanDev &c, const PlanPoolDev &pool, int n_active, hipStream_t s) {
    static size_t granted = 0;
    const size_t lds = sizeof(double) * 2 * (size_t)c.max_nodes;
    if (lds > granted) {  // dynamic LDS beyond 64 KiB has to be asked for once per size
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_plan_pool<SETS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        granted = lds;
    }
    hipLaunchKernelGGL(k_plan_pool<SETS>, dim3((unsigned)n_active), dim3(PLAN_BLOCK), lds, s, c, pool);
    return hipGetLastError();
}

hipError_t launch_plan_pool(const PlanDev &c, const PlanPoolDev &pool, int n_active, hipStream_t s) {
    if (n_active <= 0) return hipSuccess;
    return pool.sets ? launch_plan_pool_as<true>(c, pool, n_active, s) : launch_plan_pool_as<false>(c, pool, n_active, s);
}

}  // namespace mgx
