// mgx_collisions.hip — robot-robot collision bookkeeping on the device (update_robot_robot_collisions,
// crates/magics/src/planner/collisions.rs:72-140, with the Free / Colliding state machine of CollisionHistory, :455-495;
// restated on the host by magics_amd/sim.py:_collide, which is the checker of this file).
//
// One PASS looks at the robots alive at that moment and their Transforms (x, z) as f32, radius r = (float)desc.radius:
//   * pair (a, b), a < b by robot id, OVERLAPS iff dx*dx + dy*dy <= (r_a + r_b)*(r_a + r_b) with d = p_b - p_a, every
//     operation rounded to f32 on its own (parry2d BoundingSphere::intersects).  Spelled with round-to-nearest intrinsics so
//     that no contraction setting fuses anything: libmgx.so and libmgx_fma.so agree.  A NaN anywhere makes the comparison
//     false: such a robot overlaps nobody.
//   * a pair that overlaps now and did not in the pass before (or was not looked at then) is one collision EVENT
//     {pass, a, b, mins, maxs}: the intersection of the two balls' AABBs, mins = max(p - r), maxs = min(p + r) per axis; it
//     counts once for robot a and once for robot b.
//   * a pair that parts, or loses a robot, is Free again.
// Robot-environment collisions are NOT here (exported as 0 / []): they need parry2d's shape queries against the map
// generator's colliders (environment/map_generator.rs:141-514: quaternion-rotated triangles, convex hulls), and there is no
// source of those queries to be bit-identical to.  The position / velocity tracker samples stay on the host as well.
//
// STATE (all keyed by robot ID, so nothing moves when the world lays its arrays out again; CollDev, mgx_dev.h):
//   bits   one bit per ordered pair (a * stride + b): the pair overlapped after the last pass
//   list   the same set as a list of pairs, two buffers: pass p reads list[p & 1] and writes list[(p + 1) & 1]
//   cnt    three length words in rotation: pass p reads cnt[p % 3], appends under cnt[(p + 1) % 3], zeroes cnt[(p + 2) % 3]
//          (the one the NEXT pass appends under: nobody else touches it in this pass, so no clearing launch is needed)
// A pass is work proportional to the overlaps plus the search: RETEST lanes walk the old list — a pair that still overlaps is
// copied to the new list, one that parted (or lost a robot) has its bit cleared; SEARCH lanes find every overlapping pair and
// set its bit with an atomic OR: where the bit was clear the pair is new — appended to the new list, logged as an event,
// counted for both robots.  The two never touch the same pair in conflicting ways (the retest only clears bits of pairs that
// do not overlap, the search only sets bits of pairs that do), so both run in ONE launch.
//   log    append-only, 32-byte records under an atomic cursor that keeps counting when the log is full (what did not fit is
//          cursor - capacity: nothing is lost silently, nothing traps or spins)
//   words  [0] the cursor, [1] sticky: the pair list overflowed (a pair's bit is set but nobody will ever clear it: later
//          passes may miss events — mgx_collisions_read reports it as an error)
//
// SEARCH, two forms with the identical event set by construction:
//   all pairs   64 robots x a chunk of 256 candidates per workgroup, candidates staged through LDS; chunks below the diagonal
//               are skipped (a < b)
//   hash grid   cells of 2 * r_max * 1.001 over x and z (r_max over the alive robots: the host knows it), so that the 3 x 3
//               cells around a robot hold every robot it can overlap; cells hash into buckets, a bucket is a linked list
//               (head per bucket, next per robot) built by one launch in front of the search; heads carry the pass number,
//               so a stale head is an empty bucket and nothing is cleared between passes.  A candidate counts only if its
//               TRUE cell is the one being looked at (two of the nine cells may share a bucket: no pair is seen twice).
//               Robots that are not alive or have a non-finite coordinate are in no cell: they overlap nobody under the
//               predicate above.  (A non-finite or non-positive r_max takes the all-pairs form: the host decides.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mgx.h"
#include "gbp_math.h"
#include "mgx_dev.h"

namespace mgx {

static_assert(sizeof(mgx_collision_event) == 32 && sizeof(CollEvent) == 32, "the log's records are 32 bytes");
static_assert(offsetof(mgx_collision_event, robot_a) == offsetof(CollEvent, robot_a) && offsetof(mgx_collision_event, mins) == offsetof(CollEvent, mins) &&
                  offsetof(mgx_collision_event, maxs) == offsetof(CollEvent, maxs),
              "CollEvent is the ABI's record");

__device__ __forceinline__ bool balls_overlap(float ax, float az, float ar, float bx, float bz, float br) {
    const float dx = __fsub_rn(bx, ax), dy = __fsub_rn(bz, az), rs = __fadd_rn(ar, br);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) <= __fmul_rn(rs, rs);
}

// (x, z, r) of robot i as a pass sees it: a robot that is not alive is nowhere (NaN overlaps nobody)
__device__ __forceinline__ void robot_ball(const CollDev &c, int i, float &x, float &z, float &r) {
    const bool alive = c.alive[i] != 0;
    x = alive ? c.pos[3 * i] : NAN;
    z = alive ? c.pos[3 * i + 2] : NAN;
    r = c.radius[i];
}

__device__ __forceinline__ void list_append(const CollDev &c, int a, int b) {
    const uint32_t at = atomicAdd(&c.cnt[(c.pass + 1) % 3], 1u);
    if (at < c.list_cap) c.list[(c.pass + 1) & 1][at] = make_int2(a, b);
    else atomicOr(&c.words[1], 1ull);
}

// pair (a, b), a < b, overlaps in this pass
__device__ __forceinline__ void pair_overlaps(const CollDev &c, int a, float ax, float az, float ar, int b, float bx, float bz, float br) {
    const uint64_t bit = (uint64_t)a * c.stride + (uint64_t)b;
    const uint32_t m = 1u << (bit & 31u);
    if (atomicOr(&c.bits[bit >> 5], m) & m) return;  // Colliding -> Colliding (the retest lanes carry it over)
    list_append(c, a, b);
    const unsigned long long e = atomicAdd(&c.words[0], 1ull);
    if (e < c.log_cap) {
        CollEvent ev;
        ev.pass = c.pass;
        ev.robot_a = a;
        ev.robot_b = b;
        ev.mins[0] = fmaxf(__fsub_rn(ax, ar), __fsub_rn(bx, br));
        ev.mins[1] = fmaxf(__fsub_rn(az, ar), __fsub_rn(bz, br));
        ev.maxs[0] = fminf(__fadd_rn(ax, ar), __fadd_rn(bx, br));
        ev.maxs[1] = fminf(__fadd_rn(az, ar), __fadd_rn(bz, br));
        c.log[e] = ev;
    }
    atomicAdd(&c.per_robot[a], 1u);
    atomicAdd(&c.per_robot[b], 1u);
}

// the pairs that overlapped after the pass before: still together -> the new list; parted / a robot gone -> Free
__device__ void retest(const CollDev &c, int lane, int n_lanes) {
    const uint32_t n_old = min(c.cnt[c.pass % 3], c.list_cap);
    for (uint32_t t = (uint32_t)lane; t < n_old; t += (uint32_t)n_lanes) {
        const int2 p = c.list[c.pass & 1][t];
        bool keep = p.x >= 0 && p.y > p.x && p.y < c.n;
        if (keep) {
            float ax, az, ar, bx, bz, br;
            robot_ball(c, p.x, ax, az, ar);
            robot_ball(c, p.y, bx, bz, br);
            keep = balls_overlap(ax, az, ar, bx, bz, br);
        }
        if (keep) list_append(c, p.x, p.y);
        else if (p.x >= 0 && p.y >= 0 && (uint32_t)p.x < c.stride && (uint32_t)p.y < c.stride) {
            const uint64_t bit = (uint64_t)p.x * c.stride + (uint64_t)p.y;
            atomicAnd(&c.bits[bit >> 5], ~(1u << (bit & 31u)));
        }
    }
}

constexpr int COLL_BLOCK = 64, COLL_CHUNK = 256, COLL_RETEST_BLOCKS = 8;

// workgroups [0, n_search): robots [64 bi, 64 bi + 64) against candidates [256 bj, 256 bj + 256); the last COLL_RETEST_BLOCKS: retest
__global__ void __launch_bounds__(COLL_BLOCK) k_collisions_pairs(CollDev c, int n_i, int n_search) {
    __shared__ float X[COLL_CHUNK], Z[COLL_CHUNK], Rr[COLL_CHUNK];
    const int blk = (int)blockIdx.x;
    if (blk >= n_search) {
        if (blk == n_search && threadIdx.x == 0) c.cnt[(c.pass + 2) % 3] = 0u;
        retest(c, (blk - n_search) * COLL_BLOCK + (int)threadIdx.x, COLL_RETEST_BLOCKS * COLL_BLOCK);
        return;
    }
    const int bi = blk % n_i, bj = blk / n_i;
    const int i0 = bi * COLL_BLOCK, j0 = bj * COLL_CHUNK;
    if (j0 + COLL_CHUNK <= i0 + 1) return;  // every candidate of the chunk has an id <= every robot's of the workgroup
    for (int q = (int)threadIdx.x; q < COLL_CHUNK; q += COLL_BLOCK) {
        float x = NAN, z = NAN, r = 0.f;
        if (j0 + q < c.n) robot_ball(c, j0 + q, x, z, r);
        X[q] = x; Z[q] = z; Rr[q] = r;
    }
    __syncthreads();
    const int i = i0 + (int)threadIdx.x;
    if (i >= c.n) return;
    float ax, az, ar;
    robot_ball(c, i, ax, az, ar);
    if (ax != ax || az != az) return;
    for (int q = max(0, i + 1 - j0); q < COLL_CHUNK; q++)
        if (balls_overlap(ax, az, ar, X[q], Z[q], Rr[q])) pair_overlaps(c, i, ax, az, ar, j0 + q, X[q], Z[q], Rr[q]);
}

__device__ __forceinline__ int coll_cell_of(float x, double inv_cell) {  // monotone, clamped (as mgx_topology.hip's)
    double v = floor((double)x * inv_cell);
    v = fmin(fmax(v, -1073741824.0), 1073741824.0);
    return (int)v;
}
__device__ __forceinline__ uint32_t coll_bucket_of(int cx, int cz, uint32_t mask) {
    return (((uint32_t)cx * 73856093u) ^ ((uint32_t)cz * 19349663u)) & mask;
}

// every alive robot with finite coordinates goes to the front of its bucket's list; a head of another pass is an empty bucket
__global__ void __launch_bounds__(256) k_collisions_link(CollDev c, double inv_cell, uint32_t mask) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= c.n) return;
    float x, z, r;
    robot_ball(c, i, x, z, r);
    if (!isfinite(x) || !isfinite(z)) return;
    const unsigned long long stamp = (unsigned long long)(uint32_t)(c.pass + 1u) << 32;
    const unsigned long long old = atomicExch(&c.head[coll_bucket_of(coll_cell_of(x, inv_cell), coll_cell_of(z, inv_cell), mask)], stamp | (uint32_t)i);
    c.next[i] = (old >> 32) == (stamp >> 32) ? (int32_t)(uint32_t)old : -1;
}

__global__ void __launch_bounds__(COLL_BLOCK) k_collisions_grid(CollDev c, double inv_cell, uint32_t mask, int n_search) {
    const int blk = (int)blockIdx.x;
    if (blk >= n_search) {
        if (blk == n_search && threadIdx.x == 0) c.cnt[(c.pass + 2) % 3] = 0u;
        retest(c, (blk - n_search) * COLL_BLOCK + (int)threadIdx.x, COLL_RETEST_BLOCKS * COLL_BLOCK);
        return;
    }
    const int i = blk * COLL_BLOCK + (int)threadIdx.x;
    if (i >= c.n) return;
    float ax, az, ar;
    robot_ball(c, i, ax, az, ar);
    if (!isfinite(ax) || !isfinite(az)) return;
    const int cx = coll_cell_of(ax, inv_cell), cz = coll_cell_of(az, inv_cell);
    const uint32_t stamp = (uint32_t)(c.pass + 1u);
    for (int ox = -1; ox <= 1; ox++)
        for (int oz = -1; oz <= 1; oz++) {
            const int qx = cx + ox, qz = cz + oz;
            const unsigned long long h = c.head[coll_bucket_of(qx, qz, mask)];
            int j = (uint32_t)(h >> 32) == stamp ? (int)(uint32_t)h : -1;
            for (int guard = 0; j >= 0 && j < c.n && guard < c.n; guard++) {
                if (j > i) {
                    float bx, bz, br;
                    robot_ball(c, j, bx, bz, br);
                    if (coll_cell_of(bx, inv_cell) == qx && coll_cell_of(bz, inv_cell) == qz && balls_overlap(ax, az, ar, bx, bz, br))
                        pair_overlaps(c, i, ax, az, ar, j, bx, bz, br);
                }
                j = c.next[j];
            }
        }
}

// a new stride of the pair bits (robots joined): the bits of the listed pairs, from the list the next pass reads
__global__ void __launch_bounds__(256) k_collisions_rebits(CollDev c) {
    const uint32_t n_old = min(c.cnt[c.pass % 3], c.list_cap);
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < n_old; t += gridDim.x * 256) {
        const int2 p = c.list[c.pass & 1][t];
        if (p.x < 0 || p.y < 0 || (uint32_t)p.x >= c.stride || (uint32_t)p.y >= c.stride) continue;
        const uint64_t bit = (uint64_t)p.x * c.stride + (uint64_t)p.y;
        atomicOr(&c.bits[bit >> 5], 1u << (bit & 31u));
    }
}

hipError_t launch_collisions_pass(const CollDev &c, bool grid, double cell, uint32_t n_buckets, hipStream_t s) {
    if (c.n <= 0) return hipSuccess;
    if (grid) {
        const double inv_cell = 1.0 / cell;
        const int n_search = (c.n + COLL_BLOCK - 1) / COLL_BLOCK;
        hipLaunchKernelGGL(k_collisions_link, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, s, c, inv_cell, n_buckets - 1u);
        hipLaunchKernelGGL(k_collisions_grid, dim3((unsigned)(n_search + COLL_RETEST_BLOCKS)), dim3(COLL_BLOCK), 0, s, c, inv_cell, n_buckets - 1u,
                           n_search);
    } else {
        const int n_i = (c.n + COLL_BLOCK - 1) / COLL_BLOCK, n_j = (c.n + COLL_CHUNK - 1) / COLL_CHUNK;
        hipLaunchKernelGGL(k_collisions_pairs, dim3((unsigned)(n_i * n_j + COLL_RETEST_BLOCKS)), dim3(COLL_BLOCK), 0, s, c, n_i, n_i * n_j);
    }
    return hipGetLastError();
}
hipError_t launch_collisions_rebits(const CollDev &c, hipStream_t s) {
    hipLaunchKernelGGL(k_collisions_rebits, dim3(16), dim3(256), 0, s, c);
    return hipGetLastError();
}

}  // namespace mgx
