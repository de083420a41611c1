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
// Robot-environment collisions are the second half of this file (k_env_collisions: its own state, log and calls).  The
// position / velocity tracker samples are a pass of their own beside these two (mgx_tracks.hip).
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
//          cursor - capacity: nothing is lost silently, nothing traps or spins): ContactLog and contact_append, shared with
//          the robot-environment pass
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
// GROUPS (include/mgx.h, ROBOT GROUPS): in a grouped world only robots of one group collide.  The all-pairs form stages the
// candidates' groups beside x, z and r and asks for equality in front of the predicate; the hash grid mixes the group into the
// bucket hash, so that equal cells of different groups do not share a list, and compares the group before the predicate as well
// (two groups' cells may still share a bucket).  Group 0 mixes to nothing: an ungrouped world (CollDev::group null) hashes as
// before.  The listed pairs are pairs of one group by construction, so the retest does not look.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mgx.h"
#include "gbp_math.h"
#include "mgx_dev.h"
#include "mgx_env_contact.h"
#include "mgx_grid.h"

namespace mgx {

static_assert(sizeof(mgx_collision_event) == 32 && sizeof(ContactEvent) == 32, "the log's records are 32 bytes");
static_assert(offsetof(mgx_collision_event, robot_a) == offsetof(ContactEvent, a) && offsetof(mgx_collision_event, robot_b) == offsetof(ContactEvent, b) &&
                  offsetof(mgx_collision_event, mins) == offsetof(ContactEvent, mins) && offsetof(mgx_collision_event, maxs) == offsetof(ContactEvent, maxs),
              "ContactEvent is the ABI's record");

// one record under the log's cursor, which keeps counting when the log is full (the overflow word is the callers' business)
__device__ __forceinline__ void contact_append(const ContactLog &log, unsigned long long pass, int a, int b, float min0, float min1, float max0, float max1) {
    const unsigned long long e = atomicAdd(&log.words[0], 1ull);
    if (e < log.cap) {
        ContactEvent ev;
        ev.pass = pass;
        ev.a = a;
        ev.b = b;
        ev.mins[0] = min0;
        ev.mins[1] = min1;
        ev.maxs[0] = max0;
        ev.maxs[1] = max1;
        log.events[e] = ev;
    }
}

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

__device__ __forceinline__ uint32_t robot_group(const CollDev &c, int i) { return c.group ? c.group[i] : 0u; }
// the bucket of a cell of one group's robots
__device__ __forceinline__ uint32_t group_bucket_of(int cx, int cz, uint32_t group, uint32_t mask) {
    return (bucket_of(cx, cz, mask) + group * 0x9E3779B1u) & mask;
}

__device__ __forceinline__ void list_append(const CollDev &c, int a, int b) {
    const uint32_t at = atomicAdd(&c.cnt[(c.pass + 1) % 3], 1u);
    if (at < c.list_cap) c.list[(c.pass + 1) & 1][at] = make_int2(a, b);
    else atomicOr(&c.log.words[1], 1ull);
}

// pair (a, b), a < b, overlaps in this pass
__device__ __forceinline__ void pair_overlaps(const CollDev &c, int a, float ax, float az, float ar, int b, float bx, float bz, float br) {
    const uint64_t bit = (uint64_t)a * c.stride + (uint64_t)b;
    const uint32_t m = 1u << (bit & 31u);
    if (atomicOr(&c.bits[bit >> 5], m) & m) return;  // Colliding -> Colliding (the retest lanes carry it over)
    list_append(c, a, b);
    contact_append(c.log, c.pass, a, b, fmaxf(__fsub_rn(ax, ar), __fsub_rn(bx, br)), fmaxf(__fsub_rn(az, ar), __fsub_rn(bz, br)),
                   fminf(__fadd_rn(ax, ar), __fadd_rn(bx, br)), fminf(__fadd_rn(az, ar), __fadd_rn(bz, br)));
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
    __shared__ uint32_t G[COLL_CHUNK];
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
        uint32_t g = 0u;
        if (j0 + q < c.n) {
            robot_ball(c, j0 + q, x, z, r);
            g = robot_group(c, j0 + q);
        }
        X[q] = x; Z[q] = z; Rr[q] = r; G[q] = g;
    }
    __syncthreads();
    const int i = i0 + (int)threadIdx.x;
    if (i >= c.n) return;
    float ax, az, ar;
    robot_ball(c, i, ax, az, ar);
    if (ax != ax || az != az) return;
    const uint32_t ag = robot_group(c, i);
    for (int q = max(0, i + 1 - j0); q < COLL_CHUNK; q++)
        if (G[q] == ag && balls_overlap(ax, az, ar, X[q], Z[q], Rr[q])) pair_overlaps(c, i, ax, az, ar, j0 + q, X[q], Z[q], Rr[q]);
}

// every alive robot with finite coordinates goes to the front of its bucket's list; a head of another pass is an empty bucket
__global__ void __launch_bounds__(256) k_collisions_link(CollDev c, double inv_cell, uint32_t mask) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= c.n) return;
    float x, z, r;
    robot_ball(c, i, x, z, r);
    if (!isfinite(x) || !isfinite(z)) return;
    const unsigned long long stamp = (unsigned long long)(uint32_t)(c.pass + 1u) << 32;
    const unsigned long long old = atomicExch(&c.head[group_bucket_of(cell_of(x, inv_cell), cell_of(z, inv_cell), robot_group(c, i), mask)], stamp | (uint32_t)i);
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
    const int cx = cell_of(ax, inv_cell), cz = cell_of(az, inv_cell);
    const uint32_t stamp = (uint32_t)(c.pass + 1u);
    const uint32_t ag = robot_group(c, i);
    for (int ox = -1; ox <= 1; ox++)
        for (int oz = -1; oz <= 1; oz++) {
            const int qx = cx + ox, qz = cz + oz;
            const unsigned long long h = c.head[group_bucket_of(qx, qz, ag, mask)];
            int j = (uint32_t)(h >> 32) == stamp ? (int)(uint32_t)h : -1;
            for (int guard = 0; j >= 0 && j < c.n && guard < c.n; guard++) {
                if (j > i && robot_group(c, j) == ag) {
                    float bx, bz, br;
                    robot_ball(c, j, bx, bz, br);
                    if (cell_of(bx, inv_cell) == qx && cell_of(bz, inv_cell) == qz && balls_overlap(ax, az, ar, bx, bz, br))
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

// ---- robot-environment collisions (update_robot_environment_collisions, collisions.rs:368-438) -----------------------------
// Every alive robot's ball against the map's colliders (mgx_env_colliders: tile cuboids, then the placeable obstacles), through
// the same Free / Colliding state machine.  include/mgx.h holds the specification of a contact; sim.py:_collide_environment
// restates it on the host and is the checker.  The map is static, so everything about it is built on the host once
// (mgx_env_collisions_enable): the collider records, the polygons' world vertices, and a uniform grid of one cell per tile with
// a CSR list of the colliders whose AABB overlaps each cell.
// One lane per robot: it walks the cells its (padded) AABB overlaps, however many; a collider listed in several of them is
// tested in the first cell the two ranges share and nowhere else.  STATE per robot: ENV_COLL_SLOTS collider ids, the contacts
// after the last pass (32 bytes, read and rewritten by its own lane only: no atomics, nothing to clear between passes).  A
// contact that is not among them is a Hit: one 32-byte record under the log's atomic cursor (which keeps counting when the
// log is full) and one count for the robot.  More simultaneous contacts than slots set the sticky word [1].
// A few hundred bytes of collider data per lane out of L2, no LDS; the launch is latency, not throughput.
static_assert(sizeof(mgx_env_collision_event) == 32, "the log's records are 32 bytes");
static_assert(offsetof(mgx_env_collision_event, robot) == offsetof(ContactEvent, a) && offsetof(mgx_env_collision_event, collider) == offsetof(ContactEvent, b) &&
                  offsetof(mgx_env_collision_event, mins) == offsetof(ContactEvent, mins) && offsetof(mgx_env_collision_event, maxs) == offsetof(ContactEvent, maxs),
              "ContactEvent is the ABI's record");
static_assert(ENV_COLL_SLOTS == 8, "the slots travel as two int4");

// (the contact itself, env_touches, is shared with the global planner: mgx_env_contact.h)

__global__ void __launch_bounds__(64) k_env_collisions(EnvCollDev c) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= c.n) return;
    int4 *slots = reinterpret_cast<int4 *>(c.touching + (size_t)ENV_COLL_SLOTS * i);
    const int4 o0 = slots[0], o1 = slots[1];
    const int32_t old[ENV_COLL_SLOTS] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
    int32_t cur[ENV_COLL_SLOTS] = {-1, -1, -1, -1, -1, -1, -1, -1};
    int n_cur = 0;
    const float x = c.pos[3 * i], z = c.pos[3 * i + 2], r = c.radius[i];
    if (c.alive[i] != 0 && isfinite(x) && isfinite(z) && r == r && c.n_colliders > 0) {
        const double reach = (double)fabsf(r) * 1.001 + c.pad;
        const int rx0 = env_cell_of((double)x - reach, c.x0, c.inv_cell, c.n_cx), rx1 = env_cell_of((double)x + reach, c.x0, c.inv_cell, c.n_cx);
        const int rz0 = env_cell_of((double)z - reach, c.z0, c.inv_cell, c.n_cz), rz1 = env_cell_of((double)z + reach, c.z0, c.inv_cell, c.n_cz);
        for (int cz = rz0; cz <= rz1; cz++)
            for (int cx = rx0; cx <= rx1; cx++) {
                const uint32_t cell = (uint32_t)cz * (uint32_t)c.n_cx + (uint32_t)cx;
                for (uint32_t q = c.cell_ptr[cell], q1 = c.cell_ptr[cell + 1]; q < q1; q++) {
                    const int32_t ki = c.cell_idx[q];
                    const EnvCollider &k = c.colliders[ki];
                    if (cx != max(rx0, k.cx0) || cz != max(rz0, k.cz0)) continue;  // met in an earlier cell, or will be
                    if (!env_touches(k, c.verts, x, z, r)) continue;
                    bool was = false;
#pragma unroll
                    for (int s = 0; s < ENV_COLL_SLOTS; s++) was = was || old[s] == ki;
                    if (n_cur < ENV_COLL_SLOTS) {
#pragma unroll
                        for (int s = 0; s < ENV_COLL_SLOTS; s++)
                            if (s == n_cur) cur[s] = ki;
                        n_cur++;
                    } else {
                        atomicOr(&c.log.words[1], 1ull);
                    }
                    if (was) continue;  // Colliding -> Colliding
                    contact_append(c.log, c.pass, i, ki, fmaxf(__fsub_rn(x, r), k.mins[0]), fmaxf(__fsub_rn(z, r), k.mins[1]),
                                   fminf(__fadd_rn(x, r), k.maxs[0]), fminf(__fadd_rn(z, r), k.maxs[1]));
                    c.per_robot[i] += 1u;  // (this lane's own word)
                }
            }
    }
    slots[0] = make_int4(cur[0], cur[1], cur[2], cur[3]);
    slots[1] = make_int4(cur[4], cur[5], cur[6], cur[7]);
}

hipError_t launch_env_collisions_pass(const EnvCollDev &c, hipStream_t s) {
    if (c.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_env_collisions, dim3((unsigned)((c.n + 63) / 64)), dim3(64), 0, s, c);
    return hipGetLastError();
}

}  // namespace mgx
