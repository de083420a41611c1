// mgx_env_contact.h — the contact of include/mgx.h ("specification of a contact") on the device, and the walk over the map's tile
// grid that finds the colliders a ball can touch.  Shared by the robot-environment collision pass (mgx_collisions.hip) and the
// global planner's feasibility test (mgx_planner.hip); sim.py:environment_contacts restates the predicate on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mgx.h"
#include "mgx_dev.h"
#include "mgx_grid.h"

namespace mgx {

__device__ __forceinline__ float sq_sum(float a, float b) { return __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)); }

// the cuboid line of that contact: centre (tx, tz), half extents (hx, hz), no rotation.  env_touches' cuboid arm, and the whole
// contact of a goal area (mgx_goal_areas.hip)
__device__ __forceinline__ bool cuboid_touches(float tx, float tz, float hx, float hz, float x, float z, float r) {
    const float dx = __fsub_rn(fabsf(__fsub_rn(x, tx)), hx), dz = __fsub_rn(fabsf(__fsub_rn(z, tz)), hz);
    if (dx != dx || dz != dz) return false;  // (fmaxf below would drop a NaN)
    return sq_sum(fmaxf(dx, 0.f), fmaxf(dz, 0.f)) <= __fmul_rn(r, r);
}

// the contact of include/mgx.h: every operation rounded to f32 on its own; a NaN anywhere: false
__device__ inline bool env_touches(const EnvCollider &k, const float *__restrict__ verts, float x, float z, float r) {
    switch (k.kind) {
    case MGX_COLLIDER_BALL: {
        const float rs = __fadd_rn(r, k.radius);
        return sq_sum(__fsub_rn(x, k.tx), __fsub_rn(z, k.tz)) <= __fmul_rn(rs, rs);
    }
    case MGX_COLLIDER_CUBOID: return cuboid_touches(k.tx, k.tz, k.hx, k.hz, x, z, r);
    case MGX_COLLIDER_POLYGON: {
        const uint32_t n = k.n_vertices;
        if (n == 0) return false;
        const float *v = verts + 2 * (size_t)k.first_vertex;
        bool inside = n >= 3 && r == r;
        float best = INFINITY;
        float ax = v[2 * (n - 1)], az = v[2 * (n - 1) + 1];  // edge n-1 first: v_{n-1} -> v_0
        for (uint32_t i = 0; i < n; i++) {
            const float bx = v[2 * i], bz = v[2 * i + 1];
            const float ex = __fsub_rn(bx, ax), ez = __fsub_rn(bz, az), qx = __fsub_rn(x, ax), qz = __fsub_rn(z, az);
            inside = inside && (__fsub_rn(__fmul_rn(ex, qz), __fmul_rn(ez, qx)) >= 0.f);
            const float len2 = sq_sum(ex, ez);
            float t = len2 == 0.f ? 0.f : __fdiv_rn(__fadd_rn(__fmul_rn(qx, ex), __fmul_rn(qz, ez)), len2);
            if (t != t) return false;
            t = fminf(fmaxf(t, 0.f), 1.f);
            const float d2 = sq_sum(__fsub_rn(qx, __fmul_rn(t, ex)), __fsub_rn(qz, __fmul_rn(t, ez)));
            if (d2 != d2) return false;
            best = fminf(best, d2);
            ax = bx; az = bz;
        }
        return inside || best <= __fmul_rn(r, r);
    }
    default: return false;
    }
}

// the cells (inclusive ranges) whose colliders a ball of radius r at (x, z) can touch: its AABB, padded by what covers the roundings
// of the f32 predicate, clamped into the grid
struct EnvCellRange { int x0, x1, z0, z1; };
__device__ __forceinline__ EnvCellRange env_cells_of_ball(const EnvMapDev &m, float x, float z, float r) {
    const double reach = (double)fabsf(r) * 1.001 + m.pad;
    EnvCellRange c;
    c.x0 = env_cell_of((double)x - reach, m.x0, m.inv_cell, m.n_cx); c.x1 = env_cell_of((double)x + reach, m.x0, m.inv_cell, m.n_cx);
    c.z0 = env_cell_of((double)z - reach, m.z0, m.inv_cell, m.n_cz); c.z1 = env_cell_of((double)z + reach, m.z0, m.inv_cell, m.n_cz);
    return c;
}

}  // namespace mgx
