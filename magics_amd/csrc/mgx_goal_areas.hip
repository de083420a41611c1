// mgx_goal_areas.hip — goal areas on the device: the first arrival of every robot in every area (goal_area::detect_collisions,
// crates/magics/src/goal_area.rs:67-103; restated on the host by magics_amd/sim.py:_goal_areas_host, which is the checker of
// this file).  include/mgx.h holds the specification.
//
// One PASS at tick k looks at the robots alive at that moment and their Transforms (x, z) as f32, radius r = (float)desc.radius:
// robot i touches area a iff the cuboid contact of mgx_env_contact.h holds for the area's centre and half extents (the very
// predicate of the robot-environment pass: nothing is contracted, libmgx.so and libmgx_fma.so agree; a NaN anywhere: no
// contact).  The first time they touch, first[a][i] = k + 1; a cell that is set is never written again
// (history.contains_key -> continue).
//
// STATE: first[n_areas][stride], u32, 0 = never — keyed by robot ID, so nothing moves when the world lays its arrays out again;
// stride is the robots a row has room for (the head-room of a reserved world), n the robots the world has.
// One lane per robot.  The area table is at most 64 x 16 bytes: the first lanes of a workgroup (one wave) stage it in LDS once,
// every lane then walks it there.  Cell (a, i) is written by lane i of this pass only, and only while it holds 0; passes are
// ordered by the stream: plain vector loads and stores — no atomics, no log, no capacity that can overflow.  The cell is read
// only when the two touch, so a pass over robots that touch nothing reads x, z, the radius and the alive byte of each and writes nothing.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mgx.h"
#include "mgx_dev.h"
#include "mgx_env_contact.h"

namespace mgx {

constexpr int GOAL_BLOCK = 64;
static_assert(GOAL_AREAS_MAX == (int)MGX_GOAL_AREAS_MAX && GOAL_AREAS_MAX <= GOAL_BLOCK, "one lane stages one area");
static_assert(sizeof(mgx_goal_area) == 16 && sizeof(mgx_goal_arrival) == 16 && sizeof(GoalAreaRec) == 16, "16-byte records");

__global__ void __launch_bounds__(GOAL_BLOCK) k_goal_areas(GoalAreasDev g) {
    __shared__ GoalAreaRec A[GOAL_AREAS_MAX];
    const int t = (int)threadIdx.x;
    const int n_areas = min(g.n_areas, GOAL_AREAS_MAX);
    if (t < n_areas) A[t] = g.areas[t];
    __syncthreads();
    const int i = (int)blockIdx.x * GOAL_BLOCK + t;
    if (i >= g.n || (uint32_t)i >= g.stride || g.alive[i] == 0) return;
    const float x = g.pos[3 * (size_t)i], z = g.pos[3 * (size_t)i + 2], r = g.radius[i];
    for (int a = 0; a < n_areas; a++) {
        const GoalAreaRec k = A[a];
        if (!cuboid_touches(k.cx, k.cz, k.hx, k.hz, x, z, r)) continue;
        uint32_t *cell = g.first + (size_t)a * g.stride + (size_t)i;
        if (*cell == 0u) *cell = g.stamp;
    }
}

hipError_t launch_goal_areas_pass(const GoalAreasDev &g, hipStream_t s) {
    if (g.n <= 0 || g.n_areas <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_goal_areas, dim3((unsigned)((g.n + GOAL_BLOCK - 1) / GOAL_BLOCK)), dim3(GOAL_BLOCK), 0, s, g);
    return hipGetLastError();
}

}  // namespace mgx
