// mgx_grid.h — cells of the uniform grids: the hash grids of the neighbour search (mgx_topology.hip) and of the robot-robot
// collision pass (mgx_collisions.hip), and the map's tile grid of the robot-environment pass (kernel and host, mgx_world.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace mgx {

// cell coordinate of one axis: floor(x / cell) in f64, clamped (monotone, so robots within one
// radius of each other stay within one cell of each other)
__device__ __forceinline__ int cell_of(float x, double inv_cell) {
    double c = floor((double)x * inv_cell);
    c = fmin(fmax(c, -1073741824.0), 1073741824.0);
    return (int)c;
}
__device__ __forceinline__ uint32_t bucket_of(int cx, int cz, uint32_t mask) {
    return (((uint32_t)cx * 73856093u) ^ ((uint32_t)cz * 19349663u)) & mask;
}

// cell of a coordinate on the map's grid of n cells from `origin`: monotone, clamped into the grid.  The host files every collider
// under the cells the kernel will look in, so both sides take this one function.
__host__ __device__ inline int env_cell_of(double v, double origin, double inv_cell, int n) {
    const double c = floor((v - origin) * inv_cell);
    return (int)fmin(fmax(c, 0.0), (double)(n - 1));
}

}  // namespace mgx
