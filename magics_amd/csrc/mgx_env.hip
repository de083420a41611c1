// mgx_env.hip — the environment rasteriser on the device: env_to_png::env_to_image /
// env_to_sdf_image (crates/env_to_png/src/lib.rs:149-479) with the placeable shapes of
// gbp_environment (crates/gbp_environment/src/lib.rs:114-530), and image 0.25.1's
// imageops::blur (Cargo.lock:4052; vertical_sample + horizontal_sample, Gaussian of support
// 2 sigma) — what simulation_loader.rs:154-162 runs for every scenario before the first robot
// spawns.  Output: the u8 image ObstacleFactor::measure samples (factor/obstacle.rs:141-188).
//
// Division of labour.  Everything that is per ENVIRONMENT is computed on the host with the C
// library the reference's std calls (sinf / cosf / expf / sin / cos): tile thresholds, shape
// vertices, the rotation quaternion of every obstacle, the normalised blur weights of every output
// row / column.  Everything that is per PIXEL runs on the device and uses only + - * / floor ceil
// and comparisons in the reference's types (f32 for the coordinate maps, the rotation, circles and
// triangles; f64 for polygons and rectangles), which are correctly rounded on both sides, so the
// image is bit-identical to the CPU restatement (oracle/env.py).  FMA contraction is off for this
// file whatever the build (a*b+c fused would move pixels on shape borders).
//
// Byte work, HBM-bound: one thread per pixel, rows coalesced; the red plane only (the reference
// writes R = G = B and the factor reads pixel[0]).  The blur's vertical pass re-reads each source
// row once per tap through L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mgx.h"

#pragma clang fp contract(off)

extern "C" int mgx_set_error_(int code, const char *text);  // mgx_world.hip: thread-local last error

namespace mgx {

static int env_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mgx_set_error_(code, buf);
}
#define ENV_HIP(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) return env_fail(MGX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// one placeable obstacle, constants only (device record)
struct EnvObstacle {
    int32_t kind, row, col;
    int32_t n, p0;     // regular polygon / polygon: vertex count and first vertex in `pts`
    float tx, ty;      // translation as f32 (Vec2::from(RelativePoint))
    float s, c, k;     // Quat::from_rotation_z: sin, cos of the half angle; k = c c - s s
    float f[6];        // circle: f[0] = (r r) as f32; triangle: ax ay bx by cx cy
    double hw, hh;     // rectangle: width / 4, height / 4
};

struct EnvRaster {
    uint32_t W, H, n_rows, n_cols, resolution;
    float res_f, tile_size;
    float ow, owp, lo, hi;  // is_tile_obstacle thresholds (lib.rs:346-351,368,376,384,392)
    int n_obstacles;
    const uint32_t *tiles;
    const EnvObstacle *obstacles;
    const double *pts;  // (x, y) pairs
    int *error;         // set when a Percentage::new assertion of the reference would fire
};

// tile_units_to_percentage(image_to_tile_units(..)) (lib.rs:208-243)
__device__ __forceinline__ float pixel_percentage(uint32_t p, float res, float tile_size) {
    const float u = ((float)p + 0.5f) / res * tile_size;
    return -(ceilf(u / tile_size) * tile_size - u) / tile_size + 1.0f;
}

__device__ bool tile_obstacle(uint32_t tile, float px, float py, const EnvRaster &e) {  // lib.rs:338-479
    const bool xl = px < e.ow, xh = px > e.owp, yl = py < e.ow, yh = py > e.owp;
    switch (tile) {
    case 0x2500: return yl || yh;                    // ─
    case 0x2502: return xl || xh;                    // │
    case 0x2574: return yl || yh || px > e.lo;       // ╴
    case 0x2576: return yl || yh || px < e.hi;       // ╶
    case 0x2577: return xl || xh || py < e.hi;       // ╷
    case 0x2575: return xl || xh || py > e.lo;       // ╵
    case 0x250C: return xl || yl || (xh && yh);      // ┌
    case 0x2510: return xh || yl || (xl && yh);      // ┐
    case 0x2514: return xl || yh || (xh && yl);      // └
    case 0x2518: return xh || yh || (xl && yl);      // ┘
    case 0x252C: return yl || (yh && (xl || xh));    // ┬
    case 0x2534: return yh || (yl && (xl || xh));    // ┴
    case 0x251C: return xl || (xh && (yl || yh));    // ├
    case 0x2524: return xh || (xl && (yl || yh));    // ┤
    case 0x253C: return (xl || xh) && (yl || yh);    // ┼
    case 0x20: return true;                          // ' '
    default: return false;
    }
}

__device__ bool shape_inside(const EnvObstacle &o, const double *pts, float x, float y) {
    switch (o.kind) {
    case MGX_SHAPE_CIRCLE:  // Circle::inside (gbp_environment lib.rs:139-143)
        return x * x + y * y <= o.f[0];
    case MGX_SHAPE_TRIANGLE: {  // Triangle::inside (lib.rs:206-223)
        const float ax = o.f[0], ay = o.f[1], bx = o.f[2], by = o.f[3], cx = o.f[4], cy = o.f[5];
        const float d1 = (x - bx) * (ay - by) - (ax - bx) * (y - by);
        const float d2 = (x - cx) * (by - cy) - (bx - cx) * (y - cy);
        const float d3 = (x - ax) * (cy - ay) - (cx - ax) * (y - ay);
        const bool has_neg = d1 < 0.0f || d2 < 0.0f || d3 < 0.0f, has_pos = d1 > 0.0f || d2 > 0.0f || d3 > 0.0f;
        return !(has_neg && has_pos);
    }
    case MGX_SHAPE_REGULAR_POLYGON: {  // RegularPolygon::inside (lib.rs:283-300)
        const double X = (double)x * 2.0, Y = (double)y * 2.0;
        bool inside = false;
        int j = o.n - 1;
        for (int i = 0; i < o.n; i++) {
            const double xi = pts[2 * (o.p0 + i)], yi = pts[2 * (o.p0 + i) + 1];
            const double xj = pts[2 * (o.p0 + j)], yj = pts[2 * (o.p0 + j) + 1];
            if ((yi < Y && yj >= Y) || (yj < Y && yi >= Y))
                if (xi + (Y - yi) / (yj - yi) * (xj - xi) < X) inside = !inside;
            j = i;
        }
        return inside;
    }
    case MGX_SHAPE_RECTANGLE: {  // Rectangle::inside (lib.rs:328-340)
        const double X = (double)x, Y = (double)y;
        return X >= -o.hh && X <= o.hh && Y >= -o.hw && Y <= o.hw;
    }
    case MGX_SHAPE_POLYGON: {  // is_point_in_polygon (lib.rs:398-415)
        const double X = (double)x, Y = (double)y;
        bool inside = false;
        int j = o.n - 1;
        for (int i = 0; i < o.n; i++) {
            const double ix = pts[2 * (o.p0 + i)], iy = pts[2 * (o.p0 + i) + 1];
            const double jx = pts[2 * (o.p0 + j)], jy = pts[2 * (o.p0 + j) + 1];
            if ((iy > Y) != (jy > Y) && X < (jx - ix) * (Y - iy) / (jy - iy) + ix) inside = !inside;
            j = i;
        }
        return inside;
    }
    default: return false;
    }
}

// four horizontally adjacent bytes per thread go out as one 32-bit store when the rows allow it
__device__ __forceinline__ void store4(uint8_t *__restrict__ out, uint32_t W, uint32_t x, uint32_t y, const uint8_t (&v)[4]) {
    uint8_t *p = out + (size_t)y * W + x;
    if ((W & 3u) == 0 && x + 3 < W) {
        *reinterpret_cast<uint32_t *>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
        for (uint32_t i = 0; i < 4 && x + i < W; i++) p[i] = v[i];
    }
}

// env_to_image (lib.rs:165-206): one thread per four pixels of a row of the red plane
__global__ void __launch_bounds__(256) k_env_raster(EnvRaster e, uint8_t *__restrict__ out) {
    const uint32_t x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x0 >= e.W || y >= e.H) return;
    const uint32_t tcy = (uint32_t)floorf((float)y / e.res_f);  // lib.rs:248-257
    const float py = pixel_percentage(y, e.res_f, e.tile_size);
    uint8_t v[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < 4 && x0 + i < e.W; i++) {
        const uint32_t x = x0 + i;
        const uint32_t tcx = (uint32_t)floorf((float)x / e.res_f);
        const float px = pixel_percentage(x, e.res_f, e.tile_size);
        if (!(px >= 0.0f && px <= 1.0f && py >= 0.0f && py <= 1.0f) || tcx >= e.n_cols || tcy >= e.n_rows) {
            *e.error = 1;  // Percentage::new assert / "Tile not found"
            continue;
        }
        bool obstacle = tile_obstacle(e.tiles[tcy * e.n_cols + tcx], px, py, e);
        for (int q = 0; q < e.n_obstacles && !obstacle; q++) {  // is_placeable_obstacle (lib.rs:279-336)
            const EnvObstacle &o = e.obstacles[q];
            if ((uint32_t)o.col != tcx || (uint32_t)o.row != tcy) continue;
            const float tx = px - o.tx, ty = py - o.ty;
            // glam Quat::from_rotation_z(a).mul_vec3((tx, ty, 0)): v (w w - b.b) + b (2 v.b) + (w (b x v)) 2, b = (0, 0, s)
            const float rx = (tx * o.k + 0.0f) + (o.c * (0.0f - ty * o.s)) * 2.0f;
            const float ry = (ty * o.k + 0.0f) + (o.c * (o.s * tx)) * 2.0f;
            obstacle = shape_inside(o, e.pts, rx, ry);
        }
        v[i] = obstacle ? 0 : 255;
    }
    store4(out, e.W, x0, y, v);
}

// imageops::blur, first pass (vertical_sample): u8 plane -> f32 plane.  Row `o` of the output is the
// weighted sum of rows left[o] .. left[o] + cnt[o] - 1, accumulated in f32 in tap order.  One thread
// per four pixels of a row: a 32-bit load per tap, a 16-byte store.
__global__ void __launch_bounds__(256) k_blur_vertical(const uint8_t *__restrict__ src, float *__restrict__ tmp, uint32_t W, uint32_t H,
                                                       const int32_t *__restrict__ left, const int32_t *__restrict__ cnt,
                                                       const float *__restrict__ wgt, int T) {
    const uint32_t x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, o = blockIdx.y;
    if (x0 >= W || o >= H) return;
    const int l = left[o], n = cnt[o];
    const float *w = wgt + (size_t)o * T;
    float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if ((W & 3u) == 0) {
        for (int i = 0; i < n; i++) {
            const uint32_t q = *reinterpret_cast<const uint32_t *>(src + (size_t)(l + i) * W + x0);
            const float wi = w[i];
#pragma unroll
            for (int c = 0; c < 4; c++) t[c] += (float)((q >> (8 * c)) & 0xffu) * wi;
        }
        *reinterpret_cast<float4 *>(tmp + (size_t)o * W + x0) = make_float4(t[0], t[1], t[2], t[3]);
    } else {
        for (uint32_t c = 0; c < 4 && x0 + c < W; c++) {
            for (int i = 0; i < n; i++) t[c] += (float)src[(size_t)(l + i) * W + x0 + c] * w[i];
            tmp[(size_t)o * W + x0 + c] = t[c];
        }
    }
}
// second pass (horizontal_sample): f32 plane -> u8, clamp to [0, 255] and round half away from zero.
// One output per thread; the 256 outputs of a workgroup read overlapping windows of one row, so the
// row segment they cover (256 + taps floats) is staged in LDS once instead of being fetched once per
// tap through L1 / L2; four lanes then merge their bytes so that every fourth lane issues one
// 32-bit store.  The weight table is tap-major ([tap][column]) so that a wave's weight loads coalesce.
constexpr int BLUR_TAPS_REG = 16;
__global__ void __launch_bounds__(256) k_blur_horizontal(const float *__restrict__ tmp, uint8_t *__restrict__ out, uint32_t W, uint32_t H,
                                                         const int32_t *__restrict__ left, const int32_t *__restrict__ cnt,
                                                         const float *__restrict__ wgt, int T, uint32_t rows) {
    // `rows` rows per workgroup: the column's weights are fetched once and reused (large images); small
    // images keep one row per workgroup so that the grid still fills the chip
    extern __shared__ float s_row[];
    const uint32_t o_first = blockIdx.x * blockDim.x, o = o_first + threadIdx.x, y0 = blockIdx.y * rows;
    const uint32_t o_last = (o_first + blockDim.x - 1 < W) ? o_first + blockDim.x - 1 : W - 1;
    const int lo = left[o_first], hi = left[o_last] + cnt[o_last];  // windows move right with the output
    const int l = (o < W) ? left[o] - lo : 0, n = (o < W) ? cnt[o] : 0;
    float wreg[BLUR_TAPS_REG];  // this column's weights, when they fit (sigma up to ~3 pixels)
    const bool in_regs = T <= BLUR_TAPS_REG;
    if (in_regs) {
#pragma unroll
        for (int i = 0; i < BLUR_TAPS_REG; i++) wreg[i] = (i < n) ? wgt[(size_t)i * W + o] : 0.0f;
    }
    for (uint32_t y = y0; y < y0 + rows && y < H; y++) {
        const float *row = tmp + (size_t)y * W;
        __syncthreads();  // the previous row's readers are done
        for (int j = threadIdx.x; j < hi - lo; j += blockDim.x) s_row[j] = row[lo + j];
        __syncthreads();
        uint32_t v = 0;
        if (o < W) {
            float t = 0.0f;
            if (in_regs) {
#pragma unroll
                for (int i = 0; i < BLUR_TAPS_REG; i++)
                    if (i < n) t += s_row[l + i] * wreg[i];
            } else {
                for (int i = 0; i < n; i++) t += s_row[l + i] * wgt[(size_t)i * W + o];
            }
            t = (t < 0.0f) ? 0.0f : (t > 255.0f ? 255.0f : t);
            v = (uint32_t)roundf(t);
        }
        const uint32_t v1 = __shfl_down(v, 1, 64), v2 = __shfl_down(v, 2, 64), v3 = __shfl_down(v, 3, 64);
        if (o < W) {
            if ((W & 3u) == 0) {
                if ((o & 3u) == 0) *reinterpret_cast<uint32_t *>(out + (size_t)y * W + o) = v | (v1 << 8) | (v2 << 16) | (v3 << 24);
            } else {
                out[(size_t)y * W + o] = (uint8_t)v;
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------
namespace {

bool percentage_ok(float v) { return v >= 0.0f && v <= 1.0f; }  // Percentage::new (lib.rs:52-57)
bool spf(double v) { return v > 0.0 && std::isfinite(v); }      // StrictlyPositiveFinite

// What is wrong with an ENVIRONMENT whatever the resolution or the expansion: the one validation env_red_plane and
// mgx_env_colliders share (the rasteriser adds what depends on its own arguments: resolution, expansion, blur)
int env_check(const mgx_env_desc *d) {
    if (!d || !d->tiles || !d->n_rows || !d->n_cols) return env_fail(MGX_ERR_INVALID, "EmptyGrid: environment matrix representation is empty");
    if (d->n_obstacles && !d->obstacles) return env_fail(MGX_ERR_INVALID, "null obstacle list");
    if (!percentage_ok(d->path_width)) return env_fail(MGX_ERR_INVALID, "percentage outside [0, 1]");
    for (uint32_t q = 0; q < d->n_obstacles; q++) {
        const mgx_env_obstacle &in = d->obstacles[q];
        if (!(in.translation_x >= 0.0 && in.translation_x <= 1.0 && in.translation_y >= 0.0 && in.translation_y <= 1.0))
            return env_fail(MGX_ERR_INVALID, "obstacle %u: Invalid relative point", q);
        if (!(in.rotation >= 0.0 && in.rotation <= 2.0 * 3.14159265358979323846))
            return env_fail(MGX_ERR_INVALID, "obstacle %u: Angle value %g is not inside [0,2pi]", q, in.rotation);
        switch (in.shape) {
        case MGX_SHAPE_CIRCLE:
        case MGX_SHAPE_TRIANGLE:
            if (!spf(in.radius)) return env_fail(MGX_ERR_INVALID, "obstacle %u: radius must be strictly positive and finite", q);
            break;
        case MGX_SHAPE_REGULAR_POLYGON:
            if (!spf(in.radius) || in.sides < 1) return env_fail(MGX_ERR_INVALID, "obstacle %u: bad regular polygon", q);
            break;
        case MGX_SHAPE_RECTANGLE:
            if (!spf(in.width) || !spf(in.height)) return env_fail(MGX_ERR_INVALID, "obstacle %u: width / height must be strictly positive and finite", q);
            break;
        case MGX_SHAPE_POLYGON:
            if (!in.n_points || !in.points_xy) return env_fail(MGX_ERR_INVALID, "obstacle %u: polygon without points", q);
            break;
        default: return env_fail(MGX_ERR_INVALID, "obstacle %u: unknown shape %d", q, in.shape);
        }
    }
    return MGX_OK;
}

// image::imageops::sample::gaussian
float gaussian(float x, float r) { return 1.0f / (sqrtf(2.0f * 3.14159265358979323846f) * r) * expf(-(x * x) / (2.0f * (r * r))); }

// taps of {vertical,horizontal}_sample when the new size equals the old one (ratio = sratio = 1)
void blur_taps(uint32_t n, float sigma, std::vector<int32_t> &left, std::vector<int32_t> &cnt, std::vector<float> &wgt, int &T) {
    const float support = 2.0f * sigma;
    T = (int)std::ceil(2.0 * (double)support) + 3;
    left.assign(n, 0);
    cnt.assign(n, 0);
    wgt.assign((size_t)n * T, 0.0f);
    for (uint32_t o = 0; o < n; o++) {
        float inp = ((float)o + 0.5f) * 1.0f;
        long long l = (long long)floorf(inp - support);
        l = l < 0 ? 0 : (l > (long long)n - 1 ? (long long)n - 1 : l);
        long long r = (long long)ceilf(inp + support);
        r = r < l + 1 ? l + 1 : (r > (long long)n ? (long long)n : r);
        inp = inp - 0.5f;
        float sum = 0.0f;
        float *w = wgt.data() + (size_t)o * T;
        int c = 0;
        for (long long i = l; i < r && c < T; i++, c++) {
            w[c] = gaussian(((float)i - inp) / 1.0f, sigma);
            sum += w[c];
        }
        for (int i = 0; i < c; i++) w[i] /= sum;
        left[o] = (int32_t)l;
        cnt[o] = c;
    }
}

template <class T>
struct Dev {
    T *p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    hipError_t put(const std::vector<T> &h, hipStream_t s) {
        hipError_t e = hipMalloc((void **)&p, sizeof(T) * (h.empty() ? 1 : h.size()));
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, s);
    }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(T) * (n ? n : 1)); }
};

}  // namespace

// Rasterises (and blurs when blur_percent * resolution >= 1) on stream `s`; returns the red plane.
int env_red_plane(const mgx_env_desc *d, uint32_t resolution, float expansion, float blur_percent, bool with_blur, hipStream_t s,
                  std::vector<uint8_t> &red, uint32_t &W, uint32_t &H) {
    if (const int rc = env_check(d)) return rc;
    if (!resolution) return env_fail(MGX_ERR_INVALID, "Pixels per tile must be non-zero");
    if (!percentage_ok(expansion) || !percentage_ok(d->path_width) || (with_blur && !percentage_ok(blur_percent)))
        return env_fail(MGX_ERR_INVALID, "percentage outside [0, 1]");
    if ((uint64_t)d->n_cols * resolution > (1u << 24) || (uint64_t)d->n_rows * resolution > 65535u)
        return env_fail(MGX_ERR_INVALID, "image too large");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return env_fail(MGX_ERR_NO_DEVICE, "no usable HIP device (the rasteriser has no CPU path)");

    EnvRaster e{};
    e.W = W = d->n_cols * resolution;
    e.H = H = d->n_rows * resolution;
    e.n_rows = d->n_rows; e.n_cols = d->n_cols; e.resolution = resolution;
    e.res_f = (float)resolution; e.tile_size = d->tile_size;
    {  // is_tile_obstacle's constants (lib.rs:346-351); each is a Percentage::new
        const float pw = d->path_width - expansion;
        const float almost_full = 1.0f - pw;
        e.ow = almost_full / 2.0f;
        e.owp = e.ow + pw;
        e.lo = 0.5f - expansion / 2.0f;
        e.hi = 0.5f + expansion / 2.0f;
        if (!percentage_ok(pw) || !percentage_ok(almost_full) || !percentage_ok(e.ow) || !percentage_ok(e.owp) || !percentage_ok(e.lo))
            return env_fail(MGX_ERR_INVALID, "percentage outside [0, 1] (path-width %g, expansion %g)", (double)d->path_width, (double)expansion);
        bool uses_hi = false;
        for (uint32_t i = 0; i < d->n_rows * d->n_cols; i++) uses_hi |= d->tiles[i] == 0x2576 || d->tiles[i] == 0x2577;
        if (uses_hi && !percentage_ok(e.hi)) return env_fail(MGX_ERR_INVALID, "percentage outside [0, 1]");
    }
    std::vector<EnvObstacle> obs;
    std::vector<double> pts;
    const double ex = (double)expansion;  // PlaceableShape::expanded(expansion.0 as f64), lib.rs:295
    const float PI32 = 3.14159265358979323846f, HALF_PI32 = 1.57079632679489661923f;
    for (uint32_t q = 0; q < d->n_obstacles; q++) {
        const mgx_env_obstacle &in = d->obstacles[q];
        EnvObstacle o{};
        o.kind = in.shape; o.row = in.tile_row; o.col = in.tile_col;
        o.tx = (float)in.translation_x; o.ty = (float)in.translation_y;
        float offset = HALF_PI32;  // lib.rs:299-312
        switch (in.shape) {
        case MGX_SHAPE_CIRCLE: {
            if (!spf(in.radius) || !spf(in.radius + ex)) return env_fail(MGX_ERR_INVALID, "obstacle %u: radius must be strictly positive and finite", q);
            const double r = in.radius + ex;
            o.f[0] = (float)(r * r);
            break;
        }
        case MGX_SHAPE_TRIANGLE: {  // Triangle::points (gbp_environment lib.rs:186-204)
            if (!spf(in.radius) || !spf(in.radius + ex)) return env_fail(MGX_ERR_INVALID, "obstacle %u: radius must be strictly positive and finite", q);
            const float a = (float)in.angle_a, b = (float)in.angle_b, c = PI32 - (a + b), r = (float)(in.radius + ex);
            const float hyp[3] = {r / sinf(a), r / sinf(b), r / sinf(c)};
            const float ang[3] = {PI32 + a / 2.0f, -b / 2.0f, PI32 - b - c / 2.0f};
            for (int v = 0; v < 3; v++) {
                o.f[2 * v] = cosf(ang[v]) * hyp[v];
                o.f[2 * v + 1] = sinf(ang[v]) * hyp[v];
            }
            break;
        }
        case MGX_SHAPE_REGULAR_POLYGON: {  // RegularPolygon::expanded / point_at (lib.rs:246-279)
            if (!spf(in.radius) || !spf(in.radius + ex * 2.0) || in.sides < 1) return env_fail(MGX_ERR_INVALID, "obstacle %u: bad regular polygon", q);
            const double r = in.radius + ex * 2.0;
            o.n = (int32_t)in.sides; o.p0 = (int32_t)(pts.size() / 2);
            for (uint32_t i = 0; i < in.sides; i++) {
                const double angle = 2.0 * 3.14159265358979323846 / (double)in.sides * (double)i + 0.78539816339744830962;
                pts.push_back(cos(angle) * r);
                pts.push_back(sin(angle) * r);
            }
            offset = HALF_PI32 + HALF_PI32 + ((in.sides % 2 != 0) ? PI32 / (float)in.sides : 0.0f);
            break;
        }
        case MGX_SHAPE_RECTANGLE: {  // Rectangle::expanded / inside (lib.rs:318-340)
            if (!spf(in.width) || !spf(in.height) || !spf(in.width + ex * 2.0) || !spf(in.height + ex * 2.0))
                return env_fail(MGX_ERR_INVALID, "obstacle %u: width / height must be strictly positive and finite", q);
            o.hw = (in.width + ex * 2.0) / 4.0;
            o.hh = (in.height + ex * 2.0) / 4.0;
            break;
        }
        case MGX_SHAPE_POLYGON: {  // Polygon::expanded (lib.rs:352-380)
            double ax = 0.0, ay = 0.0;
            for (uint32_t i = 0; i < in.n_points; i++) { ax = ax + in.points_xy[2 * i]; ay = ay + in.points_xy[2 * i + 1]; }
            const double cx = ax / (double)in.n_points, cy = ay / (double)in.n_points;
            o.n = (int32_t)in.n_points; o.p0 = (int32_t)(pts.size() / 2);
            for (uint32_t i = 0; i < in.n_points; i++) {
                const double x = in.points_xy[2 * i], y = in.points_xy[2 * i + 1];
                pts.push_back(x + (x - cx) * 4.0 * ex);
                pts.push_back(y + (y - cy) * 4.0 * ex);
            }
            offset = 0.0f;
            break;
        }
        default: return env_fail(MGX_ERR_INVALID, "obstacle %u: unknown shape %d", q, in.shape);
        }
        const float half = ((float)in.rotation + offset) * 0.5f;  // Quat::from_rotation_z
        o.s = sinf(half); o.c = cosf(half);
        o.k = o.c * o.c - o.s * o.s;
        obs.push_back(o);
    }

    Dev<uint32_t> tiles_d;
    Dev<EnvObstacle> obs_d;
    Dev<double> pts_d;
    Dev<int> err_d;
    Dev<uint8_t> plane, blurred;
    std::vector<uint32_t> tiles(d->tiles, d->tiles + (size_t)d->n_rows * d->n_cols);
    ENV_HIP(tiles_d.put(tiles, s));
    ENV_HIP(obs_d.put(obs, s));
    ENV_HIP(pts_d.put(pts, s));
    ENV_HIP(err_d.alloc(1));
    ENV_HIP(hipMemsetAsync(err_d.p, 0, sizeof(int), s));
    ENV_HIP(plane.alloc((size_t)W * H));
    e.n_obstacles = (int)obs.size();
    e.tiles = tiles_d.p; e.obstacles = obs_d.p; e.pts = pts_d.p; e.error = err_d.p;
    const dim3 grid((W + 1023) / 1024, H), block(256);  // four pixels of a row per thread
    hipLaunchKernelGGL(k_env_raster, grid, block, 0, s, e, plane.p);
    ENV_HIP(hipGetLastError());
    const uint8_t *result = plane.p;

    // env_to_sdf_image (lib.rs:149-163)
    std::vector<int32_t> vl, vc, hl, hc;
    std::vector<float> vw, hw;
    Dev<int32_t> vl_d, vc_d, hl_d, hc_d;
    Dev<float> vw_d, hw_d, tmp;
    const float blur_pixels = blur_percent * (float)resolution;
    if (with_blur && !(blur_pixels < 1.0f)) {
        const float sigma = blur_pixels <= 0.0f ? 1.0f : blur_pixels;
        int TV = 0, TH = 0;
        blur_taps(H, sigma, vl, vc, vw, TV);
        blur_taps(W, sigma, hl, hc, hw, TH);
        {  // the horizontal pass reads its weights tap-major ([tap][column]) so that a wave's loads coalesce
            std::vector<float> t((size_t)W * TH);
            for (uint32_t o = 0; o < W; o++)
                for (int i = 0; i < TH; i++) t[(size_t)i * W + o] = hw[(size_t)o * TH + i];
            hw.swap(t);
        }
        ENV_HIP(vl_d.put(vl, s)); ENV_HIP(vc_d.put(vc, s)); ENV_HIP(vw_d.put(vw, s));
        ENV_HIP(hl_d.put(hl, s)); ENV_HIP(hc_d.put(hc, s)); ENV_HIP(hw_d.put(hw, s));
        const uint32_t hrows = ((uint64_t)W * H >= (1u << 22)) ? 16u : ((uint64_t)W * H >= (1u << 19) ? 4u : 1u);
        ENV_HIP(tmp.alloc((size_t)W * H));
        ENV_HIP(blurred.alloc((size_t)W * H));
        hipLaunchKernelGGL(k_blur_vertical, grid, block, 0, s, plane.p, tmp.p, W, H, vl_d.p, vc_d.p, vw_d.p, TV);
        hipLaunchKernelGGL(k_blur_horizontal, dim3((W + 255) / 256, (H + hrows - 1) / hrows), block, sizeof(float) * (size_t)(256 + TH + 2), s, tmp.p, blurred.p, W, H,
                           hl_d.p, hc_d.p, hw_d.p, TH, hrows);
        ENV_HIP(hipGetLastError());
        result = blurred.p;
    }
    red.resize((size_t)W * H);
    int err = 0;
    ENV_HIP(hipMemcpyAsync(red.data(), result, red.size(), hipMemcpyDeviceToHost, s));
    ENV_HIP(hipMemcpyAsync(&err, err_d.p, sizeof(int), hipMemcpyDeviceToHost, s));
    ENV_HIP(hipStreamSynchronize(s));
    if (err) return env_fail(MGX_ERR_INVALID, "percentage outside [0, 1] or tile not found while rasterising");
    return MGX_OK;
}

// ---- the map's colliders (host code, no device needed) ------------------------------------------
// build_tile_grid piped into build_obstacles (crates/magics/src/environment/map_generator.rs:537-1293, 141-514) as plain data:
// what update_robot_environment_collisions (planner/collisions.rs:368-438) tests every robot against.  f32 arithmetic as the
// reference writes it (this file never contracts; its mul_add is fmaf); include/mgx.h says what is restated and how.
namespace {

struct P2 { float x, y; };

// Andrew's monotone chain: counter-clockwise, collinear points dropped (the cross products of f32 points in f64)
std::vector<P2> convex_hull(std::vector<P2> pts) {
    std::sort(pts.begin(), pts.end(), [](const P2 &a, const P2 &b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
    pts.erase(std::unique(pts.begin(), pts.end(), [](const P2 &a, const P2 &b) { return a.x == b.x && a.y == b.y; }), pts.end());
    const size_t n = pts.size();
    if (n < 3) return pts;
    auto cross = [](const P2 &o, const P2 &a, const P2 &b) {
        return ((double)a.x - o.x) * ((double)b.y - o.y) - ((double)a.y - o.y) * ((double)b.x - o.x);
    };
    std::vector<P2> h(2 * n);
    size_t k = 0;
    for (size_t i = 0; i < n; i++) {
        while (k >= 2 && cross(h[k - 2], h[k - 1], pts[i]) <= 0.0) k--;
        h[k++] = pts[i];
    }
    for (size_t i = n - 1, t = k + 1; i-- > 0;) {
        while (k >= t && cross(h[k - 2], h[k - 1], pts[i]) <= 0.0) k--;
        h[k++] = pts[i];
    }
    h.resize(k - 1);
    return h;
}

struct ColliderList {
    std::vector<mgx_env_collider> c;
    std::vector<float> v;  // world (x, z) pairs
    mgx_env_collider &push(int32_t kind, int32_t row, int32_t col, int32_t obstacle, float tx, float tz, float angle) {
        mgx_env_collider e{};
        e.kind = kind; e.tile_row = row; e.tile_col = col; e.obstacle = obstacle;
        e.tx = tx; e.tz = tz; e.angle = angle;
        c.push_back(e);
        return c.back();
    }
    // Bevy Cuboid::new(x, _, z) at Transform (tx, _, tz): half extents (x / 2, z / 2), no rotation
    void cuboid(int32_t row, int32_t col, int32_t obstacle, float hx, float hz, float tx, float tz) {
        mgx_env_collider &e = push(MGX_COLLIDER_CUBOID, row, col, obstacle, tx, tz, 0.0f);
        e.half_extents[0] = hx; e.half_extents[1] = hz;
        e.mins[0] = tx - hx; e.mins[1] = tz - hz;
        e.maxs[0] = tx + hx; e.maxs[1] = tz + hz;
    }
    // local points -> hull -> Isometry2::new((tx, tz), angle) * p (nalgebra UnitComplex: (re x - im y, im x + re y) + t)
    void polygon(int32_t row, int32_t col, int32_t obstacle, const std::vector<P2> &local, float tx, float tz, float angle) {
        const std::vector<P2> h = convex_hull(local);
        mgx_env_collider &e = push(MGX_COLLIDER_POLYGON, row, col, obstacle, tx, tz, angle);
        e.first_vertex = (uint32_t)(v.size() / 2);
        e.n_vertices = (uint32_t)h.size();
        const float re = cosf(angle), im = sinf(angle);
        for (size_t i = 0; i < h.size(); i++) {
            const float wx = (re * h[i].x - im * h[i].y) + tx, wz = (im * h[i].x + re * h[i].y) + tz;
            v.push_back(wx); v.push_back(wz);
            if (i == 0) { e.mins[0] = e.maxs[0] = wx; e.mins[1] = e.maxs[1] = wz; }
            e.mins[0] = std::min(e.mins[0], wx); e.maxs[0] = std::max(e.maxs[0], wx);
            e.mins[1] = std::min(e.mins[1], wz); e.maxs[1] = std::max(e.maxs[1], wz);
        }
    }
};

// build_tile_grid (map_generator.rs:537-1293)
void tile_colliders(const mgx_env_desc *d, ColliderList &L) {
    const float ts = d->tile_size, pw = d->path_width;
    const float base_dim = ts * (1.0f - pw) / 2.0f;                // :559
    const float gox = (float)d->n_cols / 2.0f - 0.5f;              // :563
    const float goz = -((float)d->n_rows / 2.0f - 0.5f);           // :564
    const float po = fmaf(pw, ts, base_dim) / 2.0f;                // :566
    const float full = ts / 2.0f, base = base_dim / 2.0f;          // half extents of tile_size / base_dim
    const float plug_long = (ts / 2.0f) / 2.0f, plug_wide = (pw * ts) / 2.0f, quarter = ts / 4.0f;
    for (uint32_t y = 0; y < d->n_rows; y++)
        for (uint32_t x = 0; x < d->n_cols; x++) {
            const float ox = ((float)x - gox) * ts, oz = (-(float)y - goz) * ts;  // :574-579
            const int32_t r = (int32_t)y, c = (int32_t)x;
            auto wide = [&](float tz) { L.cuboid(r, c, -1, full, base, ox, tz); };   // Cuboid::new(tile_size, _, base_dim)
            auto tall = [&](float tx) { L.cuboid(r, c, -1, base, full, tx, oz); };   // Cuboid::new(base_dim, _, tile_size)
            auto cube = [&](float tx, float tz) { L.cuboid(r, c, -1, base, base, tx, tz); };
            switch (d->tiles[y * d->n_cols + x]) {
            case 0x2500: case '-': wide(oz - po); wide(oz + po); break;                                             // ─ :582-614
            case 0x2502: case '|': tall(ox - po); tall(ox + po); break;                                             // │ :615-648
            case 0x2574: wide(oz - po); wide(oz + po); L.cuboid(r, c, -1, plug_long, plug_wide, ox + quarter, oz); break;  // ╴ :649-699
            case 0x2576: wide(oz - po); wide(oz + po); L.cuboid(r, c, -1, plug_long, plug_wide, ox - quarter, oz); break;  // ╶ :700-750
            case 0x2577: tall(ox - po); tall(ox + po); L.cuboid(r, c, -1, plug_wide, plug_long, ox, oz + quarter); break;  // ╷ :751-801
            case 0x2575: tall(ox - po); tall(ox + po); L.cuboid(r, c, -1, plug_wide, plug_long, ox, oz - quarter); break;  // ╵ :802-852
            case 0x250C: cube(ox + po, oz - po); tall(ox - po); wide(oz + po); break;                               // ┌ :853-897
            case 0x2510: cube(ox - po, oz - po); tall(ox + po); wide(oz + po); break;                               // ┐ :898-941
            case 0x2514: cube(ox + po, oz + po); tall(ox - po); wide(oz - po); break;                               // └ :942-986
            case 0x2518: cube(ox - po, oz + po); tall(ox + po); wide(oz - po); break;                               // ┘ :987-1031
            case 0x252C: cube(ox - po, oz - po); cube(ox + po, oz - po); wide(oz + po); break;                      // ┬ :1032-1072
            case 0x2534: cube(ox - po, oz + po); cube(ox + po, oz + po); wide(oz - po); break;                      // ┴ :1073-1113
            case 0x251C: cube(ox + po, oz - po); cube(ox + po, oz + po); tall(ox - po); break;                      // ├ :1114-1154
            case 0x2524: cube(ox - po, oz - po); cube(ox - po, oz + po); tall(ox + po); break;                      // ┤ :1155-1195
            case 0x253C: cube(ox - po, oz - po); cube(ox + po, oz - po); cube(ox - po, oz + po); cube(ox + po, oz + po); break;  // ┼ :1196-1244
            case 0x20: L.cuboid(r, c, -1, full, full, ox, oz); break;                                               // ' ' :1245-1255
            default: break;                                                                                         // _ => None
            }
        }
}

// build_obstacles (map_generator.rs:141-514)
void obstacle_colliders(const mgx_env_desc *d, ColliderList &L) {
    const float ts = d->tile_size;
    const float PI32 = 3.14159265358979323846f, HALF_PI32 = 1.57079632679489661923f;
    const float gox = (float)d->n_cols / 2.0f - 0.5f, goz = (float)d->n_rows / 2.0f - 0.5f;  // :154-155
    for (uint32_t q = 0; q < d->n_obstacles; q++) {
        const mgx_env_obstacle &in = d->obstacles[q];
        const int32_t row = in.tile_row, col = in.tile_col, ix = (int32_t)q;
        const float ox = ((float)col - gox) * ts, oz = ((float)row - goz) * ts;  // :169-173
        const float po = ts / 2.0f;                                             // :175
        const float tx = (float)in.translation_x, ty = (float)in.translation_y, rot = (float)in.rotation;
        const float cx = fmaf(tx, ts, ox) - po;
        const float cz_neg = -(fmaf(ty, ts, oz) - po);  // triangle, regular polygon, rectangle
        switch (in.shape) {
        case MGX_SHAPE_CIRCLE: {  // :181-208
            const float cz = fmaf(1.0f - ty, ts, oz) - po, radius = (float)in.radius * ts;
            mgx_env_collider &e = L.push(MGX_COLLIDER_BALL, row, col, ix, cx, cz, 0.0f);
            e.radius = radius;
            e.mins[0] = cx - radius; e.mins[1] = cz - radius;
            e.maxs[0] = cx + radius; e.maxs[1] = cz + radius;
            break;
        }
        case MGX_SHAPE_TRIANGLE: {  // :209-276, Triangle::points (gbp_environment lib.rs:192-210)
            const float a = (float)in.angle_a, b = (float)in.angle_b, c = PI32 - (a + b), r = (float)in.radius;
            const float hyp[3] = {r / sinf(a), r / sinf(b), r / sinf(c)};
            const float ang[3] = {PI32 + a / 2.0f, -b / 2.0f, PI32 - b - c / 2.0f};
            const float rotation_angle = HALF_PI32 - rot;              // :253-254
            const float hs = sinf(rotation_angle * 0.5f), hc = cosf(rotation_angle * 0.5f), k = hc * hc - hs * hs;
            std::vector<P2> pts;
            for (int v = 0; v < 3; v++) {
                const float px = -(cosf(ang[v]) * hyp[v]) * ts, py = (sinf(ang[v]) * hyp[v]) * ts;  // :227-229
                // glam Quat::from_rotation_y(a).mul_vec3((px, 0, py)).xz(): v (w w - b.b) + b (2 v.b) + (w (b x v)) 2, b = (0, s, 0)
                pts.push_back({px * k + (hc * (hs * py)) * 2.0f, py * k + (hc * (0.0f - hs * px)) * 2.0f});
            }
            L.polygon(row, col, ix, pts, cx, cz_neg, rotation_angle - HALF_PI32);  // :257-260
            break;
        }
        case MGX_SHAPE_REGULAR_POLYGON: {  // :277-379, RegularPolygon::points (lib.rs:271-294)
            const float rotation_offset = PI32 + (in.sides == 4 ? 0.0f : (in.sides % 2 != 0 ? HALF_PI32 : -HALF_PI32));  // :323-328
            const float rotation_angle = rot + rotation_offset;        // :342
            const float hs = sinf(rotation_angle * 0.5f), hc = cosf(rotation_angle * 0.5f), k = hc * hc - hs * hs;
            const float scale = ts / 2.0f;
            std::vector<P2> pts;
            for (uint32_t i = 0; i < in.sides; i++) {
                const double angle = 2.0 * 3.14159265358979323846 / (double)in.sides * (double)i + 0.78539816339744830962;
                const float px = (float)(cos(angle) * in.radius), py = (float)(sin(angle) * in.radius);
                // Quat::from_rotation_z(a).mul_vec3((px, py, 0)), b = (0, 0, s)
                const float rx = px * k + (hc * (0.0f - hs * py)) * 2.0f, ry = py * k + (hc * (hs * px)) * 2.0f;
                pts.push_back({rx * scale, ry * scale});
            }
            L.polygon(row, col, ix, pts, cx, cz_neg, rotation_angle);  // :373-376
            break;
        }
        case MGX_SHAPE_POLYGON: {  // :380-429
            const float cz = fmaf(ty, ts, oz) - po;
            std::vector<P2> pts;
            for (uint32_t i = 0; i < in.n_points; i++) pts.push_back({(float)in.points_xy[2 * i] * ts, (float)in.points_xy[2 * i + 1] * ts});
            L.polygon(row, col, ix, pts, cx, cz, 0.0f);
            break;
        }
        case MGX_SHAPE_RECTANGLE:  // :430-477
            L.cuboid(row, col, ix, (float)in.width * ts / 4.0f, (float)in.height * ts / 4.0f, cx, cz_neg);
            break;
        default: break;
        }
    }
}

}  // namespace

}  // namespace mgx

extern "C" {

int mgx_env_colliders(const mgx_env_desc *env, mgx_env_collider *out, uint32_t capacity, uint32_t *n, float *vertices_xz, uint32_t vertex_capacity,
                      uint32_t *n_vertices) {
    const int rc = mgx::env_check(env);
    if (rc != MGX_OK) return rc;
    if ((!out && capacity) || (!vertices_xz && vertex_capacity)) return mgx::env_fail(MGX_ERR_INVALID, "null output with a capacity");
    mgx::ColliderList L;
    mgx::tile_colliders(env, L);
    mgx::obstacle_colliders(env, L);
    if (n) *n = (uint32_t)L.c.size();
    if (n_vertices) *n_vertices = (uint32_t)(L.v.size() / 2);
    if (!capacity && !vertex_capacity) return MGX_OK;  // the capacity query
    if (capacity < L.c.size() || vertex_capacity < L.v.size() / 2)
        return mgx::env_fail(MGX_ERR_INVALID, "room for %u colliders and %u vertices, the environment has %zu and %zu", capacity, vertex_capacity, L.c.size(), L.v.size() / 2);
    std::copy(L.c.begin(), L.c.end(), out);
    std::copy(L.v.begin(), L.v.end(), vertices_xz);
    return MGX_OK;
}

int mgx_env_image_size(const mgx_env_desc *env, uint32_t resolution, uint32_t *width, uint32_t *height) {
    if (!env || !width || !height || !resolution) return mgx::env_fail(MGX_ERR_INVALID, "bad arguments");
    *width = env->n_cols * resolution;
    *height = env->n_rows * resolution;
    return MGX_OK;
}

static int to_rgb(const mgx_env_desc *env, uint32_t resolution, float expansion, float blur, bool with_blur, uint8_t *rgb) {
    if (!rgb) return mgx::env_fail(MGX_ERR_INVALID, "null image buffer");
    std::vector<uint8_t> red;
    uint32_t W = 0, H = 0;
    const int rc = mgx::env_red_plane(env, resolution, expansion, blur, with_blur, nullptr, red, W, H);
    if (rc != MGX_OK) return rc;
    for (size_t i = 0; i < red.size(); i++) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = red[i];
    return MGX_OK;
}

int mgx_env_to_image(const mgx_env_desc *env, uint32_t resolution, float expansion, uint8_t *rgb) {
    return to_rgb(env, resolution, expansion, 0.0f, false, rgb);
}

int mgx_env_to_sdf_image(const mgx_env_desc *env, uint32_t resolution, float expansion, float blur_percent, uint8_t *rgb) {
    return to_rgb(env, resolution, expansion, blur_percent, true, rgb);
}

}  // extern "C"
