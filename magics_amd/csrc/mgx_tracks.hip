// mgx_tracks.hip — the robots' trackers on the device: PositionTracker / VelocityTracker samples
// (crates/magics/src/planner/tracking.rs:117-136, 210-240; 100 ms timers from planner/spawner.rs:627-628) and the distance every
// robot has travelled (export.rs:249-262).  Restated on the host by magics_amd/sim.py:_track / _tracks (samples) and
// magics_amd/driver.py:Driver.tick (distance), which are the checkers of this file.  The specification: include/mgx.h,
// "trackers on the device".
//
// One PASS at tick k, one lane per robot id, for the robots that moved in that tick:
//   * distance (the mission chain's pass only): c = ts * (mu_1 - mu_0) per axis — the f64 increment k_mission_prepare has just
//     cast into the Transform, formed again from the same means (the prior updates that change them run behind this pass) —
//     travelled += sqrt(c0*c0 + c1*c1), every operation rounded to f64 on its own.
//   * the timer: elapsed_ns += tick_ns; below the period nothing else happens, otherwise elapsed_ns %= period_ns and ONE sample
//     {k, robot, p, span = k - previous tick} is taken, with velocity (p - prev) / (float)(t(k) - t(k - span)) when there is a
//     previous sample, t(k) = (double)((k + 1) * tick_ns) * 1e-9.  Then prev = (p, k) — also when the log is full.
// The arithmetic is written with plain operators under `#pragma clang fp contract(off)`, so no build setting fuses anything (the
// *_rn intrinsics are inline functions of a header compiled under the build's own setting: they would be fused again); the f32
// division and the f64 square root are the correctly rounded ones: libmgx.so and libmgx_fma.so agree bit for bit.
//   log     append-only 40-byte records under an atomic cursor that keeps counting when the log is full (what did not fit is
//           cursor - capacity: nothing is lost silently); one atomic per sample, i.e. per robot every 100 ms of simulated time.
//   metrics (mgx_track_metrics.h; off unless mgx_track_metrics_enable): a robot that takes a sample also feeds the sample's velocity
//           to its jerk state and the sample's position, against its route, to its deviation state — 152 bytes of state and the
//           route's points, loaded and stored inside the sampling branch only.  k_track_metrics_read finalises copies.
// A lane touches its own robot's state only; no LDS, one wave per 64 robots.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mgx.h"
#include "mgx_dev.h"

#pragma clang fp contract(off)  // for every operation written below, whatever -ffp-contract says

namespace mgx {

static_assert(sizeof(mgx_track_sample) == 40 && sizeof(TrackSample) == 40 && sizeof(TrackState) == 40, "40-byte records");
static_assert(offsetof(mgx_track_sample, tick) == offsetof(TrackSample, tick) && offsetof(mgx_track_sample, robot) == offsetof(TrackSample, robot) &&
                  offsetof(mgx_track_sample, span_ticks) == offsetof(TrackSample, span_ticks) &&
                  offsetof(mgx_track_sample, position) == offsetof(TrackSample, position) &&
                  offsetof(mgx_track_sample, velocity) == offsetof(TrackSample, velocity),
              "TrackSample is the ABI's record");
static_assert(sizeof(mgx_track_metrics) == 48 && sizeof(TrackMetricsOut) == 48, "48-byte records");
static_assert(offsetof(mgx_track_metrics, n_positions) == offsetof(TrackMetricsOut, n_positions) &&
                  offsetof(mgx_track_metrics, n_velocities) == offsetof(TrackMetricsOut, n_velocities) &&
                  offsetof(mgx_track_metrics, n_unrouted) == offsetof(TrackMetricsOut, n_unrouted) &&
                  offsetof(mgx_track_metrics, flags) == offsetof(TrackMetricsOut, flags) &&
                  offsetof(mgx_track_metrics, dimensionless_jerk) == offsetof(TrackMetricsOut, dimensionless_jerk) &&
                  offsetof(mgx_track_metrics, vmax2) == offsetof(TrackMetricsOut, vmax2) &&
                  offsetof(mgx_track_metrics, deviation_sum) == offsetof(TrackMetricsOut, deviation_sum) &&
                  offsetof(mgx_track_metrics, deviation_max) == offsetof(TrackMetricsOut, deviation_max),
              "TrackMetricsOut is the ABI's record");
static_assert(MGX_TRACK_JERK_VALID == TRACK_METRICS_JERK_VALID && MGX_TRACK_DEVIATION_VALID == TRACK_METRICS_DEVIATION_VALID, "the record's flags");

// t(k): the simulated time at the end of tick k — an exact integer product, one f64 multiplication
__device__ __forceinline__ double track_time(unsigned long long k, unsigned long long tick_ns) {
    return (double)((k + 1ull) * tick_ns) * 1e-9;
}

__global__ void __launch_bounds__(64) k_tracks_pass(TrackDev t) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= t.n || !t.moved[r]) return;
    TrackState st = t.state[r];
    if (t.blob) {
        const BlobLayout L(t.K);
        const double *b = t.blob + (size_t)r * (size_t)t.BS;
        const double ts = t.time_scale[r];
        const double c0 = ts * (b[L.mu() + 0 * t.K + 1] - b[L.mu() + 0 * t.K + 0]);
        const double c1 = ts * (b[L.mu() + 1 * t.K + 1] - b[L.mu() + 1 * t.K + 0]);
        const double q0 = c0 * c0, q1 = c1 * c1;
        st.travelled = st.travelled + __builtin_sqrt(q0 + q1);
    }
    st.elapsed_ns += t.tick_ns;
    if (st.elapsed_ns >= t.period_ns) {
        st.elapsed_ns %= t.period_ns;
        TrackSample s;
        s.tick = t.tick;
        s.robot = r;
        s.span_ticks = st.has_prev ? (uint32_t)(t.tick - st.prev_tick) : 0u;
        const float dt = s.span_ticks ? (float)(track_time(t.tick, t.tick_ns) - track_time(st.prev_tick, t.tick_ns)) : 1.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float p = t.pos[3 * r + c];
            s.position[c] = p;
            const float d = p - st.prev[c];
            s.velocity[c] = s.span_ticks ? d / dt : 0.f;
            st.prev[c] = p;
        }
        st.prev_tick = t.tick;
        st.has_prev = 1u;
        if (!t.no_log) {
            const unsigned long long e = atomicAdd(t.cursor, 1ull);
            if (e < t.cap) t.log[e] = s;
        }
        if (t.metrics) {  // the run metrics: state and route are touched by the robots that take a sample only
            TrackMetricsState m = t.metrics[r];
            if (s.span_ticks) track_metrics_velocity(m, (double)s.velocity[0], (double)s.velocity[2]);
            const TrackRoute rt = t.routes[r];
            const uint32_t np = rt.count < t.max_route_points ? rt.count : t.max_route_points;
            track_metrics_position(m, (double)s.position[0], (double)s.position[2], t.route_xy + 2 * (size_t)rt.offset, np);
            t.metrics[r] = m;
        }
    }
    t.state[r] = st;
}

// every robot's metrics as if its series ended now, from a copy of the state: nothing is written back
__global__ void __launch_bounds__(64) k_track_metrics_read(int n, const TrackMetricsState *state, TrackMetricsOut *out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    out[r] = track_metrics_finalise(state[r]);
}

hipError_t launch_tracks_pass(const TrackDev &t, hipStream_t s) {
    if (t.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tracks_pass, dim3((unsigned)((t.n + 63) / 64)), dim3(64), 0, s, t);
    return hipGetLastError();
}

hipError_t launch_track_metrics_read(int n, const TrackMetricsState *state, TrackMetricsOut *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_track_metrics_read, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, state, out);
    return hipGetLastError();
}

}  // namespace mgx
