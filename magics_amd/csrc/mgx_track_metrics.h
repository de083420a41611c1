// mgx_track_metrics.h — the lane arithmetic of the run metrics the trackers carry per robot: the dimensionless jerk of the velocity
// samples (the reference's scripts/ldj.py with the times cancelled out) and the perpendicular deviation of the position samples from
// the route's lines (scripts/perpendicular-path-deviation.py).  The specification: include/mgx.h, "run metrics on the device".
// Three functions of one robot's state: take a velocity, take a position against a route, finalise a COPY of the state.  They are
// called by k_tracks_pass / k_track_metrics_read (mgx_tracks.hip) and compile on the host as they stand (tests/cpu_metrics);
// magics_amd/track_metrics.py restates them operation by operation and is their checker.
// All arithmetic is f64, every operation rounded on its own, written with plain operators: nothing here may be contracted,
// whatever the build says.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MGX_TM_HD __host__ __device__ __forceinline__
#else
#define MGX_TM_HD inline
#endif

// clang: the pragma opens every function body below, so it ends with the function and an including unit keeps its own setting
#if defined(__clang__)
#define MGX_TM_EXACT _Pragma("clang fp contract(off)")
#else
#define MGX_TM_EXACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

namespace mgx {

// 152 bytes; all zero: a robot nobody has sampled yet.  u / w: the last five velocities, [4] the newest.
struct TrackMetricsState {
    double u[5], w[5];
    double q0;             // q_0, settled with the fourth velocity
    double s_odd, s_even;  // sums of the settled q_i in arrival order: odd i from q_1 on, even i from q_2 on — up to i = n - 4
    double hold;           // q_{n-3}, the most recent settled one (n >= 5): its weight depends on the parity of the final n
    double vmax2;
    double dev_sum, dev_max;
    uint32_t n_vel, n_pos, n_unrouted, reserved;
};
static_assert(sizeof(TrackMetricsState) == 152, "152-byte state");

struct TrackMetricsOut {   // == mgx_track_metrics (include/mgx.h; mgx_tracks.hip asserts it)
    uint32_t n_positions, n_velocities, n_unrouted, flags;
    double dimensionless_jerk, vmax2, deviation_sum, deviation_max;
};
constexpr uint32_t TRACK_METRICS_JERK_VALID = 1u, TRACK_METRICS_DEVIATION_VALID = 2u;

MGX_TM_HD double tm_sq2(double a, double b) {
    MGX_TM_EXACT
    const double a2 = a * a, b2 = b * b;
    return a2 + b2;
}

// one more velocity (u, w) of the series, index m = n_vel
MGX_TM_HD void track_metrics_velocity(TrackMetricsState &s, double u, double w) {
    MGX_TM_EXACT
    const uint32_t m = s.n_vel;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s.u[i] = s.u[i + 1];
        s.w[i] = s.w[i + 1];
    }
    s.u[4] = u;
    s.w[4] = w;
    const double v2 = tm_sq2(u, w);
    s.vmax2 = v2 > s.vmax2 ? v2 : s.vmax2;
    s.n_vel = m + 1u;
    // Both cases are formed whatever m is and the state takes what applies through selects: branches here ended as stores through
    // a selected address, i.e. as scratch in the tracker pass.
    // m == 3: x_0 .. x_3 are [1] .. [4] — q_0 and q_1 settle (a_0 one-sided, a_1 and a_2 central)
    const double au0 = s.u[2] - s.u[1], aw0 = s.w[2] - s.w[1];
    const double au1 = (s.u[3] - s.u[1]) / 2.0, aw1 = (s.w[3] - s.w[1]) / 2.0;
    const double aup = (s.u[4] - s.u[2]) / 2.0, awp = (s.w[4] - s.w[2]) / 2.0;  // a_2 there, a_{m-1} below
    const double q0 = tm_sq2(au1 - au0, aw1 - aw0);
    const double q1 = tm_sq2((aup - au0) / 2.0, (awp - aw0) / 2.0);
    // m >= 4: q_{m-2} settles — central differences of central differences over x_{m-4} .. x_m
    const double aum = (s.u[2] - s.u[0]) / 2.0, awm = (s.w[2] - s.w[0]) / 2.0;
    const double q = tm_sq2((aup - aum) / 2.0, (awp - awm) / 2.0);
    // m >= 5: the one held back so far, q_{m-3}, joins the sum of its parity
    const bool odd = ((m - 3u) & 1u) != 0u;
    const double so = s.s_odd + s.hold, se = s.s_even + s.hold;
    s.q0 = m == 3u ? q0 : s.q0;
    s.s_odd = m == 3u ? q1 : (m >= 5u && odd ? so : s.s_odd);
    s.s_even = m >= 5u && !odd ? se : s.s_even;
    s.hold = m >= 4u ? q : s.hold;
}

// one more position (px, py) against a route of `n_points` points (x, y) — the distance to the nearest of the infinite lines
// through consecutive points, segments of zero length left out
MGX_TM_HD void track_metrics_position(TrackMetricsState &s, double px, double py, const double *route_xy, uint32_t n_points) {
    MGX_TM_EXACT
    bool found = false;
    double best = 0.0;
    for (uint32_t k = 0; k + 1u < n_points; k++) {
        const double ax = route_xy[2 * k], ay = route_xy[2 * k + 1];
        const double dx = route_xy[2 * k + 2] - ax, dy = route_xy[2 * k + 3] - ay;
        const double l2 = tm_sq2(dx, dy);
        if (!(l2 > 0.0)) continue;
        const double c1 = dx * (py - ay), c2 = dy * (px - ax);
        const double d = __builtin_fabs(c1 - c2) / __builtin_sqrt(l2);
        if (!found || d < best) best = d;
        found = true;
    }
    if (!found) {
        s.n_unrouted += 1u;
        return;
    }
    s.dev_sum = s.dev_sum + best;
    s.dev_max = best > s.dev_max ? best : s.dev_max;
    s.n_pos += 1u;
}

// what the state amounts to if the series ended here; the state is not changed
MGX_TM_HD TrackMetricsOut track_metrics_finalise(const TrackMetricsState &s) {
    MGX_TM_EXACT
    TrackMetricsOut o;
    const uint32_t n = s.n_vel;
    o.n_positions = s.n_pos;
    o.n_velocities = n;
    o.n_unrouted = s.n_unrouted;
    o.flags = s.n_pos ? TRACK_METRICS_DEVIATION_VALID : 0u;
    o.vmax2 = s.vmax2;
    o.deviation_sum = s.dev_sum;
    o.deviation_max = s.dev_max;
    o.dimensionless_jerk = __builtin_nan("");
    if (n < 3u || !(s.vmax2 > 0.0)) return o;
    double W;
    // the one-sided end: a_{n-1} = x_{n-1} - x_{n-2}
    const double aul = s.u[4] - s.u[3], awl = s.w[4] - s.w[3];
    if (n == 3u) {  // x_0 .. x_2 are [2] .. [4]
        const double au0 = s.u[3] - s.u[2], aw0 = s.w[3] - s.w[2];
        const double au1 = (s.u[4] - s.u[2]) / 2.0, aw1 = (s.w[4] - s.w[2]) / 2.0;
        const double q0 = tm_sq2(au1 - au0, aw1 - aw0);
        const double q1 = tm_sq2((aul - au0) / 2.0, (awl - aw0) / 2.0);
        const double q2 = tm_sq2(aul - au1, awl - aw1);
        W = ((q0 + 4.0 * q1) + q2) / 3.0;
    } else {
        // a_{n-2} and a_{n-3} are central (n >= 4)
        const double au2 = (s.u[4] - s.u[2]) / 2.0, aw2 = (s.w[4] - s.w[2]) / 2.0;
        const double au3 = (s.u[3] - s.u[1]) / 2.0, aw3 = (s.w[3] - s.w[1]) / 2.0;
        const double qa = tm_sq2((aul - au3) / 2.0, (awl - aw3) / 2.0);  // q_{n-2}
        const double qb = tm_sq2(aul - au2, awl - aw2);                  // q_{n-1}
        if (n & 1u) {  // Simpson over all n points
            const double O = s.s_odd + qa, E = s.s_even + s.hold;
            W = (((s.q0 + 4.0 * O) + 2.0 * E) + qb) / 3.0;
        } else {       // Simpson over q_0 .. q_{n-2}, and the last interval by the three-point correction
            const double O = n == 4u ? s.s_odd : s.s_odd + s.hold;
            const double qc = n == 4u ? s.s_odd : s.hold;            // q_{n-3}
            const double simpson = (((s.q0 + 4.0 * O) + 2.0 * s.s_even) + qa) / 3.0;
            const double last = ((5.0 / 12.0) * qb + (2.0 / 3.0) * qa) - (1.0 / 12.0) * qc;
            W = simpson + last;
        }
    }
    const double T = (double)(n - 1u);
    o.dimensionless_jerk = (((T * T) * T) * W) / s.vmax2;
    o.flags |= TRACK_METRICS_JERK_VALID;
    return o;
}

}  // namespace mgx

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
