"""Run metrics per robot: smoothness as Log Dimensionless Jerk (the reference's scripts/ldj.py:17-55) and perpendicular path
deviation (scripts/perpendicular-path-deviation.py:40-60, 99-115), as include/mgx.h specifies them ("run metrics on the device").

Three forms:
  * `Stream`: the streaming form, operation by operation what magics_amd/csrc/mgx_track_metrics.h does — the device's checker, equal
    to it as f64 bit patterns.  Python floats are f64 and every operator rounds once, `math.sqrt` is correctly rounded.
  * `dimensionless_jerk` / `deviations`: the plain batch forms over whole series (numpy), the specification's formulas written down
    once more without any state — the streaming form's own checker, up to rounding.
  * `summary`: the per-run figures the reference prints (`statistics` module, ldj.py:107-125).

The times cancel out of the jerk integral: ldj.py differentiates with dt = the mean spacing of the time stamps and integrates over
linspace(t_0, t_{n-1}, n), whose spacing is the same dt, so T^3 / vmax^2 * integral = (n - 1)^3 * W / vmax2 with W the Simpson sum of
the squared second differences at unit spacing."""
import math
import statistics

import numpy as np

JERK_VALID, DEVIATION_VALID = 1, 2
NAN = float("nan")
_C512, _C23, _C112 = 5.0 / 12.0, 2.0 / 3.0, 1.0 / 12.0


def _sq2(a, b):
    a2, b2 = a * a, b * b
    return a2 + b2


class Stream:
    """one robot's state (mgx_track_metrics.h, TrackMetricsState): `velocity` and `position` take a sample's figures, `read`
    finalises a copy — reading changes nothing"""

    __slots__ = ("u", "w", "q0", "s_odd", "s_even", "hold", "vmax2", "dev_sum", "dev_max", "n_vel", "n_pos", "n_unrouted")

    def __init__(self):
        self.u, self.w = [0.0] * 5, [0.0] * 5
        self.q0 = self.s_odd = self.s_even = self.hold = self.vmax2 = self.dev_sum = self.dev_max = 0.0
        self.n_vel = self.n_pos = self.n_unrouted = 0

    def velocity(self, u, w):
        u, w = float(u), float(w)
        m = self.n_vel
        self.u = self.u[1:] + [u]
        self.w = self.w[1:] + [w]
        v2 = _sq2(u, w)
        self.vmax2 = v2 if v2 > self.vmax2 else self.vmax2
        self.n_vel = m + 1
        U, W = self.u, self.w
        if m == 3:
            au0, aw0 = U[2] - U[1], W[2] - W[1]
            au1, aw1 = (U[3] - U[1]) / 2.0, (W[3] - W[1]) / 2.0
            au2, aw2 = (U[4] - U[2]) / 2.0, (W[4] - W[2]) / 2.0
            self.q0 = _sq2(au1 - au0, aw1 - aw0)
            self.s_odd = _sq2((au2 - au0) / 2.0, (aw2 - aw0) / 2.0)
        elif m >= 4:
            aup, awp = (U[4] - U[2]) / 2.0, (W[4] - W[2]) / 2.0
            aum, awm = (U[2] - U[0]) / 2.0, (W[2] - W[0]) / 2.0
            q = _sq2((aup - aum) / 2.0, (awp - awm) / 2.0)
            if m >= 5:
                if (m - 3) & 1:
                    self.s_odd = self.s_odd + self.hold
                else:
                    self.s_even = self.s_even + self.hold
            self.hold = q

    def position(self, px, py, route):
        """route: a sequence of (x, y), or None"""
        px, py = float(px), float(py)
        found, best = False, 0.0
        pts = [] if route is None else route
        for k in range(len(pts) - 1):
            ax, ay = float(pts[k][0]), float(pts[k][1])
            dx, dy = float(pts[k + 1][0]) - ax, float(pts[k + 1][1]) - ay
            l2 = _sq2(dx, dy)
            if not l2 > 0.0:
                continue
            c1, c2 = dx * (py - ay), dy * (px - ax)
            d = abs(c1 - c2) / math.sqrt(l2)
            if not found or d < best:
                best = d
            found = True
        if not found:
            self.n_unrouted += 1
            return
        self.dev_sum = self.dev_sum + best
        self.dev_max = best if best > self.dev_max else self.dev_max
        self.n_pos += 1

    def read(self):
        """the record of mgx_track_metrics_read as a dict"""
        n, U, W = self.n_vel, self.u, self.w
        out = {"n_positions": self.n_pos, "n_velocities": n, "n_unrouted": self.n_unrouted, "flags": DEVIATION_VALID if self.n_pos else 0,
               "dimensionless_jerk": NAN, "vmax2": self.vmax2, "deviation_sum": self.dev_sum, "deviation_max": self.dev_max}
        if n < 3 or not self.vmax2 > 0.0:
            return out
        aul, awl = U[4] - U[3], W[4] - W[3]
        if n == 3:
            au0, aw0 = U[3] - U[2], W[3] - W[2]
            au1, aw1 = (U[4] - U[2]) / 2.0, (W[4] - W[2]) / 2.0
            q0 = _sq2(au1 - au0, aw1 - aw0)
            q1 = _sq2((aul - au0) / 2.0, (awl - aw0) / 2.0)
            q2 = _sq2(aul - au1, awl - aw1)
            Wq = ((q0 + 4.0 * q1) + q2) / 3.0
        else:
            au2, aw2 = (U[4] - U[2]) / 2.0, (W[4] - W[2]) / 2.0
            au3, aw3 = (U[3] - U[1]) / 2.0, (W[3] - W[1]) / 2.0
            qa = _sq2((aul - au3) / 2.0, (awl - aw3) / 2.0)
            qb = _sq2(aul - au2, awl - aw2)
            if n & 1:
                O, E = self.s_odd + qa, self.s_even + self.hold
                Wq = (((self.q0 + 4.0 * O) + 2.0 * E) + qb) / 3.0
            else:
                O = self.s_odd if n == 4 else self.s_odd + self.hold
                qc = self.s_odd if n == 4 else self.hold
                simpson = (((self.q0 + 4.0 * O) + 2.0 * self.s_even) + qa) / 3.0
                last = (_C512 * qb + _C23 * qa) - _C112 * qc
                Wq = simpson + last
        T = float(n - 1)
        out["dimensionless_jerk"] = (((T * T) * T) * Wq) / self.vmax2
        out["flags"] |= JERK_VALID
        return out


def stream(velocities_uw=(), positions_xy=(), route=None):
    """the streaming form over whole series: the record after everything has been taken"""
    s = Stream()
    for u, w in velocities_uw:
        s.velocity(u, w)
    for x, y in positions_xy:
        s.position(x, y, route)
    return s.read()


# ---- the batch forms ------------------------------------------------------------------------------------------------------------
def simpson_unit(q):
    """composite Simpson sum at unit spacing under scipy.integrate.simpson's rule (>= 1.11): an even number of points takes the
    last interval by the three-point correction"""
    q = np.asarray(q, dtype=np.float64)
    n = len(q)
    if n < 3:
        raise ValueError("three points at least")
    if n % 2 == 0:
        return simpson_unit(q[:-1]) + (5.0 / 12.0 * q[-1] + 2.0 / 3.0 * q[-2] - 1.0 / 12.0 * q[-3])
    return (q[0] + 4.0 * q[1:-1:2].sum() + 2.0 * q[2:-1:2].sum() + q[-1]) / 3.0


def dimensionless_jerk(velocities_uw):
    """DJ of a velocity series [n, 2]; NaN for n < 3 or a series that never moves"""
    v = np.asarray(velocities_uw, dtype=np.float64).reshape(-1, 2)
    n = len(v)
    vmax2 = float((v[:, 0] ** 2 + v[:, 1] ** 2).max()) if n else 0.0
    if n < 3 or not vmax2 > 0.0:
        return NAN
    ju, jw = np.gradient(np.gradient(v[:, 0])), np.gradient(np.gradient(v[:, 1]))
    return float((n - 1) ** 3 * simpson_unit(ju ** 2 + jw ** 2) / vmax2)


def ldj(dj):
    """Log Dimensionless Jerk of a dimensionless jerk (the device has no logarithm): NaN stays NaN, DJ = 0 gives +inf"""
    dj = float(dj)
    if math.isnan(dj):
        return NAN
    return math.inf if dj == 0.0 else -math.log(dj)


def deviations(positions_xy, route):
    """the distance of every position [n, 2] to the nearest of the infinite lines through consecutive route points, segments of
    zero length left out; None when no segment is left"""
    p = np.asarray(positions_xy, dtype=np.float64).reshape(-1, 2)
    r = np.zeros((0, 2)) if route is None else np.asarray(route, dtype=np.float64).reshape(-1, 2)
    a, d = r[:-1], r[1:] - r[:-1]
    keep = (d ** 2).sum(axis=1) > 0.0
    a, d = a[keep], d[keep]
    if not len(a):
        return None
    cross = d[None, :, 0] * (p[:, None, 1] - a[None, :, 1]) - d[None, :, 1] * (p[:, None, 0] - a[None, :, 0])
    return (np.abs(cross) / np.sqrt((d ** 2).sum(axis=1))[None, :]).min(axis=1)


def path_deviation(dev_sum, n_positions):
    """the reference's "RMSE": sqrt(sum of the distances / n) (sic, perpendicular-path-deviation.py:114-115)"""
    return math.sqrt(dev_sum / n_positions) if n_positions else NAN


def robot_metrics(record):
    """{ldj, path_deviation, mean_deviation, max_deviation} of one record (a dict as Stream.read makes it, or a row of
    World.track_metrics_read)"""
    n = int(record["n_positions"])
    s = float(record["deviation_sum"])
    return {"ldj": ldj(record["dimensionless_jerk"]), "path_deviation": path_deviation(s, n), "mean_deviation": s / n if n else NAN,
            "max_deviation": float(record["deviation_max"]) if n else NAN}


def summary(values):
    """robots, mean, median, largest, smallest, variance, stdev with the `statistics` module's meaning (ldj.py:107-125) over the
    values that are numbers; variance and stdev need two"""
    v = [float(x) for x in values if x is not None and not math.isnan(float(x))]
    out = {"robots": len(v), "mean": NAN, "median": NAN, "largest": NAN, "smallest": NAN, "variance": NAN, "stdev": NAN}
    if v:
        out.update(mean=statistics.mean(v), median=statistics.median(v), largest=max(v), smallest=min(v))
    if len(v) >= 2:
        out.update(variance=statistics.variance(v), stdev=statistics.stdev(v))
    return out
