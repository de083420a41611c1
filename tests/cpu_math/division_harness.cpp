// Test-only host build of gbp_math.h: the short forms of the divisions by invariant divisors against the plain divisions they
// replace, bit for bit.  The `old_*` functions are the forms the library had before (kept here, not in the product).
// Every check returns the number of disagreements (0 = pass).
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../magics_amd/csrc/gbp_math.h"

namespace {

struct Rng {  // xorshift64*
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint64_t next() {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    double bits() {  // every exponent (zeros, denormals, inf, NaN included) equally likely
        const uint64_t u = next();
        double d;
        std::memcpy(&d, &u, 8);
        return d;
    }
    double unit() { return (double)(next() >> 11) * 0x1p-53; }
    double uniform(double a, double b) { return a + (b - a) * unit(); }
};

bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
// whole messages: the same bits, or a NaN in both.  (Which payload and sign a NaN carries out of an operation on TWO NaNs, or out
// of an invalid operation next to one, depends on the operand order the compiler picked for a commutative instruction — it differs
// between two compilations of the SAME source, so it cannot be held against the new form.  The quotients themselves are
// compared with `same`, NaNs included.)
template <int N>
bool same_message(const double (&a)[N], const double (&b)[N]) {
    for (int i = 0; i < N; i++)
        if (!same(a[i], b[i]) && !(a[i] != a[i] && b[i] != b[i])) return false;
    return true;
}
double from_bits(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
double ulp_step(double v, int k) { return from_bits(mgx::f64_bits(v) + (uint64_t)(int64_t)k); }

long check_one(double a, double b, double y) { return same(mgx::divide_by_invariant(a, b, y), a / b) ? 0 : 1; }

long directed(double b, double y) {
    long bad = 0;
    const double specials[] = {0.0, -0.0, 0x1p-1022, -0x1p-1022, 0x1.fffffffffffffp1023, -0x1.fffffffffffffp1023, 0x1p-1074, -0x1p-1074,
                               0x1.8p-1060, 0x0.fffffffffffffp-1022, 1.0 / 0.0, -1.0 / 0.0, from_bits(0x7ff8000000000000ull),
                               from_bits(0xfff8000000000001ull), from_bits(0x7ff0000000000001ull), 1.0, -1.0};
    for (double a : specials) bad += check_one(a, b, y);
    for (int k = 1; k <= 64; k++)
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            const double m = sgn * (double)k * b;  // small multiples of the divisor, and one ulp either side
            for (int d = -1; d <= 1; d++) bad += check_one(ulp_step(m, d), b, y);
        }
    for (int e = -1070; e <= 1020; e += 7) {  // the divisor scaled through every binade region, one ulp either side
        const double m = std::ldexp(b, e);
        for (int d = -1; d <= 1; d++) bad += check_one(ulp_step(m, d), b, y);
    }
    return bad;
}

long random_numerators(double b, double y, uint64_t seed, long n) {
    Rng g(seed);
    long bad = 0;
    for (long i = 0; i < n; i++) bad += check_one(g.bits(), b, y);
    return bad;
}

// ---- the forms before ----
double old_sdf_value(uint8_t red) { return 1.0 - (double)red / 255.0; }
void old_obstacle_message(const double (&h)[4], double delta, double inv_sigma2, const double (&x0)[4], double (&eta)[4], double (&lam)[16]) {
    double J[4];
    J[0] = (h[1] - h[0]) / delta;
    J[1] = (h[2] - h[0]) / delta;
    J[2] = (h[3] - h[0]) / delta;
    J[3] = (h[3] - h[0]) / delta;
    double jl[4];
    for (int i = 0; i < 4; i++) jl[i] = J[i] * inv_sigma2;
    const double jx = ((J[0] * x0[0] + J[1] * x0[1]) + J[2] * x0[2]) + J[3] * x0[3];
    const double rhs = jx + (0.0 - h[0]);
    for (int i = 0; i < 4; i++) {
        eta[i] = jl[i] * rhs;
        for (int j = 0; j < 4; j++) lam[i * 4 + j] = jl[i] * J[j];
    }
}
// the factor's quotients and everything in front of the Schur complement, as they were; the rest of both functions is unchanged
// and shared (mgx::schur4 for the dense form), so the old message is rebuilt from the old quotients
struct OldIr {
    bool skip;
    double h0, jl0, jl1, jh0, jh1;
};
OldIr old_ir_front(const double (&x_lo)[4], const double (&x_hi)[4], double d_safe, double tiny_offset) {
    OldIr o{false, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double dx = x_lo[0] - x_hi[0], dy = x_lo[1] - x_hi[1];
    if (dx * dx + dy * dy >= d_safe * d_safe) { o.skip = true; return o; }
    const double d0 = dx + tiny_offset, d1 = dy + tiny_offset;
    const double r = std::sqrt(d0 * d0 + d1 * d1);
    if (r <= d_safe) {
        o.h0 = 1.0 * (1.0 - r / d_safe);
        const double cl = -1.0 / d_safe / r, ch = 1.0 / d_safe / r;
        o.jl0 = cl * d0; o.jl1 = cl * d1; o.jh0 = ch * d0; o.jh1 = ch * d1;
    }
    return o;
}
bool old_interrobot_message(const double (&x_lo)[4], const double (&x_hi)[4], double d_safe, double tiny_offset, double inv_sigma2,
                            int dst_slot, const double (&eo)[4], const double (&lo)[16], double (&out_eta)[4], double (&out_lam)[16]) {
    const OldIr f = old_ir_front(x_lo, x_hi, d_safe, tiny_offset);
    if (f.skip) return false;
    const double jl0 = f.jl0, jl1 = f.jl1, jh0 = f.jh0, jh1 = f.jh1, h0 = f.h0;
    const double jx = (jl0 * x_lo[0] + jh0 * x_hi[0]) + (jl1 * x_lo[1] + jh1 * x_hi[1]);
    const double rhs = jx + (0.0 - h0);
    const double ja0 = dst_slot ? jh0 : jl0, ja1 = dst_slot ? jh1 : jl1;
    const double jb0 = dst_slot ? jl0 : jh0, jb1 = dst_slot ? jl1 : jh1;
    const double wa0 = ja0 * inv_sigma2, wa1 = ja1 * inv_sigma2;
    const double wb0 = jb0 * inv_sigma2, wb1 = jb1 * inv_sigma2;
    double laa[16], lab[16], lba[16], lbb[16], ea[4], eb[4];
    for (int i = 0; i < 16; i++) { laa[i] = 0.0; lab[i] = 0.0; lba[i] = 0.0; lbb[i] = lo[i]; }
    laa[0] = wa0 * ja0; laa[1] = wa0 * ja1; laa[4] = wa1 * ja0; laa[5] = wa1 * ja1;
    lab[0] = wa0 * jb0; lab[1] = wa0 * jb1; lab[4] = wa1 * jb0; lab[5] = wa1 * jb1;
    lba[0] = wb0 * ja0; lba[1] = wb0 * ja1; lba[4] = wb1 * ja0; lba[5] = wb1 * ja1;
    lbb[0] = wb0 * jb0 + lo[0]; lbb[1] = wb0 * jb1 + lo[1]; lbb[4] = wb1 * jb0 + lo[4]; lbb[5] = wb1 * jb1 + lo[5];
    ea[0] = wa0 * rhs; ea[1] = wa1 * rhs; ea[2] = 0.0; ea[3] = 0.0;
    eb[0] = wb0 * rhs + eo[0]; eb[1] = wb1 * rhs + eo[1]; eb[2] = eo[2]; eb[3] = eo[3];
    return mgx::schur4(laa, lab, lba, lbb, ea, eb, out_eta, out_lam);
}
bool old_interrobot_message_compact(const double (&x_lo)[4], const double (&x_hi)[4], double d_safe, double tiny_offset, double inv_sigma2,
                                    int dst_slot, const double (&eo)[4], const double (&lo)[16], double (&out)[6]) {
    using namespace mgx;
    const OldIr f = old_ir_front(x_lo, x_hi, d_safe, tiny_offset);
    if (f.skip) return false;
    const double jl0 = f.jl0, jl1 = f.jl1, jh0 = f.jh0, jh1 = f.jh1, h0 = f.h0;
    const double jx = (jl0 * x_lo[0] + jh0 * x_hi[0]) + (jl1 * x_lo[1] + jh1 * x_hi[1]);
    const double rhs = jx + (0.0 - h0);
    const double ja0 = dst_slot ? jh0 : jl0, ja1 = dst_slot ? jh1 : jl1;
    const double jb0 = dst_slot ? jl0 : jh0, jb1 = dst_slot ? jl1 : jh1;
    const double wa0 = ja0 * inv_sigma2, wa1 = ja1 * inv_sigma2;
    const double wb0 = jb0 * inv_sigma2, wb1 = jb1 * inv_sigma2;
    double lbb[16];
    for (int i = 0; i < 16; i++) lbb[i] = lo[i];
    lbb[0] = wb0 * jb0 + lo[0]; lbb[1] = wb0 * jb1 + lo[1]; lbb[4] = wb1 * jb0 + lo[4]; lbb[5] = wb1 * jb1 + lo[5];
    double cf0[4], c0[4], c1[4];
    {
        const double r0[4] = {lbb[0], lbb[1], lbb[2], lbb[3]}, r1[4] = {lbb[4], lbb[5], lbb[6], lbb[7]};
        const double r2[4] = {lbb[8], lbb[9], lbb[10], lbb[11]}, r3[4] = {lbb[12], lbb[13], lbb[14], lbb[15]};
        double mn[4];
        minors_of_removed_row(r1, r2, r3, mn);
        cofactors_from_minors(0, mn, cf0);
        c0[0] = cf0[0]; c1[0] = cf0[1];
        double m2[2];
        minors_of_removed_row_first2(r0, r2, r3, m2);
        c0[1] = -m2[0]; c1[1] = m2[1];
        minors_of_removed_row_first2(r0, r1, r3, m2);
        c0[2] = m2[0]; c1[2] = -m2[1];
        minors_of_removed_row_first2(r0, r1, r2, m2);
        c0[3] = -m2[0]; c1[3] = m2[1];
        const double det = det_from_row0(r0, cf0);
        if (det == 0.0) return false;
        const double id = 1.0 / det;
        for (int i = 0; i < 4; i++) { c0[i] = c0[i] * id; c1[i] = c1[i] * id; }
    }
    const double lab00 = wa0 * jb0, lab01 = wa0 * jb1, lab10 = wa1 * jb0, lab11 = wa1 * jb1;
    double t0[4], t1[4];
    for (int c = 0; c < 4; c++) {
        t0[c] = lab00 * c0[c] + lab01 * c1[c];
        t1[c] = lab10 * c0[c] + lab11 * c1[c];
    }
    const double eb0 = wb0 * rhs + eo[0], eb1 = wb1 * rhs + eo[1];
    out[0] = wa0 * rhs - (((t0[0] * eb0 + t0[1] * eb1) + t0[2] * eo[2]) + t0[3] * eo[3]);
    out[1] = wa1 * rhs - (((t1[0] * eb0 + t1[1] * eb1) + t1[2] * eo[2]) + t1[3] * eo[3]);
    const double lba00 = wb0 * ja0, lba01 = wb0 * ja1, lba10 = wb1 * ja0, lba11 = wb1 * ja1;
    out[2] = wa0 * ja0 - (t0[0] * lba00 + t0[1] * lba10);
    out[3] = wa0 * ja1 - (t0[0] * lba01 + t0[1] * lba11);
    out[4] = wa1 * ja0 - (t1[0] * lba00 + t1[1] * lba10);
    out[5] = wa1 * ja1 - (t1[0] * lba01 + t1[1] * lba11);
    return !(std::isinf(out[2]) || std::isinf(out[3]) || std::isinf(out[4]) || std::isinf(out[5]));
}

template <typename F>
long in_threads(int n_threads, F f) {  // f(thread index) -> disagreements
    std::vector<long> bad((size_t)n_threads, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; t++) th.emplace_back([&, t] { bad[(size_t)t] = f(t); });
    for (auto &x : th) x.join();
    long s = 0;
    for (long b : bad) s += b;
    return s;
}

double random_divisor(Rng &g, int i) {
    // three in four within the range that has a reciprocal, with random mantissas; the rest anywhere (denormals, huge, inf, NaN, 0)
    if (i % 4 == 3) return g.bits();
    const double m = 1.0 + g.unit();
    const int e = (int)(g.next() % 801) - 400;
    const double v = std::ldexp(m, e > 399 ? 399 : e);
    return (g.next() & 1) ? -v : v;
}

}  // namespace

extern "C" {

// red / 255 and sdf_value for all 256 values of a pixel
long d_check_255() {
    long bad = 0;
    for (int k = 0; k < 256; k++) {
        if (!same(mgx::divide3((double)k, 255.0, 1.0 / 255.0), (double)k / 255.0)) bad++;
        if (!same(mgx::sdf_value((uint8_t)k), old_sdf_value((uint8_t)k))) bad++;
    }
    return bad;
}

// divide_by_invariant(a, b, reciprocal_for_division(b)) against a / b: n random numerators (per thread) + the directed ones
long d_check_divisor(double b, uint64_t seed, long n, int n_threads) {
    const double y = mgx::reciprocal_for_division(b);
    long bad = directed(b, y);
    bad += in_threads(n_threads, [&](int t) { return random_numerators(b, y, seed * 1000 + (uint64_t)t, n / n_threads + 1); });
    return bad;
}
// how many of n random numerators take the short form for this divisor (the checks above are not all fall-backs)
long d_short_form_taken(double b, uint64_t seed, long n) {
    const double y = mgx::reciprocal_for_division(b);
    Rng g(seed);
    long taken = 0;
    for (long i = 0; i < n; i++) {
        const double q = g.bits() * y;
        const uint32_t ex = (uint32_t)(mgx::f64_bits(q) >> 52) & 0x7ffu;
        taken += (ex - 523u <= 1000u) ? 1 : 0;
    }
    return taken;
}
// n_div random divisors, the same numerator set (seed) for each
long d_check_random_divisors(uint64_t seed, int n_div, long n, int n_threads) {
    std::vector<double> bs;
    Rng g(seed ^ 0xabcdefull);
    for (int i = 0; i < n_div; i++) bs.push_back(random_divisor(g, i));
    return in_threads(n_threads, [&](int t) {
        long bad = 0;
        for (int i = t; i < n_div; i += n_threads) {
            const double y = mgx::reciprocal_for_division(bs[(size_t)i]);
            bad += directed(bs[(size_t)i], y) + random_numerators(bs[(size_t)i], y, seed, n);
        }
        return bad;
    });
}

// the obstacle Jacobian's quotient for one delta: what obstacle_inv_delta answers (returned through *inv), and obstacle_slope
// against the division for every pair of samples (0 outside the image included)
long d_check_obstacle_delta(double delta, double *inv) {
    const double y = mgx::obstacle_inv_delta(delta);
    *inv = y;
    long bad = 0;
    if (!(mgx::f64_bits(y) << 1)) return 0;  // no reciprocal: such a world is not committed, the kernels never see it
    for (int i = 0; i <= 256; i++)
        for (int j = 0; j <= 256; j++) {
            const double hi = i == 256 ? 0.0 : mgx::sdf_value((uint8_t)i), h0 = j == 256 ? 0.0 : mgx::sdf_value((uint8_t)j);
            if (!same(mgx::obstacle_slope(hi, h0, delta, y), (hi - h0) / delta)) bad++;
        }
    return bad;
}

// h0, cl, ch of the inter-robot factor: interrobot_slopes against the three expressions as they were written, random (d_safe, r)
long d_check_slopes(uint64_t seed, long n, int n_threads) {
    return in_threads(n_threads, [&](int t) {
        Rng g(seed * 77 + (uint64_t)t);
        long bad = 0;
        for (long i = 0; i < n / n_threads + 1; i++) {
            double d_safe, r;
            switch (i % 8) {
            case 0: d_safe = g.uniform(0.1, 10.0); r = 0.0; break;
            case 1: d_safe = g.uniform(0.1, 10.0); r = (i & 8) ? 1.0 / 0.0 : from_bits(0x7ff8000000000000ull | (g.next() >> 13)); break;
            case 2: d_safe = g.bits(); r = std::fabs(g.bits()); break;
            case 3: d_safe = std::fabs(g.bits()); r = (i & 8) ? 0.0 : d_safe * g.unit(); break;
            case 4: d_safe = (i & 8) ? 1.0 / 0.0 : 0.0; r = (i & 16) ? 0.0 : g.unit(); break;
            default: d_safe = g.uniform(0.01, 100.0); r = d_safe * g.unit(); break;
            }
            const double oh = 1.0 * (1.0 - r / d_safe), ocl = -1.0 / d_safe / r, och = 1.0 / d_safe / r;
            if (r <= d_safe) {  // the factor evaluates them under this test only (a NaN r or d_safe never gets here)
                double h0, cl, ch;
                mgx::interrobot_slopes(r, d_safe, mgx::reciprocal_for_division(d_safe), h0, cl, ch);
                if (!same(h0, oh) || !same(cl, ocl) || !same(ch, och)) bad++;
            }
            // the claim the short form rests on: wherever cl is a number, ch is its negation
            if (ocl == ocl && !same(och, -ocl)) bad++;
        }
        return bad;
    });
}

static void random_message(Rng &g, double (&eo)[4], double (&lo)[16], int kind) {
    double a[16];
    for (double &v : a) v = g.uniform(-1.0, 1.0);
    const double scale = kind == 1 ? 0.0 : std::ldexp(1.0, (int)(g.next() % 40) - 10);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += a[i * 4 + k] * a[j * 4 + k];
            lo[i * 4 + j] = s * scale;
        }
    for (double &v : eo) v = kind == 1 ? 0.0 : g.uniform(-100.0, 100.0);
    if (kind == 2) lo[g.next() % 16] = g.bits();
    if (kind == 3) eo[g.next() % 4] = g.bits();
}

// whole functions, old against new: interrobot_message (both signatures) and interrobot_message_compact
long d_check_interrobot(uint64_t seed, long n, int n_threads) {
    return in_threads(n_threads, [&](int t) {
        Rng g(seed * 131 + (uint64_t)t);
        long bad = 0;
        for (long i = 0; i < n / n_threads + 1; i++) {
            const int kind = (int)(i % 16);
            double d_safe = (i & 1) ? 2.5 : g.uniform(0.5, 8.0);
            double off = (kind == 5) ? 0.0 : 1e-6f * (double)(g.next() % 2000);
            double x_lo[4], x_hi[4], eo[4], lo[16];
            for (int c = 0; c < 4; c++) { x_lo[c] = g.uniform(-50.0, 50.0); x_hi[c] = x_lo[c] + g.uniform(-1.0, 1.0) * d_safe * 0.9; }
            if (kind == 5 || kind == 6) { x_hi[0] = x_lo[0]; x_hi[1] = x_lo[1]; }       // same position: r == 0 when the offset is 0
            if (kind == 7) { x_hi[0] = x_lo[0] + 3.0 * d_safe; }                        // outside the safety distance
            if (kind == 8) x_lo[g.next() % 2] = g.bits();                               // non-finite / extreme linearisation point
            if (kind == 9) d_safe = g.bits();
            if (kind == 10) { d_safe = 1.0 / 0.0; if (i & 16) { x_hi[0] = x_lo[0]; x_hi[1] = x_lo[1]; off = 0.0; } }
            if (kind == 11) { const double s = std::ldexp(1.0, -(int)(g.next() % 1000)); for (int c = 0; c < 2; c++) { x_lo[c] *= s; x_hi[c] *= s; } off = 0.0; d_safe *= (i & 16) ? s : 1.0; }
            random_message(g, eo, lo, kind == 12 ? 1 : (kind == 13 ? 2 : (kind == 14 ? 3 : 0)));
            const double inv_s2 = 1.0 / (0.005 * 0.005);
            for (int slot = 0; slot < 2; slot++) {
                double e0[4], l0[16], e1[4], l1[16], e2[4], l2[16], c0[6], c1[6];
                for (int c = 0; c < 4; c++) e0[c] = e1[c] = e2[c] = 0.0;
                for (int c = 0; c < 16; c++) l0[c] = l1[c] = l2[c] = 0.0;
                for (int c = 0; c < 6; c++) c0[c] = c1[c] = 0.0;
                const bool ok0 = old_interrobot_message(x_lo, x_hi, d_safe, off, inv_s2, slot, eo, lo, e0, l0);
                const bool ok1 = mgx::interrobot_message(x_lo, x_hi, d_safe, off, inv_s2, slot, eo, lo, e1, l1);
                const bool ok2 = mgx::interrobot_message(x_lo, x_hi, d_safe, mgx::reciprocal_for_division(d_safe), off, inv_s2, slot, eo, lo, e2, l2);
                const bool k0 = old_interrobot_message_compact(x_lo, x_hi, d_safe, off, inv_s2, slot, eo, lo, c0);
                const bool k1 = mgx::interrobot_message_compact(x_lo, x_hi, d_safe, mgx::reciprocal_for_division(d_safe), off, inv_s2, slot, eo, lo, c1);
                if (ok0 != ok1 || ok0 != ok2 || k0 != k1) { bad++; continue; }
                if (ok0 && !(same_message(e0, e1) && same_message(l0, l1) && same_message(e0, e2) && same_message(l0, l2))) bad++;
                if (k0 && !same_message(c0, c1)) bad++;
            }
        }
        return bad;
    });
}

// obstacle_message and obstacle_message_row, with the checked reciprocal and with none, against the old form
long d_check_obstacle(double delta, uint64_t seed, long n) {
    Rng g(seed);
    const double y = mgx::obstacle_inv_delta(delta);
    long bad = 0;
    for (long i = 0; i < n; i++) {
        double h[4], x0[4];
        for (int q = 0; q < 4; q++) {
            const uint64_t k = g.next() % 300;  // 256 and above: outside the image
            h[q] = k >= 256 ? 0.0 : mgx::sdf_value((uint8_t)k);
            if (i % 5 == 0 && q) h[q] = h[0];                      // flat neighbourhood: zero numerators
            if (i % 7 == 0) h[q] = (g.next() & 1) ? 1.0 : 0.0;     // red = 0 / red = 255
        }
        for (double &v : x0) v = (i % 11 == 0) ? g.bits() : g.uniform(-100.0, 100.0);
        const double inv_s2 = 1.0 / (0.005 * 0.005);
        double e0[4], l0[16];
        old_obstacle_message(h, delta, inv_s2, x0, e0, l0);
        for (int form = 0; form < 3; form++) {
            double e1[4], l1[16];
            if (form != 1 && !(mgx::f64_bits(y) << 1)) continue;  // the reciprocal forms need one
            if (form == 0) mgx::obstacle_message(h, delta, y, inv_s2, x0, e1, l1);
            else if (form == 1) mgx::obstacle_message(h, delta, inv_s2, x0, e1, l1);
            else
                for (int q = 0; q < 4; q++) {
                    double lam_q[4];
                    mgx::obstacle_message_row(h, delta, y, inv_s2, x0, q, e1[q], lam_q);
                    for (int c = 0; c < 4; c++) l1[q * 4 + c] = lam_q[c];
                }
            if (!(same_message(e0, e1) && same_message(l0, l1))) bad++;
        }
    }
    return bad;
}

}  // extern "C"
