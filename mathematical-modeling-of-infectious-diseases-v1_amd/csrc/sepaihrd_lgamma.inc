// csrc/sepaihrd_lgamma.inc -- log Gamma(x) for x > 0 as ONE explicit operation sequence for host and device, in the manner of
// glibc_log (csrc/sepaihrd_rng.inc), on whose constants and table path it is built.  The negative-binomial likelihood of the
// deterministic objective (DESIGN.md section 6o) needs g(obs, k) = lgamma(obs + k) - lgamma(k) - obs log(k) with a k that differs
// from chain to chain, so it cannot come from the host as the particle filters' row constants do
// (csrc/sepaihrd_particle_nb_host.h: glibc's lgamma).
//
//   x >= 16:  Stirling's series  (x - 1/2) log x - x + log(2 pi) / 2 + 1/(12 x) - 1/(360 x^3) + 1/(1260 x^5) - 1/(1680 x^7) + 1/(1188 x^9)
//             (the first term left out, 691 / (360360 x^11), is below 1.1e-16 at x = 16);
//   x <  16:  the recurrence Gamma(x + m) = x (x + 1) ... (x + m - 1) Gamma(x) with the smallest m that brings x + m to 16 or beyond:
//             lgamma(x) = stirling(x + m) - log(x (x + 1) ... (x + m - 1)), one log of the product (at most 16 factors, below 1.4e12).
//
// The value is kept in TWO parts, hi + lo (lgamma_parts).  At k = 1e6 lgamma is 1.3e7, one ulp of which is 1.9e-9: a difference
// of two lgammas ROUNDED to doubles is off by up to that, more than the whole likelihood cell may be (1e-9 of a value near 1).
// So the leading term (x - 1/2) log x - x is formed from the two parts glibc's log ends with (log_parts: its last operation is
// their sum), the product's rounding error recovered by one fma and the subtraction's by Knuth's two-sum; the caller subtracts
// hi from hi (exact for neighbours) and lo from lo.  lgamma_pos(x) = hi + lo is the value as one double.
// Domain: x in [1e-3, 1e6 + the largest observation]; a NaN gives NaN.  Accuracy of lgamma_pos: what limits it is the
// cancellation of the shifted branch, a few ulp of stirling(16 ..) ~ 30; tests/test_nb_objective_cpu.py states the measured worst
// case against glibc's lgamma.  Only correctly rounded IEEE operations, an fma only where written: every includer compiles with
// contraction off, and host and device then produce the same bits.
// Included by csrc/sepaihrd_nb_objective.inc.
#pragma once
#include "sepaihrd_rng.inc"

namespace sepaihrd_lgamma {

using sepaihrd_rng::as_f64;
using sepaihrd_rng::as_u64;
using sepaihrd_rng::glibc_log;

constexpr double SHIFT_TO = 16.0;
constexpr double HALF_LOG_2PI = 0x1.d67f1c864beb5p-1;  // 0.91893853320467274178

struct Parts {
    double hi, lo;
};

// glibc_log's table path (csrc/sepaihrd_rng.inc, the same operations on the same constants) with its last addition left
// undone: log(x) = hi + lo to about 2^-58 relative.  For normal x outside glibc's near-one window; here x >= 16.
SEP_RNG_FN Parts log_parts(const double x) {
#include "sepaihrd_glibc_log.inc"
    (void)GLOG_B;  // the coefficients of glibc's near-one branch, which this path does not take
    const uint64_t ix = as_u64(x);
    const uint64_t tmp = ix - 0x3fe6000000000000ULL;
    const int i = (int)((tmp >> 45) & 127);
    const int k = (int)((int64_t)tmp >> 52);
    const uint64_t iz = ix - (tmp & (0xfffULL << 52));
    const double invc = GLOG_T[i][0], logc = GLOG_T[i][1], z = as_f64(iz);
    const double r = __builtin_fma(z, invc, -1.0);
    const double kd = (double)k;
    const double w = __builtin_fma(kd, GLOG_LN2HI, logc);
    const double hi = r + w;
    const double t39 = (w - hi) + r;
    const double lo = __builtin_fma(kd, GLOG_LN2LO, t39);
    const double r2 = r * r;
    const double t42 = __builtin_fma(r2, GLOG_A[0], lo);
    const double t43 = r * r2;
    const double t45 = __builtin_fma(r, GLOG_A[2], GLOG_A[1]);
    const double t47 = __builtin_fma(r, GLOG_A[4], GLOG_A[3]);
    const double t49 = __builtin_fma(t47, r2, t45);
    Parts p;
    p.hi = hi;
    p.lo = __builtin_fma(t43, t49, t42);
    return p;
}

// x >= SHIFT_TO
SEP_RNG_FN Parts stirling_parts(double x) {
    const double r = 1.0 / x;
    const double w = r * r;
    double s = 1.0 / 1188.0;
    s = s * w - 1.0 / 1680.0;
    s = s * w + 1.0 / 1260.0;
    s = s * w - 1.0 / 360.0;
    s = s * w + 1.0 / 12.0;
    const double tail = HALF_LOG_2PI + s * r;
    const Parts L = log_parts(x);
    const double a = x - 0.5;                      // exact
    const double ph = a * L.hi;
    const double pe = __builtin_fma(a, L.hi, -ph);  // a L.hi = ph + pe exactly
    const double pl = pe + a * L.lo;
    const double sh = ph - x;                      // two-sum of ph + (-x)
    const double bb = sh - ph;
    const double se = (ph - (sh - bb)) + (-x - bb);
    Parts out;
    out.hi = sh;
    out.lo = (se + pl) + tail;
    return out;
}

SEP_RNG_FN Parts lgamma_parts(double x) {
    if (x >= SHIFT_TO) return stirling_parts(x);
    double p = 1.0, y = x;
    for (int m = 0; m < 16 && y < SHIFT_TO; ++m) {  // x > 0 needs at most 16 factors; the bound ends the walk for any other input
        p *= y;
        y += 1.0;
    }
    if (!(y >= SHIFT_TO)) {  // NaN, or not positive: outside the domain
        Parts bad;
        bad.hi = bad.lo = __builtin_nan("");
        return bad;
    }
    Parts out = stirling_parts(y);
    out.lo -= glibc_log(p);
    return out;
}

SEP_RNG_FN double lgamma_pos(double x) {
    const Parts v = lgamma_parts(x);
    return v.hi + v.lo;
}

// lgamma(a) - lgamma(b) from the parts: hi from hi, lo from lo
SEP_RNG_FN double lgamma_difference(const Parts& a, const Parts& b) { return (a.hi - b.hi) + (a.lo - b.lo); }

}  // namespace sepaihrd_lgamma
