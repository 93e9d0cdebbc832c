// csrc/sepaihrd_poisson.inc -- a Poisson sampler as one text for host and device, on the counter-based stream of
// csrc/sepaihrd_stoch.inc (Philox-4x32-10, uniform_open, log_factorial, glibc_log / glibc_exp).
//
// A variate is a pure function of (seed, c0, c1, c2, lambda):
//     key     = (seed low word, seed high word)
//     counter = (c0, c1, c2, attempt)
// One Philox block serves one ATTEMPT: words (0, 1) give u, words (2, 3) give v.  The variate is returned as a double, so
// there is no integer range limit.  lambda <= 0 (minus infinity included): 0; NaN or plus infinity: NaN.
//   * lambda < 10: inversion by sequential search from 0, r = exp(-lambda), while u > r: u -= r, ++x, r *= lambda / x; a
//     search past 110 (probability < 1e-60 at lambda < 10) draws again with the next attempt, as BINV is guarded;
//   * lambda >= 10: Hoermann's transformed rejection with squeeze, PTRS (PAPERS.md), everything in double.
// Every log / exp is glibc_log / glibc_exp, every other operation a correctly rounded IEEE one, an fma only where written
// (both sides compile with contraction off): the host twin and the device agree bit for bit.
// Included by csrc/sepaihrd_predictive.hip (the probe), through csrc/sepaihrd_nb_draw.inc by the draw kernels, and by the host library (host/src/HipPosteriorPredictive.cpp).
#pragma once
#include "sepaihrd_stoch.inc"

namespace sepaihrd_poisson {

using sepaihrd_stoch::glibc_exp;
using sepaihrd_stoch::glibc_log;
using sepaihrd_stoch::log_factorial;
using sepaihrd_stoch::philox4x32_10;
using sepaihrd_stoch::uniform_open;

constexpr double INVERSION_BELOW = 10.0;  // PTRS needs lambda >= 10
constexpr int INVERSION_RESTART = 110;

SEP_RNG_FN void attempt_uniforms(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t attempt, double& u, double& v) {
    const sepaihrd_stoch::Philox b = philox4x32_10(c0, c1, c2, attempt, (uint32_t)seed, (uint32_t)(seed >> 32));
    u = uniform_open(b.w[0], b.w[1]);
    v = uniform_open(b.w[2], b.w[3]);
}

SEP_RNG_FN double poisson(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, double lambda) {
    if (lambda != lambda) return lambda;
    if (!(lambda > 0.0)) return 0.0;
    if (lambda > 0x1.fffffffffffffp+1023) return __builtin_nan("");
    double u, v;
    if (lambda < INVERSION_BELOW) {
        const double r0 = glibc_exp(-lambda);
        for (uint32_t attempt = 0;; ++attempt) {
            attempt_uniforms(seed, c0, c1, c2, attempt, u, v);
            double r = r0;
            int x = 0;
            while (u > r) {
                u -= r;
                ++x;
                if (x > INVERSION_RESTART) break;
                r *= lambda / (double)x;
            }
            if (x <= INVERSION_RESTART) return (double)x;
        }
    }
    const double b = 0.931 + 2.53 * __builtin_sqrt(lambda);
    const double a = -0.059 + 0.02483 * b;
    const double log_inv_alpha = glibc_log(1.1239 + 1.1328 / (b - 3.4));
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    const double log_lambda = glibc_log(lambda);
    for (uint32_t attempt = 0;; ++attempt) {
        attempt_uniforms(seed, c0, c1, c2, attempt, u, v);
        const double U = u - 0.5;
        const double us = 0.5 - __builtin_fabs(U);
        const double k = __builtin_floor((2.0 * a / us + b) * U + lambda + 0.43);
        if (us >= 0.07 && v <= vr) return k;
        if (k < 0.0 || (us < 0.013 && v > us)) continue;
        if (glibc_log(v) + log_inv_alpha - glibc_log(a / (us * us) + b) <= -lambda + k * log_lambda - log_factorial(k)) return k;
    }
}

// mid-PIT of an observation among n_draws draws, `less` of them below and `equal` of them at the observation
SEP_RNG_FN double mid_pit(int64_t less, int64_t equal, int64_t n_draws) {
    return n_draws > 0 ? ((double)less + 0.5 * (double)equal) / (double)n_draws : __builtin_nan("");
}

}  // namespace sepaihrd_poisson
