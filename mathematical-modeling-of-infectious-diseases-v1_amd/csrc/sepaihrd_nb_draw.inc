// csrc/sepaihrd_nb_draw.inc -- a gamma sampler and the negative-binomial variate built on it, as one text for host and device
// (DESIGN.md section 6p), on the counter-based stream of csrc/sepaihrd_poisson.inc.
//
// A negative-binomial count with mean mu and dispersion k (variance mu + mu^2 / k) is a gamma-Poisson mixture:
//     G ~ Gamma(shape k, scale 1),   y ~ Poisson(mu G / k).
// Both variates are pure functions of (seed, c0, c1, c2) and their parameters.  The Poisson draw keeps the coordinates of
// csrc/sepaihrd_poisson.inc, counter (c0, c1, c2, attempt) with attempt counted from 0; the gamma draw of the same cell takes the
// upper half of the fourth counter word, so no uniform serves both:
//     gamma attempt i    counter (c0, c1, c2, 0x80000000 + i)   words (0, 1) give u1, words (2, 3) give u2
//     boost uniform U    counter (c0, c1, c2, 0xC0000000)       words (0, 1)
//   * shape a >= 1: Cheng's rejection from the log-logistic envelope, algorithm GB (Cheng 1977, PAPERS.md; what CPython's
//     random.gammavariate runs above 1): ainv = sqrt(2 a - 1), b = a - log 4, c = a + ainv, formed once; per attempt
//     v = log(u1 / (1 - u1)) / ainv, x = a exp(v), z = u1^2 u2, r = b + c v - x; accept x if r + (1 + log 4.5) - 4.5 z >= 0, else
//     if r >= log z.  Uniforms only, one log and one exp per attempt (a second log where the squeeze fails); the acceptance
//     rate rises from 0.68 at a = 1 to 0.88.
//   * shape a < 1: Gamma(a) = Gamma(a + 1) U^(1 / a) (the boost identity), U^(1 / a) = exp_nonpositive(log(U) / a); an
//     underflow to 0 is the correct variate there (at a = 1e-3 most of the mass lies below the smallest double).
// nb_variate(mu, k): k = +inf is exactly poisson(mu) -- the same uniforms, the same bits; mu NaN or +inf gives NaN, mu <= 0
// gives 0, a NaN k gives NaN.  A finite k has been validated to lie in [1e-3, 1e6] (sepaihrd_particle_nb_validate).
// Every log / exp is glibc_log / glibc_exp, every other operation a correctly rounded IEEE one (no fma is written and both
// sides compile with contraction off): the host twin and the device agree bit for bit.
// Included by csrc/sepaihrd_predictive_nb.hip and by the host library (host/src/HipPosteriorPredictive.cpp).
#pragma once
#include "sepaihrd_poisson.inc"

namespace sepaihrd_nb_draw {

using sepaihrd_poisson::glibc_exp;
using sepaihrd_poisson::glibc_log;
using sepaihrd_poisson::philox4x32_10;
using sepaihrd_poisson::uniform_open;
using sepaihrd_stoch::exp_nonpositive;

// the variate is inlined into every kernel that draws it: a call would cost the kernel a stack frame (scratch memory)
#if defined(__HIPCC__)
#define SEP_NB_DRAW_FN __host__ __device__ __forceinline__
#else
#define SEP_NB_DRAW_FN inline
#endif

constexpr uint32_t GAMMA_ATTEMPT0 = 0x80000000u;  // fourth counter word of the first gamma attempt
constexpr uint32_t BOOST_WORD = 0xC0000000u;      // fourth counter word of the boost uniform
constexpr double LOG4 = 0x1.62e42fefa39efp+0;               // log(4) rounded to double
constexpr double ONE_PLUS_LOG4_5 = 0x1.40859baee748fp+1;   // 1 + log(4.5) rounded to double

// Gamma(a, 1) for a >= 1
SEP_RNG_FN double gamma_cheng(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, double a) {
    const double ainv = __builtin_sqrt(2.0 * a - 1.0);
    const double b = a - LOG4;
    const double c = a + ainv;
    for (uint32_t attempt = 0;; ++attempt) {
        const sepaihrd_stoch::Philox w = philox4x32_10(c0, c1, c2, GAMMA_ATTEMPT0 + attempt, (uint32_t)seed, (uint32_t)(seed >> 32));
        const double u1 = uniform_open(w.w[0], w.w[1]);
        const double u2 = uniform_open(w.w[2], w.w[3]);
        const double v = glibc_log(u1 / (1.0 - u1)) / ainv;
        const double x = a * glibc_exp(v);
        const double z = u1 * u1 * u2;
        const double r = b + c * v - x;
        if (r + ONE_PLUS_LOG4_5 - 4.5 * z >= 0.0) return x;
        if (r >= glibc_log(z)) return x;
    }
}

// Gamma(a, 1) for a > 0 (a NaN shape: NaN)
SEP_NB_DRAW_FN double gamma(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, double a) {
    if (!(a > 0.0) || a > 0x1.fffffffffffffp+1023) return __builtin_nan("");
    if (a >= 1.0) return gamma_cheng(seed, c0, c1, c2, a);
    const double g = gamma_cheng(seed, c0, c1, c2, a + 1.0);
    const sepaihrd_stoch::Philox w = philox4x32_10(c0, c1, c2, BOOST_WORD, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double U = uniform_open(w.w[0], w.w[1]);
    return g * exp_nonpositive(glibc_log(U) / a);
}

// finite (a NaN, e.g. from a NaN theta entry, counts as dispersed and gives a NaN variate)
SEP_RNG_FN bool dispersed(double k) { return !(k > 0x1.fffffffffffffp+1023); }

// y ~ NegativeBinomial(mean mu, dispersion k); k = +inf: Poisson(mu)
SEP_NB_DRAW_FN double nb_variate(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, double mu, double k) {
    if (mu != mu) return mu;
    if (!(mu > 0.0)) return 0.0;
    if (mu > 0x1.fffffffffffffp+1023) return __builtin_nan("");
    double lambda = mu;
    if (dispersed(k)) {
        const double G = gamma(seed, c0, c1, c2, k);
        lambda = mu * (G / k);
    }
    return sepaihrd_poisson::poisson(seed, c0, c1, c2, lambda);
}

}  // namespace sepaihrd_nb_draw
