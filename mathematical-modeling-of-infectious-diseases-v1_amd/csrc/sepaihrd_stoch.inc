// csrc/sepaihrd_stoch.inc -- the stochastic chain-binomial SIR model (the reference's StochasticSIRModel) as one text for
// host and device: a counter-based random stream, a binomial sampler and the model's step.
//
// The reference draws from ONE gsl_rng_mt19937 seeded from the clock and the pid (SIR_stochastic.cpp:42), replicate after
// replicate: none of its streams can be reproduced and a serial stream cannot be spread over lanes.  This build defines
// its own, stateless one.  Every variate is a pure function of
//     (seed, group, replicate, step, transition, attempt)
// through Philox-4x32-10 (Salmon et al. 2011, PAPERS.md):
//     key     = (seed low word, seed high word)
//     counter = (replicate, step, 2 group + transition, attempt)        transition 0 = infection, 1 = recovery
// One Philox block serves one ATTEMPT of the sampler: words (0, 1) give its first uniform, words (2, 3) its second (the
// inversion uses the first only).  64 bits w = lo + hi 2^32 become a double by
//     u = ((w >> 12) + 0.5) 2^-52,
// 2^52 equally spaced values from 2^-53 to 1 - 2^-53: every one is exact in double (2^52 - 0.5 has 53 significant bits),
// none is 0 or 1, so log(u) and log(1 - u) are finite.
//
// Binomial(n, p), exact in distribution (up to double rounding of the probabilities):
//   * p > 0.5: draw Binomial(n, 1 - p) and return n minus it (1 - p is exact there); n = 0 or p <= 0: 0; p >= 1: n;
//   * n min(p, 1 - p) < 10: inversion by sequential search from 0 (Kachitvichyanukul & Schmeiser's BINV), q^n formed as
//     exp(n log(1 - p)) with log(1 - p) by its series below p = 2^-10 and with the rounding of 1 - p corrected above;
//   * otherwise Hoermann's transformed rejection with squeeze, BTRS (PAPERS.md), the log-factorials by a table up to 9! and
//     Stirling's series to r^-7 beyond.
// Every log / exp is glibc_log / glibc_exp of csrc/sepaihrd_rng.inc, every other operation a correctly rounded IEEE one
// (+, -, *, /, sqrt, floor, round, explicit fma only: both sides compile with contraction off), so the host twin and the
// device kernel agree bit for bit whatever libm the host has.
// Included by csrc/sepaihrd_stoch_sir.hip and by the host library (host/src/HipStochasticSIR.cpp).
#pragma once
#include "sepaihrd_quantile.inc"
#include "sepaihrd_rng.inc"

namespace sepaihrd_stoch {

using sepaihrd_rng::glibc_exp;
using sepaihrd_rng::glibc_log;

constexpr int TRANSITION_INFECTION = 0, TRANSITION_RECOVERY = 1;
constexpr double INVERSION_BELOW = 10.0;  // n min(p, 1 - p) below this: inversion; BTRS needs n p >= 10
constexpr int INVERSION_RESTART = 110;    // BINV's guard: a search past 110 (probability < 1e-60 at n p < 10) draws again

struct Philox {
    uint32_t w[4];
};

SEP_RNG_FN Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox r;
    r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3;
    return r;
}

// two output words -> a double strictly inside (0, 1)
SEP_RNG_FN double uniform_open(uint32_t lo, uint32_t hi) {
    const uint64_t w = (uint64_t)lo | ((uint64_t)hi << 32);
    return ((double)(w >> 12) + 0.5) * 0x1p-52;
}

// where a variate sits in the stream
struct Coord {
    uint64_t seed;
    uint32_t group, replicate, step, transition;
};

SEP_RNG_FN void attempt_uniforms(const Coord& c, uint32_t attempt, double& u, double& v) {
    const Philox b = philox4x32_10(c.replicate, c.step, 2u * c.group + c.transition, attempt, (uint32_t)c.seed, (uint32_t)(c.seed >> 32));
    u = uniform_open(b.w[0], b.w[1]);
    v = uniform_open(b.w[2], b.w[3]);
}

// exp(x) for x <= 0 over the whole range: below -512 (outside glibc_exp) the true value is under 2^-738, and 1 - exp(x) is
// exactly 1.0 in double either way
SEP_RNG_FN double exp_nonpositive(double x) { return x <= -512.0 ? 0.0 : glibc_exp(x); }

SEP_RNG_FN double clamp01(double p) { return p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p); }

// SIR_stochastic.cpp:180-186: 1 - exp(-(beta I h / N)) with the double I and the model's N (0 if N <= 0), 1 - exp(-gamma h)
SEP_RNG_FN double infection_probability(double beta, double I, double h, double N) {
    const double term = (N > 0.0) ? beta * I * h / N : 0.0;
    return clamp01(1.0 - exp_nonpositive(-term));
}
SEP_RNG_FN double recovery_probability(double gamma, double h) { return clamp01(1.0 - exp_nonpositive(-gamma * h)); }

// log(1 - p) for 0 < p <= 0.5
SEP_RNG_FN double log_one_minus(double p) {
    if (p < 0x1p-10) {  // -(p + p^2/2 + ... + p^8/8): the first term left out is below 2^-80 p
        double s = 1.0 / 8.0;
        s = __builtin_fma(s, p, 1.0 / 7.0);
        s = __builtin_fma(s, p, 1.0 / 6.0);
        s = __builtin_fma(s, p, 1.0 / 5.0);
        s = __builtin_fma(s, p, 1.0 / 4.0);
        s = __builtin_fma(s, p, 1.0 / 3.0);
        s = __builtin_fma(s, p, 1.0 / 2.0);
        s = __builtin_fma(s, p, 1.0);
        return -(s * p);
    }
    const double q = 1.0 - p;              // rounded: q = (1 - p)(1 + e)
    const double lost = (1.0 - q) - p;     // exactly (1 - p) - q
    return glibc_log(q) + lost / q;        // log(1 - p) = log q + log(1 + lost / q)
}

// log(k!) for k >= 0
SEP_RNG_FN double log_factorial(double k) {
    if (k < 10.0) {
        switch ((int)k) {
            case 0: case 1: return 0.0;
            case 2: return 0x1.62e42fefa39efp-1;   // log 2
            case 3: return 0x1.cab0bfa2a2002p+0;   // log 6
            case 4: return 0x1.96ca77c922cf9p+1;   // log 24
            case 5: return 0x1.326643c4479c9p+2;   // log 120
            case 6: return 0x1.a51273acf01cap+2;   // log 720
            case 7: return 0x1.10ce1f32dcc30p+3;   // log 5040
            case 8: return 0x1.5358e82fcb70dp+3;   // log 40320
            default: return 0x1.99a8921a7f7cfp+3;  // log 362880
        }
    }
    const double r = k + 1.0, ir = 1.0 / r, ir2 = ir * ir;
    double c = -1.0 / 1680.0;
    c = __builtin_fma(c, ir2, 1.0 / 1260.0);
    c = __builtin_fma(c, ir2, -1.0 / 360.0);
    c = __builtin_fma(c, ir2, 1.0 / 12.0);
    return (k + 0.5) * glibc_log(r) - r + 0x1.d67f1c864beb5p-1 /* log(2 pi) / 2 */ + c * ir;
}

// Binomial(n, p) for 0 < p <= 0.5, n >= 1
SEP_RNG_FN int32_t binomial_lower_half(const Coord& c, int32_t n, double p) {
    const double nd = (double)n, q = 1.0 - p;
    double u, v;
    if (nd * p < INVERSION_BELOW) {
        const double s = p / q, a = (nd + 1.0) * s;
        const double r0 = exp_nonpositive(nd * log_one_minus(p));  // q^n >= exp(-13.9)
        const int32_t bound = n < INVERSION_RESTART ? n : INVERSION_RESTART;
        for (uint32_t attempt = 0;; ++attempt) {
            attempt_uniforms(c, attempt, u, v);
            double r = r0;
            int32_t x = 0;
            while (u > r) {
                u -= r;
                ++x;
                if (x > bound) break;
                r *= a / (double)x - s;  // P(x) = P(x - 1) (n - x + 1) / x  p / q
            }
            if (x <= bound) return x;
            if (n <= INVERSION_RESTART) return n;  // the rounding left over beyond the last atom
        }
    }
    const double spq = __builtin_sqrt(nd * p * q);
    const double b = 1.15 + 2.53 * spq;
    const double a = -0.0873 + 0.0248 * b + 0.01 * p;
    const double cc = nd * p + 0.5;
    const double vr = 0.92 - 4.2 / b;
    const double alpha = (2.83 + 5.1 / b) * spq;
    const double lpq = glibc_log(p / q);
    const double m = __builtin_floor((nd + 1.0) * p);
    const double h = log_factorial(m) + log_factorial(nd - m);
    for (uint32_t attempt = 0;; ++attempt) {
        attempt_uniforms(c, attempt, u, v);
        u -= 0.5;
        const double us = 0.5 - __builtin_fabs(u);
        const double k = __builtin_floor((2.0 * a / us + b) * u + cc);
        if (!(k >= 0.0 && k <= nd)) continue;
        if (us >= 0.07 && v <= vr) return (int32_t)k;
        const double lv = glibc_log(v * alpha / (a / (us * us) + b));
        if (lv <= h - log_factorial(k) - log_factorial(nd - k) + (k - m) * lpq) return (int32_t)k;
    }
}

SEP_RNG_FN int32_t binomial(const Coord& c, int32_t n, double p) {
    if (n <= 0 || !(p > 0.0)) return 0;
    if (p >= 1.0) return n;
    if (p > 0.5) return n - binomial_lower_half(c, n, 1.0 - p);
    return binomial_lower_half(c, n, p);
}

struct Group {
    double N, beta, gamma, S0, I0, R0;
};

// SIR_stochastic.cpp:152-207, one step of one replicate: row `step` -> row `step + 1`.  pR is recovery_probability(gamma, h).
// The reference's N_int only feeds its warning about negative compartments, which cannot occur here, and is left out.
SEP_RNG_FN void sir_step(double& S, double& I, double& R, const Group& g, double h, double pR, uint64_t seed, uint32_t group,
                         uint32_t replicate, uint32_t step) {
    int32_t S_int = (int32_t)__builtin_round(S), I_int = (int32_t)__builtin_round(I);
    if (S_int < 0) S_int = 0;
    if (I_int < 0) I_int = 0;
    if (I_int <= 0 || S_int <= 0) return;  // the reference's freeze: the next row is a copy, recoveries included
    const double pI = infection_probability(g.beta, I, h, g.N);
    Coord c;
    c.seed = seed; c.group = group; c.replicate = replicate; c.step = step;
    c.transition = TRANSITION_INFECTION;
    const int32_t I_new = binomial(c, S_int, pI);
    c.transition = TRANSITION_RECOVERY;
    const int32_t R_new = binomial(c, I_int, pR);
    const double S_next = (double)(S_int - I_new);
    const double I_next = (double)((int64_t)I_int + I_new - R_new);
    const double R_next = R + (double)R_new;
    S = S_next > 0.0 ? S_next : 0.0;
    I = I_next > 0.0 ? I_next : 0.0;
    R = R_next > 0.0 ? R_next : 0.0;
}

// The summaries of one segment of R values sorted ascending (SIR_stochastic.cpp:244-250; GSL's definitions of
// gsl_stats_mean, gsl_stats_median_from_sorted_data and gsl_stats_quantile_from_sorted_data, written down from memory --
// GSL is not available to this build): stat 0 mean by the running recurrence, 1 median, 2 the 0.05 and 3 the 0.95 quantile.
SEP_RNG_FN double sorted_quantile(const double* x, int R, double f) { return sepaihrd_quantile::sorted_quantile(x, (size_t)R, f); }
SEP_RNG_FN double sorted_stat(const double* x, int R, int stat) {
    if (stat == 0) {
        double m = 0.0;
        for (int i = 0; i < R; ++i) m += (x[i] - m) / (double)(i + 1);
        return m;
    }
    if (stat == 1) {
        const int lhs = (R - 1) / 2, rhs = R / 2;
        return lhs == rhs ? x[lhs] : (x[lhs] + x[rhs]) / 2.0;
    }
    return sorted_quantile(x, R, stat == 2 ? 0.05 : 0.95);
}

}  // namespace sepaihrd_stoch
