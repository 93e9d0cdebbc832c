// csrc/sepaihrd_particle.inc -- the bootstrap particle filter of the stochastic chain-binomial SEPAIHRD model as one text for
// host and device (DESIGN.md section 6k): what a particle is, the log-weight of an observed row, the normalisation and the
// systematic resampling.  The reference has no such filter; this one is this build's own (Gordon, Salmond & Smith 1993;
// Kitagawa 1996 -- PAPERS.md).
//
// Particles.  For theta at position b, slot j (0 <= j < J) starts from the rounded initial counts of b's model-values row and
// advances with sepaihrd_stoch_epi::age_step at the coordinates (seed, s = b, r = j, step, age, transition), with the midpoint
// beta kappa rule and the m steps per output interval of csrc/sepaihrd_stoch_sepaihrd.inc: until the first resampling slot j IS
// replicate j of sepaihrd_ensemble_stochastic.  A slot keeps drawing at its own slot index after an ancestor has overwritten it.
//
// Log-weight of output row k, t = k - runup_offset >= 0.  Per age a the increments of CumH, CumICU and D since the previous
// output row (the run's first row has increment 0), sim = max(0, inc) + 1e-10, term = obs glibc_log(sim) - sim where the
// observation is usable (finite and >= 0, the likelihood's rule) and 0 elsewhere;
//     t_a = (term_H + term_ICU) + term_D,     lw_j = sum_a t_a from 0.0 in ascending a.
// A row without a usable (series, age) cell is skipped: no weighting, no resampling, increment 0, ESS NaN.
// With a dispersion (DESIGN.md section 6m; stated below, above nb_term) a series' term is negative binomial instead and the row's
// increment gains a constant; with none every line here holds as it stands.
//
// Normalisation.  M = max_j lw_j, w_j = exp_nonpositive(lw_j - M); C = the inclusive prefix sums of w in the Kogge-Stone order,
// which is a function of J alone: for d = 1, 2, 4, ... < J, c[j] += c[j - d] for all j >= d at once (on the host the same loop
// with j descending); Q = the same scan over w_j^2;
//     increment = M + glibc_log(C[J - 1] / J),     ESS = C[J - 1]^2 / Q[J - 1],     loglik = sum of the increments in time order.
//
// Systematic resampling at EVERY weighted row: one uniform u per (b, k), the first uniform of attempt_uniforms at attempt 0 with
// Coord{seed, replicate = b, step = 0xFFFFFFFF, group = 512 k, transition = 13}, so that 2 group + transition = (64 k) 16 + 13.
// Particles own transitions 0 .. 12 only and their second word is r < J < 2^31: the coordinate meets none of theirs.  The
// ancestor of slot i is the smallest j with C[j] > ((u + i) / J) C[J - 1], clamped to J - 1, found by binary search (the
// search's own outcome where rounding leaves C not monotone -- the same on both sides).  Slot i takes the 11 n counts of its
// ancestor and the ancestor's previous-row CumH, CumICU and D.  After a resampling all weights are equal: no weights are carried
// from row to row and there is no adaptive (ESS-threshold) rule.
//
// Only correctly rounded IEEE operations and glibc_log / glibc_exp: both sides compile with contraction off.
// Included by csrc/sepaihrd_particle.hip, csrc/sepaihrd_particle_wide.hip (the wide form, DESIGN.md section 6l) and by the host
// library (host/src/HipParticleFilter.cpp).
#pragma once
#include "sepaihrd_stoch_sepaihrd.inc"

namespace sepaihrd_particle {

namespace epi = sepaihrd_stoch_epi;
using sepaihrd_rng::glibc_log;
using sepaihrd_stoch::exp_nonpositive;

constexpr double SIM_FLOOR = 1e-10;
constexpr uint32_t RESAMPLE_STEP = 0xFFFFFFFFu, RESAMPLE_TRANSITION = 13u;
using sepaihrd_stoch_epi::NUM_PREV;  // the previous-row values a particle carries: CumH, CumICU, D (take_increments)

// finite and >= 0 (a NaN fails the first comparison, +inf the second)
SEP_RNG_FN bool usable(double obs) { return obs >= 0.0 && obs <= 1.7976931348623157e308; }

SEP_RNG_FN double poisson_term(double obs, int32_t inc) {
    const double sim = (double)(inc > 0 ? inc : 0) + SIM_FLOOR;
    return usable(obs) ? obs * glibc_log(sim) - sim : 0.0;
}
// t_a of one age class: obs and inc in the order H, ICU, D
SEP_RNG_FN double age_term(double obs_H, double obs_ICU, double obs_D, int32_t inc_H, int32_t inc_ICU, int32_t inc_D) {
    return (poisson_term(obs_H, inc_H) + poisson_term(obs_ICU, inc_ICU)) + poisson_term(obs_D, inc_D);
}

// ---- the negative-binomial observation model (DESIGN.md section 6m): one dispersion k per observed series, +inf or finite in
// [NB_K_MIN, NB_K_MAX].  +inf keeps that series' poisson_term.  For a finite k the series is negative binomial with mean sim and
// size k (variance sim + sim^2 / k); the part of its log-pmf that depends on the particle is
//     nb_term = obs glibc_log(sim) - (obs + k) glibc_log(1.0 + sim / k).
// The rest, g(obs, k) = lgamma(obs + k) - lgamma(k) - obs log(k), is the same for every particle of a row: it never enters the
// weights and is added to the row's increment as the row constant G (csrc/sepaihrd_particle_nb_host.h forms it on the host).
// The -lgamma(obs + 1) of the pmf is left out, as poisson_term leaves it out; with that convention nb_term + g tends to
// poisson_term as k grows, the difference being ((sim - obs)^2 - obs) / (2 k) + O(k^-2).  Above NB_K_MAX the cancellation in
// these formulas costs more than 1e-8.
constexpr double NB_K_MIN = 1e-3, NB_K_MAX = 1e6;
struct Dispersion {
    double k_H, k_ICU, k_D;
};
// a validated k is +inf or finite: a finite one selects nb_term
SEP_RNG_FN bool dispersed(double k) { return k <= 1.7976931348623157e308; }
SEP_RNG_FN bool any_dispersed(const Dispersion& d) { return dispersed(d.k_H) || dispersed(d.k_ICU) || dispersed(d.k_D); }

SEP_RNG_FN double nb_term(double obs, int32_t inc, double k) {
    const double sim = (double)(inc > 0 ? inc : 0) + SIM_FLOOR;
    return usable(obs) ? obs * glibc_log(sim) - (obs + k) * glibc_log(1.0 + sim / k) : 0.0;
}
SEP_RNG_FN double series_term(double obs, int32_t inc, double k) { return dispersed(k) ? nb_term(obs, inc, k) : poisson_term(obs, inc); }
// t_a of one age class under the dispersion d: age_term's association, each series by its own k
SEP_RNG_FN double age_term(double obs_H, double obs_ICU, double obs_D, int32_t inc_H, int32_t inc_ICU, int32_t inc_D, const Dispersion& d) {
    return (series_term(obs_H, inc_H, d.k_H) + series_term(obs_ICU, inc_ICU, d.k_ICU)) + series_term(obs_D, inc_D, d.k_D);
}
// the increment of a weighted row whose constant is G
SEP_RNG_FN double increment_with_constant(double inc, double G) { return inc + G; }

SEP_RNG_FN double weight(double lw, double M) { return exp_nonpositive(lw - M); }
SEP_RNG_FN double increment(double M, double total, int J) { return M + glibc_log(total / (double)J); }
SEP_RNG_FN double effective_sample_size(double total, double total_sq) { return total * total / total_sq; }

// the uniform of the resampling at output row k of theta b
SEP_RNG_FN double resample_uniform(uint64_t seed, uint32_t b, uint32_t k) {
    sepaihrd_stoch::Coord c;
    c.seed = seed;
    c.replicate = b;
    c.step = RESAMPLE_STEP;
    c.group = k * 512u;  // 2 group + transition = (64 k) 16 + 13
    c.transition = RESAMPLE_TRANSITION;
    double u, v;
    sepaihrd_stoch::attempt_uniforms(c, 0u, u, v);
    return u;
}

// the ancestor of slot i: C the prefix sums [J]
SEP_RNG_FN int ancestor(const double* C, int J, double u, int i) {
    const double target = ((u + (double)i) / (double)J) * C[J - 1];
    int lo = 0, hi = J - 1;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (C[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the host's form of the scan: the Kogge-Stone order with j descending, so that c[j - d] is still the previous round's
SEP_RNG_FN void prefix_sums_in_order(double* c, int J) {
    for (int d = 1; d < J; d <<= 1)
        for (int j = J - 1; j >= d; --j) c[j] += c[j - d];
}

// One weighted row on the host: lw [J] in; anc [J], the increment and the ESS out; C and Q are scratch [J].
SEP_RNG_FN void normalise_and_resample(const double* lw, int J, double u, double* C, double* Q, int32_t* anc, double& inc, double& ess) {
    double M = lw[0];
    for (int j = 1; j < J; ++j) M = lw[j] > M ? lw[j] : M;
    for (int j = 0; j < J; ++j) {
        const double w = weight(lw[j], M);
        C[j] = w;
        Q[j] = w * w;
    }
    prefix_sums_in_order(C, J);
    prefix_sums_in_order(Q, J);
    inc = increment(M, C[J - 1], J);
    ess = effective_sample_size(C[J - 1], Q[J - 1]);
    for (int i = 0; i < J; ++i) anc[i] = ancestor(C, J, u, i);
}

}  // namespace sepaihrd_particle
