// csrc/sepaihrd_nb_objective.inc -- the negative-binomial observation model of the deterministic SEPAIHRD objective as one text
// for host and device (DESIGN.md section 6o).  The reference has no such likelihood; this one is this build's own.
//
// Each observed series (H, ICU, D) has one dispersion k: +inf, or finite in [NB_K_MIN, NB_K_MAX] (csrc/sepaihrd_particle.inc).  A
// cell (series, day, age) is usable when its observation is finite and >= 0; sim = max(0, increment) + 1e-10.
//   k = +inf   cell = obs log(sim) - sim                                              (today's Poisson cell)
//   k finite   cell = term + g,   term = obs log(sim) - (obs + k) glibc_log(1.0 + sim / k)   (nb_term's formula and association)
//                                 g    = (lgamma(obs + k) - lgamma(k)) - obs glibc_log(k),           exactly 0 when obs == 0
// with the difference of the two lgammas formed from their two-part values (lgamma_difference, csrc/sepaihrd_lgamma.inc: at
// k = 1e6 the rounding of either lgamma to one double would cost more than the cell may be off by),
// and an unusable cell is 0.  The -lgamma(obs + 1) of the pmf is left out, as the Poisson term leaves it out.
// Sums keep the reference's order: within a day the ages ascending, the days ascending from 0.0 per series,
// total = (H + ICU) + D; a NaN or Inf total gives status 1 and lowest().
// log(sim) is the caller's: the device passes take log_pos (csrc/sepaihrd_dev_common.inc), the host twin std::log -- the one
// operation the two sides do not share (the same difference as in the Poisson objective).  Everything else is glibc_log and
// correctly rounded IEEE operations: every includer compiles with contraction off.
// Included by csrc/sepaihrd_nb_objective.hip (the device pass and sepaihrd_nb_objective_host) and by the host library.
#pragma once
#include "sepaihrd_lgamma.inc"

namespace sepaihrd_nb_objective {

using sepaihrd_lgamma::lgamma_difference;
using sepaihrd_lgamma::lgamma_parts;
using sepaihrd_rng::glibc_log;

constexpr double SIM_FLOOR = 1e-10;
constexpr double K_MIN = 1e-3, K_MAX = 1e6;  // NB_K_MIN, NB_K_MAX of csrc/sepaihrd_particle.inc

// finite and >= 0 (a NaN fails the first comparison, +inf the second)
SEP_RNG_FN bool usable(double obs) { return obs >= 0.0 && obs <= 1.7976931348623157e308; }
// a validated k is +inf or finite: a finite one selects the negative-binomial cell (a NaN, e.g. from a NaN theta entry, too:
// its cells are NaN and the total fails the finiteness check)
SEP_RNG_FN bool dispersed(double k) { return !(k > 1.7976931348623157e308); }

// what a series' cells share: k, lgamma(k) in its two parts and glibc_log(k) (unused where k = +inf)
struct SeriesK {
    double k, log_k;
    sepaihrd_lgamma::Parts lgamma_k;
};
SEP_RNG_FN SeriesK series_k(double k) {
    SeriesK s;
    s.k = k;
    const bool nb = dispersed(k);
    s.lgamma_k = lgamma_parts(nb ? k : 1.0);
    s.log_k = nb ? glibc_log(k) : 0.0;
    return s;
}

SEP_RNG_FN double sim_of(double increment) { return ((increment < 0.0) ? 0.0 : increment) + SIM_FLOOR; }

SEP_RNG_FN double nb_g(double obs, const SeriesK& s) {
    if (obs == 0.0) return 0.0;
    return lgamma_difference(lgamma_parts(obs + s.k), s.lgamma_k) - obs * s.log_k;
}

// one cell; log_sim = log(sim) as the caller takes it.  fused_poisson: the Poisson cell as ONE fma, which is how the kernels of
// the fma arithmetic (compiled with contraction on) evaluate obs log(sim) - sim -- the device pass asks for it on a context in
// that arithmetic, so that a series left at +inf keeps the bits of the Poisson objective in either mode
SEP_RNG_FN double cell(double obs, double sim, double log_sim, const SeriesK& s, bool fused_poisson = false) {
    if (!usable(obs)) return 0.0;
    if (!dispersed(s.k)) return fused_poisson ? __builtin_fma(obs, log_sim, -sim) : obs * log_sim - sim;
    const double term = obs * log_sim - (obs + s.k) * glibc_log(1.0 + sim / s.k);
    return term + nb_g(obs, s);
}

// The host's walk over one chain: inc [T][3][n] (series H, ICU, D), obs [3][T][n] (NaN where there is none), k [3].
// parts [3] and the total; returns the status (0, or 1 for a NaN / Inf total, with total = lowest()).
template <class LogSim>
inline int chain_loglik(const double* inc, const double* obs, const double* k, int T, int n, LogSim&& log_of_sim, double* total, double* parts) {
    for (int s = 0; s < 3; ++s) {
        const SeriesK sk = series_k(k[s]);
        double acc = 0.0;
        for (int t = 0; t < T; ++t) {
            double row = 0.0;
            for (int a = 0; a < n; ++a) {
                const double sim = sim_of(inc[((size_t)t * 3 + s) * n + a]);
                row += cell(obs[((size_t)s * T + t) * n + a], sim, log_of_sim(sim), sk);
            }
            acc += row;
        }
        parts[s] = acc;
    }
    const double sum = (parts[0] + parts[1]) + parts[2];
    if (sum != sum || sum > 1.7976931348623157e308 || sum < -1.7976931348623157e308) {
        *total = -1.7976931348623157e308;
        return 1;
    }
    *total = sum;
    return 0;
}

}  // namespace sepaihrd_nb_objective
