// csrc/sepaihrd_particle_nb_host.h -- the host-only part of the negative-binomial observation model of the particle filter
// (the rule itself is in csrc/sepaihrd_particle.inc): the rules a dispersion must meet and the row
// constants G.  One text for libsepaihrd_hip.so (csrc/sepaihrd_capi.cpp) and libsepaihrd_host.so (host/src/HipParticleFilter.cpp),
// so that the table the device call uploads and the one the twin adds are the same bits.  glibc's lgamma and log: host only.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

#include "sepaihrd_particle.inc"

namespace sepaihrd_particle {

constexpr const char* NB_SERIES_NAMES[3] = {"k_H", "k_ICU", "k_D"};

// "" for a dispersion the filter takes, else the refusal, which names the entry
inline std::string nb_refusal(const double* dispersion) {
    if (!dispersion) return "dispersion must not be NULL (three entries: k_H, k_ICU, k_D)";
    for (int s = 0; s < 3; ++s) {
        const double k = dispersion[s];
        const std::string who = std::string("dispersion[") + std::to_string(s) + "] (" + NB_SERIES_NAMES[s] + ") ";
        if (k != k) return who + "is NaN: it must be +inf (Poisson) or finite in [1e-3, 1e6]";
        if (k > 1.7976931348623157e308) continue;  // +inf
        if (k < -1.7976931348623157e308) return who + "is -inf: it must be +inf (Poisson) or finite in [1e-3, 1e6]";
        char val[32];
        std::snprintf(val, sizeof(val), "%.17g", k);
        if (k <= 0.0) return who + "= " + val + " is not positive: it must be +inf (Poisson) or finite in [1e-3, 1e6]";
        if (k < NB_K_MIN) return who + "= " + val + " is below 1e-3: it must be +inf (Poisson) or finite in [1e-3, 1e6]";
        if (k > NB_K_MAX) return who + "= " + val + " is above 1e6: it must be +inf (Poisson) or finite in [1e-3, 1e6]";
    }
    return "";
}

// the particle-independent remainder of one cell's log-pmf (without -lgamma(obs + 1))
inline double nb_g(double obs, double k) { return std::lgamma(obs + k) - std::lgamma(k) - obs * std::log(k); }

// G [T_pos]: per output row t >= 0 the sum of nb_g over the usable cells whose series has a finite k, from 0.0, in ascending
// age and within an age in the order H, ICU, D.  observed(series, t, age) is the observation of the cell, NaN where there is none.
template <class Observed>
inline void nb_row_constants(const Dispersion& d, int n_age, int T_pos, Observed&& observed, double* G) {
    const double k[3] = {d.k_H, d.k_ICU, d.k_D};
    for (int t = 0; t < T_pos; ++t) {
        double sum = 0.0;
        for (int i = 0; i < n_age; ++i)
            for (int s = 0; s < 3; ++s) {
                const double obs = observed(s, t, i);
                if (dispersed(k[s]) && usable(obs)) sum += nb_g(obs, k[s]);
            }
        G[t] = sum;
    }
}

}  // namespace sepaihrd_particle
