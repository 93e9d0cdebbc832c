// csrc/sepaihrd_stoch_sepaihrd.inc -- the stochastic chain-binomial form of the age-structured SEPAIHRD model as one text for
// host and device (DESIGN.md section 6j).  The reference has no such model; this one is this build's own.
//
// State: per age class the 11 compartments S, E, P, A, I, H, ICU, R, D, CumH, CumICU as int32 counts.  Output interval k
// (times[k] .. times[k + 1]) is cut into m equal steps of length h_k = (times[k + 1] - times[k]) / m; step j of interval k has
// the global index step = k m + j and takes beta and kappa at its midpoint times[k] + (j + 0.5) h_k.  All 13 draws of a step
// read the state at its start, so an outflow never exceeds its compartment:
//     #   draw                          n                 p
//     0   S -> E                        S                 pr(lambda_i)
//     1   E -> P                        E                 pr(sigma)
//     2   P out                         P                 pr(gamma_p)
//     3   of those, -> A (rest -> I)    draw 2            p_i clamped to [0, 1]
//     4   A -> R                        A                 pr(gamma_A)
//     5   I out                         I                 pr(gamma_I + h_i + d_comm_i)
//     6   of those, -> H (into CumH)    draw 5            share(h_i, gamma_I + d_comm_i)
//     7   of the rest, -> D (rest -> R) draw 5 - draw 6   share(d_comm_i, gamma_I)
//     8   H out                         H                 pr(gamma_H + d_H_i + icu_i)
//     9   of those, -> ICU (into CumICU) draw 8           share(icu_i, gamma_H + d_H_i)
//     10  of the rest, -> D (rest -> R) draw 8 - draw 9   share(d_H_i, gamma_H)
//     11  ICU out                       ICU               pr(gamma_ICU + d_ICU_i)
//     12  of those, -> D (rest -> R)    draw 11           share(d_ICU_i, gamma_ICU)
// with pr(r) = clamp01(1 - exp_nonpositive(-(r h_k))) and share(x, y) = x / (x + y) where x + y > 0, else 0.
// Every variate is sepaihrd_stoch::binomial at key = seed, counter = (s, r, (step 64 + age) 16 + transition, attempt): s the
// sample's position, r the replicate -- the Coord of csrc/sepaihrd_stoch.inc with replicate = s, step = r and
// 2 group + transition carrying the packed third word.  T m < 2^22 keeps that word below 2^32.
// Only correctly rounded IEEE operations and glibc_log / glibc_exp: both sides compile with contraction off.
// Included by csrc/sepaihrd_stoch_sepaihrd.hip, csrc/sepaihrd_particle.hip and csrc/sepaihrd_particle_wide.hip (through
// csrc/sepaihrd_particle.inc) and by the host
// library (host/src/StochasticSEPAIHRDTwin.hpp: HipStochasticSEPAIHRD.cpp, HipParticleFilter.cpp).
#pragma once
#include "sepaihrd_stoch.inc"

#if defined(__clang__)
#define SEP_STOCH_EPI_NO_UNROLL _Pragma("nounroll")
#else
#define SEP_STOCH_EPI_NO_UNROLL _Pragma("GCC unroll 1")
#endif

namespace sepaihrd_stoch_epi {

using sepaihrd_stoch::clamp01;
using sepaihrd_stoch::exp_nonpositive;

constexpr int NUM_COMP = 11, MAX_AGES = 16, NUM_DRAWS = 13, NUM_VEC_FIELDS = 8;
enum Comp { C_S = 0, C_E, C_P, C_A, C_I, C_H, C_ICU, C_R, C_D, C_CUM_H, C_CUM_ICU };
// the per-age vectors of a model-values row, in the VecField order of csrc/sepaihrd_device.h
enum Vec { V_A = 0, V_H_INFEC, V_P, V_H, V_ICU, V_D_H, V_D_ICU, V_D_COMM };
// the scalars at the front of a row
enum Scalar { R_THETA = 0, R_SIGMA, R_GAMMA_P, R_GAMMA_A, R_GAMMA_I, R_GAMMA_H, R_GAMMA_ICU, R_BETA, R_SCALARS };

// One row of model values (sepaihrd_ensemble_stochastic's `model_values`): the 8 scalars, beta_values[nb], kappa_values[nk],
// the eight per-age vectors [8][n], the rounded initial counts [11][n].
struct RowLayout {
    int n, nb, nk;
    SEP_RNG_FN int beta_values() const { return R_SCALARS; }
    SEP_RNG_FN int kappa_values() const { return R_SCALARS + nb; }
    SEP_RNG_FN int vec(int field, int age) const { return R_SCALARS + nb + nk + field * n + age; }
    SEP_RNG_FN int initial(int comp, int age) const { return R_SCALARS + nb + nk + NUM_VEC_FIELDS * n + comp * n + age; }
    SEP_RNG_FN int width() const { return R_SCALARS + nb + nk + (NUM_VEC_FIELDS + NUM_COMP) * n; }
};

// index into a piecewise-constant schedule of `count` values: value j on (ends[j - 1], ends[j]], the baseline for t <= ends[0]
// (and so for t < 0), the last value beyond the last end
SEP_RNG_FN int schedule_index(const double* ends, int count, double t) {
    int c = 0;
    for (int k = 0; k < count; ++k) c += (t > ends[k]) ? 1 : 0;
    return c < count - 1 ? c : count - 1;
}

// beta kappa of a step with midpoint t
SEP_RNG_FN double beta_kappa(const double* row, const RowLayout& L, const double* beta_ends, const double* kappa_ends, double t) {
    const double beta = L.nb > 0 ? row[L.beta_values() + schedule_index(beta_ends, L.nb, t)] : row[R_BETA];
    const double kappa = row[L.kappa_values() + schedule_index(kappa_ends, L.nk, t)];
    return beta * kappa;
}

SEP_RNG_FN double pr(double rate, double h) { return clamp01(1.0 - exp_nonpositive(-(rate * h))); }
SEP_RNG_FN double share(double x, double y) {
    const double d = x + y;
    return d > 0.0 ? x / d : 0.0;
}

// the probabilities of draws 1 .. 12 of one age class on an interval with step length h
struct AgeProbs {
    double pE, pP, toA, pA, pI, toH, toD_I, pH, toICU, toD_H, pICU, toD_ICU;
};
SEP_RNG_FN AgeProbs age_probs(const double* row, const RowLayout& L, int age, double h) {
    const double gI = row[R_GAMMA_I], gH = row[R_GAMMA_H], gICU = row[R_GAMMA_ICU];
    const double hi = row[L.vec(V_H, age)], icu = row[L.vec(V_ICU, age)], dH = row[L.vec(V_D_H, age)], dICU = row[L.vec(V_D_ICU, age)],
                 dC = row[L.vec(V_D_COMM, age)];
    AgeProbs q;
    q.pE = pr(row[R_SIGMA], h);
    q.pP = pr(row[R_GAMMA_P], h);
    q.toA = clamp01(row[L.vec(V_P, age)]);
    q.pA = pr(row[R_GAMMA_A], h);
    q.pI = pr(gI + hi + dC, h);
    q.toH = share(hi, gI + dC);
    q.toD_I = share(dC, gI);
    q.pH = pr(gH + dH + icu, h);
    q.toICU = share(icu, gH + dH);
    q.toD_H = share(dH, gH);
    q.pICU = pr(gICU + dICU, h);
    q.toD_ICU = share(dICU, gICU);
    return q;
}

// inf_j = (P_j + A_j + theta I_j) h_infec_j inv_N_j, inv_N_j = 1 / N_j for N_j > 0 and 0 otherwise
SEP_RNG_FN double infectious_pressure(const int32_t* x, double theta, double h_infec, double N) {
    const double inv_N = N > 0.0 ? 1.0 / N : 0.0;
    return ((double)x[C_P] + (double)x[C_A] + theta * (double)x[C_I]) * h_infec * inv_N;
}
// lambda_i = max(0, contact_sum (beta kappa) a_i); a NaN becomes 0
SEP_RNG_FN double force_of_infection(double contact_sum, double bk, double a) {
    const double v = contact_sum * (bk * a);
    return 0.0 < v ? v : 0.0;
}

// One step of one age class of replicate r of sample s.  The counts of a class never exceed its population (conserved), so the
// sums below stay inside int32 as long as the class total does; they are formed in uint32, which wraps instead of overflowing.
SEP_RNG_FN void age_step(int32_t* x, double lambda, double h, const AgeProbs& q, uint64_t seed, uint32_t s, uint32_t r, uint32_t step,
                         uint32_t age) {
    sepaihrd_stoch::Coord c;
    c.seed = seed;
    c.replicate = s;
    c.step = r;
    c.group = (step * 64u + age) * 8u;  // 2 group + transition = (step 64 + age) 16 + transition
    // ONE call site of the sampler, walked 13 times: inlined 13 times over, it takes the kernel to 512 registers and 1.3 KB of
    // scratch per lane.  The selects around it cost a few instructions against the sampler's hundreds.
    const double p0 = pr(lambda, h);
    uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0, d6 = 0, d7 = 0, d8 = 0, d9 = 0, d10 = 0, d11 = 0, d12 = 0;
    SEP_STOCH_EPI_NO_UNROLL
    for (uint32_t tr = 0; tr < (uint32_t)NUM_DRAWS; ++tr) {
        int32_t n;
        double p;
        switch (tr) {
            case 0: n = x[C_S]; p = p0; break;
            case 1: n = x[C_E]; p = q.pE; break;
            case 2: n = x[C_P]; p = q.pP; break;
            case 3: n = (int32_t)d2; p = q.toA; break;
            case 4: n = x[C_A]; p = q.pA; break;
            case 5: n = x[C_I]; p = q.pI; break;
            case 6: n = (int32_t)d5; p = q.toH; break;
            case 7: n = (int32_t)(d5 - d6); p = q.toD_I; break;
            case 8: n = x[C_H]; p = q.pH; break;
            case 9: n = (int32_t)d8; p = q.toICU; break;
            case 10: n = (int32_t)(d8 - d9); p = q.toD_H; break;
            case 11: n = x[C_ICU]; p = q.pICU; break;
            default: n = (int32_t)d11; p = q.toD_ICU; break;
        }
        c.transition = tr;
        const uint32_t v = (uint32_t)sepaihrd_stoch::binomial(c, n, p);
        switch (tr) {
            case 0: d0 = v; break;
            case 1: d1 = v; break;
            case 2: d2 = v; break;
            case 3: d3 = v; break;
            case 4: d4 = v; break;
            case 5: d5 = v; break;
            case 6: d6 = v; break;
            case 7: d7 = v; break;
            case 8: d8 = v; break;
            case 9: d9 = v; break;
            case 10: d10 = v; break;
            case 11: d11 = v; break;
            default: d12 = v; break;
        }
    }
    auto add = [&](int comp, uint32_t in, uint32_t out) { x[comp] = (int32_t)((uint32_t)x[comp] + in - out); };
    add(C_S, 0u, d0);
    add(C_E, d0, d1);
    add(C_P, d1, d2);
    add(C_A, d3, d4);
    add(C_I, d2 - d3, d5);
    add(C_H, d6, d8);
    add(C_ICU, d9, d11);
    add(C_R, d4 + (d5 - d6 - d7) + (d8 - d9 - d10) + (d11 - d12), 0u);
    add(C_D, d7 + d10 + d12, 0u);
    add(C_CUM_H, d6, 0u);
    add(C_CUM_ICU, d9, 0u);
}

// ---- One output interval (t0, t0 + m h]: m steps from the counts at its start; step j takes beta kappa at its midpoint
// t0 + (j + 0.5) h, sums the contacts over jj = 0 .. n - 1 ascending and draws at the step coordinate first_step + j (first_step =
// k m for the interval that begins at times[k]).  q holds age_probs(row, L, age, h) of the interval.  Two forms of ONE walk:
// what the "device equals twin" and the "a particle is a replicate" tests compare bit for bit is that the two agree.

// What a lane of lane_interval keeps of its age class for the whole run.  Lanes of padded ages (age >= n) read age 0's entries
// of the row and use none of them; N and M are padded to lpc (N [lpc], M [lpc][lpc] row-major).
struct LaneConstants {
    double theta, h_infec, a_i, Ni;
    const double* Mrow;  // M(age, .)
    int row_age;
};
SEP_RNG_FN LaneConstants lane_constants(const double* row, const RowLayout& L, const double* N, const double* M, int lpc, int age) {
    LaneConstants c;
    c.row_age = age < L.n ? age : 0;
    c.theta = row[R_THETA];
    c.h_infec = row[L.vec(V_H_INFEC, c.row_age)];
    c.a_i = row[L.vec(V_A, c.row_age)];
    c.Ni = N[age];
    c.Mrow = M + (size_t)age * lpc;
    return c;
}

// Lane form: the caller is age class `age` of replicate r of sample s and holds its 11 counts x; exchange(inf, jj) returns the
// infectious pressure of age class jj of the same replicate (stoch_epi_step_kernel: __shfl(inf, jj, lpc); particle_filter_kernel writes the same walk out, see csrc/sepaihrd_particle.hip).  all_ages_interval below is
// the same walk with every age class in one caller.
template <class Exchange>
SEP_RNG_FN void lane_interval(int32_t* x, const double* row, const RowLayout& L, const LaneConstants& c, const double* beta_ends,
                              const double* kappa_ends, double t0, double h, const AgeProbs& q, int m, uint64_t seed, uint32_t s, uint32_t r,
                              uint32_t first_step, uint32_t age, Exchange exchange) {
    for (int j = 0; j < m; ++j) {
        const double t_mid = t0 + ((double)j + 0.5) * h;
        const double bk = beta_kappa(row, L, beta_ends, kappa_ends, t_mid);
        const double inf = infectious_pressure(x, c.theta, c.h_infec, c.Ni);
        double sum = 0.0;
        for (int jj = 0; jj < L.n; ++jj) sum += c.Mrow[jj] * exchange(inf, jj);
        const double lambda = force_of_infection(sum, bk, c.a_i);
        age_step(x, lambda, h, q, seed, s, r, first_step + (uint32_t)j, age);
    }
}

// All-ages form: the counts of age class i are x + i * stride, its probabilities q[i]; N [n], M [n][n] row-major.  Per step the
// pressures of all ages, then the lambdas of all ages, then the steps: lane_interval above with the exchange done in memory.
SEP_RNG_FN void all_ages_interval(int32_t* x, int stride, const double* row, const RowLayout& L, const double* N, const double* M,
                                  const double* beta_ends, const double* kappa_ends, double t0, double h, const AgeProbs* q, int m,
                                  uint64_t seed, uint32_t s, uint32_t r, uint32_t first_step) {
    const int n = L.n;
    double lambda[MAX_AGES], pressure[MAX_AGES];
    for (int j = 0; j < m; ++j) {
        const double t_mid = t0 + ((double)j + 0.5) * h;
        const double bk = beta_kappa(row, L, beta_ends, kappa_ends, t_mid);
        for (int i = 0; i < n; ++i) pressure[i] = infectious_pressure(x + i * stride, row[R_THETA], row[L.vec(V_H_INFEC, i)], N[i]);
        for (int i = 0; i < n; ++i) {
            double sum = 0.0;
            for (int jj = 0; jj < n; ++jj) sum += M[(size_t)i * n + jj] * pressure[jj];
            lambda[i] = force_of_infection(sum, bk, row[L.vec(V_A, i)]);
        }
        for (int i = 0; i < n; ++i) age_step(x + i * stride, lambda[i], h, q[i], seed, s, r, first_step + (uint32_t)j, (uint32_t)i);
    }
}

// The observed series of an age class are the increments of CumH, CumICU and D between output rows (in that order): inc = the
// counts now less prev, and prev takes the counts now.
constexpr int NUM_PREV = 3;
SEP_RNG_FN void take_increments(const int32_t* x, int32_t* prev, int32_t* inc) {
    const int32_t now[NUM_PREV] = {x[C_CUM_H], x[C_CUM_ICU], x[C_D]};
    for (int ser = 0; ser < NUM_PREV; ++ser) {
        inc[ser] = now[ser] - prev[ser];
        prev[ser] = now[ser];
    }
}

// a rounded initial count is usable when it lies in [0, 2^31 - 1] (a NaN is not)
SEP_RNG_FN bool count_in_range(double rounded) { return rounded >= 0.0 && rounded <= 2147483647.0; }

}  // namespace sepaihrd_stoch_epi
