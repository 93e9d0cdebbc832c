// csrc/sepaihrd_particle.hip -- the bootstrap particle filter of the stochastic SEPAIHRD model on gfx950
// (sepaihrd_particle_loglik): the filter kernel, one workgroup per theta, and the probe of one row's
// normalisation and resampling.  The rules are csrc/sepaihrd_particle.inc, the text the host twin compiles too; the decode from
// theta to model values is csrc/sepaihrd_stoch_sepaihrd.hip's.  The filter kernel keeps its own copy of the interval walk
// (csrc/sepaihrd_stoch_sepaihrd.inc's lane_interval, with first_step = (k - 1) m): through lane_interval the same registers
// and LDS gave a kernel 0.4 % slower at J = 136 on an MI355X.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_particle.inc"
#include "sepaihrd_particle_device.h"
#include "sepaihrd_particle_nb_host.h"
#include "sepaihrd_stoch_sepaihrd_device.h"

namespace sepaihrd {
namespace {

namespace epi = sepaihrd_stoch_epi;
namespace pf = sepaihrd_particle;

constexpr int STATE_INTS = epi::NUM_COMP + pf::NUM_PREV;  // what a particle keeps per age class between output rows

// The LDS of one block, carved from the dynamic allocation (particle_lds_bytes): the doubles first.
struct BlockLds {
    double* red;     // [PARTICLE_BLOCK / WAVE] the waves' maxima
    double* lw;      // [J] log-weights of the row
    double* C;       // [J] prefix sums of w
    double* Q;       // [J] prefix sums of w^2
    int32_t* anc;    // [J] ancestors of the last weighted row
    int32_t* state;  // [2][J][STATE_INTS][lpc]
};
__device__ BlockLds carve(double* base, int J) {
    BlockLds l;
    l.red = base;
    l.lw = base + PARTICLE_LDS_FIXED / sizeof(double);
    l.C = l.lw + J;
    l.Q = l.C + J;
    l.anc = reinterpret_cast<int32_t*>(l.Q + J);
    l.state = l.anc + J;
    return l;
}

// One weighted row across the block, lane j for particle j (J <= blockDim.x): the maximum, the weights, the two Kogge-Stone
// scans in the order csrc/sepaihrd_particle.inc fixes, the ancestors.  Every lane of the block calls it; lw must be visible
// (a barrier after its writes).  Lane 0 returns the increment and the ESS; anc is visible on return.
__device__ void block_normalise_and_resample(const BlockLds& l, int J, double u, double& inc, double& ess) {
    const int j = (int)threadIdx.x;
    const bool mine = j < J;
    const double my_lw = mine ? l.lw[j] : -__builtin_inf();
    double mx = my_lw;
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(mx, off, WAVE);
        mx = o > mx ? o : mx;
    }
    if ((j & (WAVE - 1)) == 0) l.red[j / WAVE] = mx;
    __syncthreads();
    double M = l.red[0];
    for (int w = 1; w < (int)(blockDim.x / WAVE); ++w) M = l.red[w] > M ? l.red[w] : M;
    if (mine) {
        const double w = pf::weight(my_lw, M);
        l.C[j] = w;
        l.Q[j] = w * w;
    }
    __syncthreads();
    for (int d = 1; d < J; d <<= 1) {
        const bool take = mine && j >= d;
        const double c = take ? l.C[j - d] : 0.0, q = take ? l.Q[j - d] : 0.0;
        __syncthreads();  // every read of this round before any write of it
        if (take) {
            l.C[j] += c;
            l.Q[j] += q;
        }
        __syncthreads();
    }
    if (j == 0) {
        inc = pf::increment(M, l.C[J - 1], J);
        ess = pf::effective_sample_size(l.C[J - 1], l.Q[J - 1]);
    }
    if (mine) l.anc[j] = pf::ancestor(l.C, J, u, j);
    __syncthreads();
}

// One workgroup per theta b.  Lanes as in stoch_epi_step_kernel: one per (particle, age class), the lpc lanes of a particle
// adjacent, so a block runs G = PARTICLE_BLOCK / lpc particles at a time and walks the J particles in ceil(J / G) passes per
// output row.  A particle's 11 counts and its previous-row CumH, CumICU, D live in LDS between output rows and in registers
// through the m steps of an interval.  There are two copies of the state: a pass reads slot anc[p] of one (p itself where the
// last row was not resampled) and writes slot p of the other, which is the resampling's copy and costs no pass of its own.
// Barriers: one at the top of every row (it also carries the block-uniform "this row has a usable observation"), so that no
// lane writes a copy others still read; then those of the weighting.  Lanes of padded ages and of the slots beyond J in the
// last pass carry zero counts and draw nothing; they reach every barrier.  An invalid theta ends its whole block at once.
//
// NB = "some series is dispersed" (DESIGN.md section 6m).  The false instantiation is the Poisson kernel, argument for argument;
// the true one takes the three k and the row constants in its argument struct, weighs each series by a kernel-uniform test on
// its k (pf::series_term) and has lane 0 add the row's constant where the increment is formed.  No per-particle state is added.
template <bool NB>
__global__ __launch_bounds__(PARTICLE_BLOCK) void particle_filter_kernel(const DevProblem pb, const std::conditional_t<NB, ParticleArgsNB, ParticleArgs> a) {
    extern __shared__ double particle_lds[];
    const int n = pb.n, lpc = pb.lpc, T = pb.T, Tp = pb.T - pb.runup_offset, J = a.J;
    const uint32_t b = blockIdx.x;
    const int tid = (int)threadIdx.x;
    const double qnan = __builtin_nan("");
    const size_t final_doubles = (size_t)J * epi::NUM_COMP * n;
    if (a.status[b] != 0) {  // uniform across the block
        if (tid == 0) a.loglik[b] = -DBL_MAX;
        for (int t = tid; t < Tp; t += PARTICLE_BLOCK) {
            if (a.increments != nullptr) a.increments[(size_t)b * Tp + t] = qnan;
            if (a.ess != nullptr) a.ess[(size_t)b * Tp + t] = qnan;
        }
        if (a.final_state != nullptr)
            for (size_t i = (size_t)tid; i < final_doubles; i += PARTICLE_BLOCK) a.final_state[(size_t)b * final_doubles + i] = qnan;
        return;
    }
    const BlockLds l = carve(particle_lds, J);
    const int G = PARTICLE_BLOCK / lpc, passes = (J + G - 1) / G;
    const int group = tid / lpc, age = tid % lpc;
    const bool real_age = age < n;
    const int row_age = real_age ? age : 0;  // padded lanes read age 0's entries and use none of them
    const epi::RowLayout L{n, pb.nb, pb.nk};
    const double* row = a.values + (size_t)b * a.W;
    const double theta = row[epi::R_THETA], h_infec = row[L.vec(epi::V_H_INFEC, row_age)], a_i = row[L.vec(epi::V_A, row_age)];
    const double Ni = pb.N[age];
    const double* Mrow = pb.Mrow + (size_t)age * lpc;
    const size_t copy_ints = (size_t)J * STATE_INTS * lpc;
    auto slot = [&](int copy, int p, int c) { return l.state + (size_t)copy * copy_ints + ((size_t)p * STATE_INTS + c) * lpc + age; };

    for (int pass = 0; pass < passes; ++pass) {
        const int p = pass * G + group;
        if (p >= J) continue;
#pragma unroll
        for (int c = 0; c < epi::NUM_COMP; ++c) *slot(0, p, c) = real_age ? (int32_t)row[L.initial(c, row_age)] : 0;
        *slot(0, p, epi::NUM_COMP + 0) = real_age ? (int32_t)row[L.initial(epi::C_CUM_H, row_age)] : 0;
        *slot(0, p, epi::NUM_COMP + 1) = real_age ? (int32_t)row[L.initial(epi::C_CUM_ICU, row_age)] : 0;
        *slot(0, p, epi::NUM_COMP + 2) = real_age ? (int32_t)row[L.initial(epi::C_D, row_age)] : 0;
    }
    int cur = 0;
    bool resampled = false;
    double loglik = 0.0;  // lane 0's
    for (int k = 0; k < T; ++k) {
        const int t = k - pb.runup_offset;
        double oH = qnan, oICU = qnan, oD = qnan;
        if (t >= 0 && real_age) {
            const double* rec = pb.grid + ((size_t)k * lpc + age) * 4;  // {obs_H, obs_ICU, obs_D, times[k + 1]}
            oH = rec[0]; oICU = rec[1]; oD = rec[2];
        }
        const bool weighted = __syncthreads_or((pf::usable(oH) || pf::usable(oICU) || pf::usable(oD)) ? 1 : 0) != 0;
        double h = 0.0, t0 = 0.0;
        epi::AgeProbs q{};
        if (k > 0) {
            t0 = pb.times[k - 1];
            h = (pb.times[k] - t0) / (double)a.m;
            q = epi::age_probs(row, L, row_age, h);
        }
        for (int pass = 0; pass < passes; ++pass) {
            const int p = pass * G + group;
            const bool in_range = p < J, ok = in_range && real_age;
            const int from = in_range ? (resampled ? l.anc[p] : p) : 0;
            int32_t x[epi::NUM_COMP];
#pragma unroll
            for (int c = 0; c < epi::NUM_COMP; ++c) x[c] = ok ? *slot(cur, from, c) : 0;
            const int32_t prevH = ok ? *slot(cur, from, epi::NUM_COMP + 0) : 0, prevICU = ok ? *slot(cur, from, epi::NUM_COMP + 1) : 0,
                          prevD = ok ? *slot(cur, from, epi::NUM_COMP + 2) : 0;
            if (k > 0) {
                for (int j = 0; j < a.m; ++j) {
                    const double t_mid = t0 + ((double)j + 0.5) * h;
                    const double bk = epi::beta_kappa(row, L, pb.beta_ends, pb.kappa_ends, t_mid);
                    const double inf = epi::infectious_pressure(x, theta, h_infec, Ni);
                    double sum = 0.0;
                    for (int jj = 0; jj < n; ++jj) sum += Mrow[jj] * __shfl(inf, jj, lpc);
                    const double lambda = epi::force_of_infection(sum, bk, a_i);
                    epi::age_step(x, lambda, h, q, a.seed, b, (uint32_t)p, (uint32_t)((k - 1) * a.m + j), (uint32_t)age);
                }
            }
            if (in_range) {
#pragma unroll
                for (int c = 0; c < epi::NUM_COMP; ++c) *slot(cur ^ 1, p, c) = x[c];
                *slot(cur ^ 1, p, epi::NUM_COMP + 0) = x[epi::C_CUM_H];
                *slot(cur ^ 1, p, epi::NUM_COMP + 1) = x[epi::C_CUM_ICU];
                *slot(cur ^ 1, p, epi::NUM_COMP + 2) = x[epi::C_D];
            }
            if (weighted) {
                double term;
                if constexpr (NB)
                    term = pf::age_term(oH, oICU, oD, x[epi::C_CUM_H] - prevH, x[epi::C_CUM_ICU] - prevICU, x[epi::C_D] - prevD,
                                        pf::Dispersion{a.k_H, a.k_ICU, a.k_D});
                else
                    term = pf::age_term(oH, oICU, oD, x[epi::C_CUM_H] - prevH, x[epi::C_CUM_ICU] - prevICU, x[epi::C_D] - prevD);
                double lw = 0.0;
                for (int aa = 0; aa < n; ++aa) lw += __shfl(term, aa, lpc);
                if (in_range && age == 0) l.lw[p] = lw;
            }
        }
        cur ^= 1;
        resampled = false;
        if (weighted) {
            __syncthreads();
            double inc = 0.0, ess = qnan;
            block_normalise_and_resample(l, J, pf::resample_uniform(a.seed, b, (uint32_t)k), inc, ess);
            resampled = true;
            if (tid == 0) {
                if constexpr (NB) inc = pf::increment_with_constant(inc, a.row_const[t]);
                loglik += inc;
                if (a.increments != nullptr) a.increments[(size_t)b * Tp + t] = inc;
                if (a.ess != nullptr) a.ess[(size_t)b * Tp + t] = ess;
            }
        } else if (t >= 0 && tid == 0) {
            if (a.increments != nullptr) a.increments[(size_t)b * Tp + t] = 0.0;
            if (a.ess != nullptr) a.ess[(size_t)b * Tp + t] = qnan;
        }
    }
    if (tid == 0) a.loglik[b] = loglik;
    if (a.final_state != nullptr) {
        for (int pass = 0; pass < passes; ++pass) {
            const int p = pass * G + group;
            if (p >= J || !real_age) continue;
            const int from = resampled ? l.anc[p] : p;
            double* dst = a.final_state + (size_t)b * final_doubles + (size_t)p * epi::NUM_COMP * n + age;
#pragma unroll
            for (int c = 0; c < epi::NUM_COMP; ++c) dst[(size_t)c * n] = (double)*slot(cur, from, c);
        }
    }
}

// the probe: one row's normalisation and resampling through block_normalise_and_resample; out2 = {increment, ESS}
__global__ __launch_bounds__(PARTICLE_BLOCK) void particle_resample_probe_kernel(uint64_t seed, uint32_t b, uint32_t row, const double* logw, int J,
                                                                                 int32_t* ancestors, double* out2) {
    extern __shared__ double particle_lds[];
    const BlockLds l = carve(particle_lds, J);
    const int j = (int)threadIdx.x;
    if (j < J) l.lw[j] = logw[j];
    __syncthreads();
    double inc = 0.0, ess = 0.0;
    block_normalise_and_resample(l, J, pf::resample_uniform(seed, b, row), inc, ess);
    if (j < J) ancestors[j] = l.anc[j];
    if (j == 0) { out2[0] = inc; out2[1] = ess; }
}

// cells of the probe of pf::nb_term: one lane per cell, grid-stride
__global__ __launch_bounds__(256) void particle_nb_term_probe_kernel(const double* obs, const int32_t* inc, int count, double k, double* out) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < count; i += (int)(gridDim.x * blockDim.x)) out[i] = pf::nb_term(obs[i], inc[i], k);
}

template <bool NB, class Args>
int launch_filter(const DevProblem& pb, const Args& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Tp = pb.T - pb.runup_offset;
    if (a.B <= 0 || a.m < 1 || pb.n < 1 || pb.n > epi::MAX_AGES || pb.lpc < pb.n || pb.lpc > epi::MAX_AGES || (pb.lpc & (pb.lpc - 1)) != 0 ||
        Tp <= 0 || a.J < 1 || a.J > particle_max_particles_for(pb.lpc) || (uint64_t)pb.T * (uint64_t)a.m >= ((uint64_t)1 << 22) ||
        a.W != epi::RowLayout{pb.n, pb.nb, pb.nk}.width())
        return -4;
    const size_t lds = particle_lds_bytes(pb.lpc, a.J);
    if (lds > PARTICLE_LDS_LIMIT) return -4;
    hipLaunchKernelGGL(particle_filter_kernel<NB>, dim3((unsigned)a.B), dim3(PARTICLE_BLOCK), lds, st, pb, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int launch_particle_filter(const DevProblem& pb, const ParticleArgs& a, void* stream) { return launch_filter<false>(pb, a, stream); }

int launch_particle_filter_nb(const DevProblem& pb, const ParticleArgsNB& a, void* stream) {
    if (!a.row_const || !pf::any_dispersed(pf::Dispersion{a.k_H, a.k_ICU, a.k_D})) return -4;
    return launch_filter<true>(pb, a, stream);
}

}  // namespace sepaihrd

using namespace sepaihrd;

extern "C" int sepaihrd_particle_max_particles(int n_age) {
    if (n_age < 1 || n_age > sepaihrd_stoch_epi::MAX_AGES) return SEPAIHRD_E_INVALID_ARG;
    return particle_max_particles_for(lanes_per_chain(n_age));
}

extern "C" int sepaihrd_particle_validate(int B, int J, int steps_per_interval, int n_times, int T_pos, int n_age, char* err, int errlen) {
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, "particle_loglik: " + msg); return SEPAIHRD_E_INVALID_ARG; };
    if (B < 1) return refuse("B must be >= 1 (parameter vectors)");
    if (n_age < 1 || n_age > sepaihrd_stoch_epi::MAX_AGES) return refuse("n_age must lie in [1, 16]");
    const int J_max = sepaihrd_particle_max_particles(n_age);
    if (J < 1 || J > J_max)
        return refuse("J must lie in [1, " + std::to_string(J_max) + "] (particles per parameter vector: one workgroup's LDS holds them all)");
    if (const char* grid = stoch_epi_grid_refusal(steps_per_interval, n_times, T_pos, n_age)) return refuse(grid);
    return SEPAIHRD_OK;
}

extern "C" int sepaihrd_particle_resample_device(int device, uint64_t seed, uint32_t b, uint32_t row, const double* logw, int J, int32_t* ancestors,
                                                 double* increment, double* ess, char* err, int errlen) {
    if (!logw || !ancestors || !increment || !ess || J < 1 || J > PARTICLE_BLOCK) {
        set_err(err, errlen, "particle_resample_device: need logw, ancestors, increment, ess and J in [1, 512]");
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (const int drc = select_device(device, err, errlen)) return drc;
    Probe pr;
    const double* d_logw = pr.in(logw, (size_t)J);
    double* d_out2 = pr.out<double>(2);
    int32_t* d_anc = pr.out<int32_t>((size_t)J);
    double out2[2] = {0.0, 0.0};
    if (pr.ready()) {
        hipLaunchKernelGGL(particle_resample_probe_kernel, dim3(1), dim3(PARTICLE_BLOCK), particle_lds_bytes(0, J), nullptr, seed, b, row, d_logw, J,
                           d_anc, d_out2);
        pr.fetch(ancestors, d_anc, (size_t)J);
        pr.fetch(out2, d_out2, 2);
    }
    if (const int prc = pr.status("particle_resample_device", err, errlen)) return prc;
    *increment = out2[0];
    *ess = out2[1];
    return SEPAIHRD_OK;
}

extern "C" int sepaihrd_particle_nb_validate(const double* dispersion, char* err, int errlen) {
    const std::string refusal = pf::nb_refusal(dispersion);
    if (refusal.empty()) return SEPAIHRD_OK;
    set_err(err, errlen, "particle_nb: " + refusal);
    return SEPAIHRD_E_INVALID_ARG;
}

extern "C" int sepaihrd_particle_nb_term_device(int device, const double* obs, const int32_t* inc, int count, double k, double* out, char* err,
                                                int errlen) {
    if (!obs || !inc || !out || count < 1 || !(k >= pf::NB_K_MIN && k <= pf::NB_K_MAX)) {
        set_err(err, errlen, "particle_nb_term_device: need obs, inc, out, count >= 1 and a finite k in [1e-3, 1e6]");
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (const int drc = select_device(device, err, errlen)) return drc;
    Probe pr;
    const double* d_obs = pr.in(obs, (size_t)count);
    const int32_t* d_inc = pr.in(inc, (size_t)count);
    double* d_out = pr.out<double>((size_t)count);
    if (pr.ready()) {
        const unsigned blocks = (unsigned)std::min<size_t>(((size_t)count + 255) / 256, 1024);
        hipLaunchKernelGGL(particle_nb_term_probe_kernel, dim3(blocks), dim3(256), 0, nullptr, d_obs, d_inc, count, k, d_out);
        pr.fetch(out, d_out, (size_t)count);
    }
    return pr.status("particle_nb_term_device", err, errlen);
}
