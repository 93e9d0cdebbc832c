// csrc/sepaihrd_stoch_sepaihrd.hip -- stochastic chain-binomial SEPAIHRD ensembles over posterior samples on gfx950
// (sepaihrd_ensemble_stochastic): the decode kernel (theta -> model values, rounded initial state, status)
// and the step kernel.  The model, its stream coordinates and the walk through one output interval (lane_interval) are
// csrc/sepaihrd_stoch_sepaihrd.inc, the text the host twin compiles too; the constraint rule of the decode is
// csrc/sepaihrd_constrain.inc, the text of every other kernel and of the host; the segment sorts and the quantiles are csrc/sepaihrd_ensemble.hip's.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_stoch_sepaihrd.inc"
#include "sepaihrd_stoch_sepaihrd_device.h"

namespace sepaihrd {
namespace {

namespace epi = sepaihrd_stoch_epi;

constexpr int STEP_BLOCK = 256;

#include "sepaihrd_constrain.inc"  // slot_scalar, slot_vec: theta decoded under the text the evaluation kernels compile

// One thread per sample: the row of model values after the constraints of the context's mode, the initial state by the
// context's initial-state rule (csrc/sepaihrd_kernels.hip, section 3 of its prologue) rounded entry by entry, and the status.
__global__ __launch_bounds__(256) void stoch_epi_decode_kernel(const DevProblem pb, const StochEpiArgs a) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= a.S) return;
    const double* th = a.theta + (size_t)s * pb.P;
    const int n = pb.n, lpc = pb.lpc;
    auto scalar_slot = [&](int slot) { return slot_scalar(pb, th, slot); };
    const epi::RowLayout L{n, pb.nb, pb.nk};
    double* row = a.values + (size_t)s * a.W;
    row[epi::R_THETA] = scalar_slot(SS_THETA);
    row[epi::R_SIGMA] = scalar_slot(SS_SIGMA);
    row[epi::R_GAMMA_P] = scalar_slot(SS_GAMMA_P);
    row[epi::R_GAMMA_A] = scalar_slot(SS_GAMMA_A);
    row[epi::R_GAMMA_I] = scalar_slot(SS_GAMMA_I);
    row[epi::R_GAMMA_H] = scalar_slot(SS_GAMMA_H);
    row[epi::R_GAMMA_ICU] = scalar_slot(SS_GAMMA_ICU);
    row[epi::R_BETA] = scalar_slot(SS_BETA);
    for (int k = 0; k < pb.nb; ++k) row[L.beta_values() + k] = scalar_slot(SS_SCHEDULE0 + k);
    for (int k = 0; k < pb.nk; ++k) row[L.kappa_values() + k] = scalar_slot(SS_SCHEDULE0 + pb.nb + k);
    for (int f = 0; f < VF_COUNT; ++f)
        for (int i = 0; i < n; ++i) row[L.vec(f, i)] = slot_vec(pb, th, f, i);

    int status = 0;
    if (pb.kappa_calibrated)
        for (int k = 1; k < pb.nk; ++k)
            if (scalar_slot(SS_SCHEDULE0 + pb.nb + k) < 0.0) status = 1;
    if (!pb.obs_rows_match && pb.init_mode == 0) status = 1;
    const double runup_days = scalar_slot(SS_RUNUP_DAYS), seed_exposed = scalar_slot(SS_SEED_EXPOSED);
    const bool seeded = pb.init_mode == 0 && runup_days > 0 && seed_exposed > 0;
    for (int i = 0; i < n; ++i) {
        double x[NUM_COMP];
        for (int c = 0; c < NUM_COMP; ++c) x[c] = pb.init_state[c * lpc + i];
        if (pb.init_mode != 1) {
            if (seeded) {
                x[1] = seed_exposed * pb.age_fraction[i];
                for (int c = 2; c < NUM_COMP; ++c) x[c] = 0.0;
            } else {
                for (int c = 1; c <= 8; ++c) x[c] *= scalar_slot(SS_E0_MULT + (c - 1));
            }
            const double Ni = pb.N[i];
            double sum = 0;
            for (int c = 1; c < NUM_POP_COMP; ++c) sum += x[c];
            if (sum > Ni || (pb.init_mode == 2 && sum < 0)) status = 1;
            x[0] = Ni - sum;
        }
        for (int c = 0; c < NUM_COMP; ++c) {
            const double r = round(x[c]);
            if (!epi::count_in_range(r)) status = 1;
            row[L.initial(c, i)] = r;
        }
    }
    a.status[s] = status;
}

// counts[0] = valid samples, counts[1] = valid samples x R
__global__ __launch_bounds__(256) void stoch_epi_count_kernel(const int32_t* status, int S, int R, int32_t* counts) {
    __shared__ int part[256];
    int c = 0;
    for (int s = threadIdx.x; s < S; s += 256) c += (status[s] == 0);
    part[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) { counts[0] = part[0]; counts[1] = part[0] * R; }
}

// One lane per (sample s, replicate r, age class): the lpc lanes of a replicate are adjacent, consecutive replicates follow
// along s R + r.  The 11 counts of the lane's age class stay in registers through the whole time loop; per step the lanes of a
// replicate exchange their infectious pressure through __shfl for the contact sum, then every lane makes its 13 draws.  Lanes of
// padded ages, of invalid samples and of the padding slots carry zero counts: they take part in the exchange, draw nothing
// (binomial(0, .) returns at once) and store +inf / NaN where a slot is theirs to fill.
__global__ __launch_bounds__(STEP_BLOCK) void stoch_epi_step_kernel(const DevProblem pb, const StochEpiArgs a) {
    const int n = pb.n, lpc = pb.lpc, T = pb.T, Tp = pb.T - pb.runup_offset;
    const size_t gl = (size_t)blockIdx.x * STEP_BLOCK + threadIdx.x;
    if (gl >= (size_t)a.N_pad * lpc) return;  // whole wavefronts: N_pad is a multiple of 64
    const size_t idx = gl / (size_t)lpc;      // the slot s R + r
    const int age = (int)(gl % (size_t)lpc);
    const bool in_range = idx < (size_t)a.S * a.R;
    const size_t s = in_range ? idx / (size_t)a.R : 0;
    const uint32_t r = (uint32_t)(idx % (size_t)a.R);
    const bool real_age = age < n;
    const bool ok = in_range && real_age && a.status[s] == 0;
    const int row_age = real_age ? age : 0;  // padded lanes read age 0's entries and use none of them
    const epi::RowLayout L{n, pb.nb, pb.nk};
    const double* row = a.values + s * (size_t)a.W;
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    const unsigned long long group_mask = (lpc == WAVE ? ~0ull : ((1ull << lpc) - 1ull)) << (lane & ~(lpc - 1));

    int32_t x[epi::NUM_COMP];
#pragma unroll
    for (int c = 0; c < epi::NUM_COMP; ++c) x[c] = ok ? (int32_t)row[L.initial(c, row_age)] : 0;
    const epi::LaneConstants lc = epi::lane_constants(row, L, pb.N, pb.Mrow, lpc, age);  // after the counts: before them, one SGPR spill more
    const double qnan = __builtin_nan("");
    const double pinf = __builtin_inf();
    const size_t seg_stride = (size_t)a.N_pad, cum_block = (size_t)3 * Tp * n;
    const bool want_traj = a.traj != nullptr && in_range && real_age && r < (uint32_t)a.keep;
    double* traj = want_traj ? a.traj + ((s * (size_t)a.keep + r) * T) * (size_t)(epi::NUM_COMP * n) + age : nullptr;

    int32_t prev[epi::NUM_PREV] = {x[epi::C_CUM_H], x[epi::C_CUM_ICU], x[epi::C_D]};
    double run[3] = {0.0, 0.0, 0.0};
    auto write_row = [&](int k) {
        if (want_traj) {
            double* dst = traj + (size_t)k * (epi::NUM_COMP * n);
#pragma unroll
            for (int c = 0; c < epi::NUM_COMP; ++c) dst[(size_t)c * n] = ok ? (double)x[c] : qnan;
        }
        int32_t since[epi::NUM_PREV];
        epi::take_increments(x, prev, since);
        const double inc[3] = {(double)since[0], (double)since[1], (double)since[2]};
        const int t = k - pb.runup_offset;
        if (t < 0 || !real_age) return;
#pragma unroll
        for (int ser = 0; ser < 3; ++ser) {
            run[ser] += inc[ser];
            const size_t cell = ((size_t)ser * Tp + t) * n + age;
            a.vals[cell * seg_stride + idx] = ok ? inc[ser] : pinf;
            a.vals[(cell + cum_block) * seg_stride + idx] = ok ? run[ser] : pinf;
        }
    };
    write_row(0);
    for (int k = 0; k + 1 < T; ++k) {
        const double t0 = pb.times[k];
        const double h = (pb.times[k + 1] - t0) / (double)a.m;
        const epi::AgeProbs q = epi::age_probs(row, L, row_age, h);
        epi::lane_interval(x, row, L, lc, pb.beta_ends, pb.kappa_ends, t0, h, q, a.m, a.seed, (uint32_t)s, r, (uint32_t)(k * a.m), (uint32_t)age,
                           [lpc](double inf, int jj) { return __shfl(inf, jj, lpc); });
        write_row(k + 1);
    }
    if (a.final_state != nullptr && in_range && real_age) {
        double* dst = a.final_state + idx * (size_t)(epi::NUM_COMP * n) + age;
#pragma unroll
        for (int c = 0; c < epi::NUM_COMP; ++c) dst[(size_t)c * n] = ok ? (double)x[c] : qnan;
    }
    const bool infected = (x[epi::C_E] | x[epi::C_P] | x[epi::C_A] | x[epi::C_I]) != 0;  // counts are >= 0
    const bool any_infected = (__ballot(infected) & group_mask) != 0ull;
    if (ok && age == 0 && !any_infected) atomicAdd(a.extinct_count + s, 1);
}

}  // namespace

int launch_stoch_epi_decode(const DevProblem& pb, const StochEpiArgs& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.S <= 0 || a.R <= 0 || a.W != epi::RowLayout{pb.n, pb.nb, pb.nk}.width()) return -4;
    hipLaunchKernelGGL(stoch_epi_decode_kernel, dim3((unsigned)((a.S + 255) / 256)), dim3(256), 0, st, pb, a);
    hipLaunchKernelGGL(stoch_epi_count_kernel, dim3(1), dim3(256), 0, st, a.status, a.S, a.R, a.counts);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_stoch_epi_steps(const DevProblem& pb, const StochEpiArgs& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Tp = pb.T - pb.runup_offset;
    if (a.S <= 0 || a.R <= 0 || a.m < 1 || a.keep < 0 || a.keep > a.R || pb.n < 1 || pb.n > epi::MAX_AGES || pb.lpc > epi::MAX_AGES ||
        Tp <= 0 || (size_t)a.S * a.R > (size_t)a.N_pad || a.N_pad % WAVE != 0 || (uint64_t)pb.T * (uint64_t)a.m >= ((uint64_t)1 << 22))
        return -4;
    const size_t lanes = (size_t)a.N_pad * pb.lpc;
    const size_t blocks = (lanes + STEP_BLOCK - 1) / STEP_BLOCK;
    if (blocks >= ((size_t)1 << 31)) return -4;
    if (hipMemsetAsync(a.extinct_count, 0, (size_t)a.S * sizeof(int32_t), st) != hipSuccess) return -3;
    hipLaunchKernelGGL(stoch_epi_step_kernel, dim3((unsigned)blocks), dim3(STEP_BLOCK), 0, st, pb, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

const char* stoch_epi_grid_refusal(int steps_per_interval, int n_times, int T_pos, int n_age) {
    if (steps_per_interval < 1) return "steps_per_interval must be >= 1";
    if (n_times < 1 || T_pos < 1 || T_pos > n_times) return "need n_times >= T_pos >= 1 (an output time >= 0)";
    if (n_age < 1) return "n_age must be >= 1";
    if ((uint64_t)n_times * (uint64_t)steps_per_interval >= ((uint64_t)1 << 22))
        return "n_times x steps_per_interval must stay below 2^22 (the third stream coordinate)";
    return nullptr;
}

}  // namespace sepaihrd

using namespace sepaihrd;

extern "C" int sepaihrd_stochastic_values_width(int n_age, int n_beta, int n_kappa) {
    if (n_age < 1 || n_beta < 0 || n_kappa < 0) return SEPAIHRD_E_INVALID_ARG;
    return sepaihrd_stoch_epi::RowLayout{n_age, n_beta, n_kappa}.width();
}

extern "C" int sepaihrd_stochastic_validate(int S, int R, int steps_per_interval, int keep, int n_times, int T_pos, int n_age,
                                            const double* probs, int n_probs, char* err, int errlen) {
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, "ensemble_stochastic: " + msg); return SEPAIHRD_E_INVALID_ARG; };
    if (S < 1) return refuse("S must be >= 1 (samples)");
    if (R < 1) return refuse("R must be >= 1 (replicates per sample)");
    if (keep < 0 || keep > R) return refuse("keep must lie in [0, R]");
    const uint64_t N = (uint64_t)S * (uint64_t)R;
    if (N >= ((uint64_t)1 << 31) || (N + WAVE - 1) / WAVE * WAVE >= ((uint64_t)1 << 31))
        return refuse("S x R rounded up to whole wavefronts must stay below 2^31 (replicates per segment)");
    if (const char* grid = stoch_epi_grid_refusal(steps_per_interval, n_times, T_pos, n_age)) return refuse(grid);
    if (!probs || n_probs < 1 || n_probs > 1024) return refuse("need probs (1..1024)");
    for (int p = 0; p < n_probs; ++p)
        if (!(probs[p] >= 0.0 && probs[p] <= 1.0)) return refuse("probabilities must lie in [0, 1]");
    return SEPAIHRD_OK;
}
