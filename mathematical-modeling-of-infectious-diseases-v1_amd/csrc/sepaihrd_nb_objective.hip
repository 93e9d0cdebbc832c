// csrc/sepaihrd_nb_objective.hip -- the negative-binomial likelihood pass of the deterministic SEPAIHRD objective on gfx950
// (DESIGN.md section 6o).  The rule is csrc/sepaihrd_nb_objective.inc, the text the host twin compiles too.
//
// A context with a dispersed series integrates in a form that parks its daily increments (EvalOutputs::cum / wstatus, layout
// cum_index; EvalOutputs::force_split = FORCE_SPLIT_PARK_ONLY keeps the launch code from running its Poisson pass) and this
// pass takes the Poisson pass's place.  It depends on the increments only, so one build serves both arithmetic modes; all it
// takes from the context's arithmetic is whether a Poisson series' cell is one fma (NbDispersion::fused_poisson).
//   nb_ll_rows_kernel    one lane per (chain, output day), one wave per day and 64 adjacent chains: the lane walks the ages of
//                        its day in ascending order for the three series and writes the three row sums to rows[day][series][chain].
//                        A chain's ages are adjacent columns of `cum`: one vector load per series brings four of them, and the
//                        loads of a wave are contiguous.  The observations of a day are wave-uniform.  The chain's k come from theta through
//                        constrained_theta (or the context's fixed values); lgamma_pos(k) and log(k) are formed once per lane.
//   nb_ll_reduce_kernel  one lane per (chain, series) adds the rows in day order from 0.0; the first lane of each chain forms
//                        total = (H + ICU) + D, the status and ll_parts as the Poisson pass's reduce kernel does.
// There is one form for every batch size: no serial-walk branch.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_nb_objective.inc"
#include "sepaihrd_nb_objective_device.h"

namespace sepaihrd {
namespace {

#include "sepaihrd_dev_common.inc"  // log_pos and its LDS table, constrained_theta

namespace nb = sepaihrd_nb_objective;

constexpr int NB_DAYS_PER_BLOCK = 4;  // one wave per day, as the Poisson pass's terms kernel

// the increments of the LPC ages of one chain, one series, one day: adjacent doubles, aligned to their own size
template <int LPC>
__device__ __forceinline__ void load_ages(const double* p, double (&v)[LPC]) {
    if constexpr (LPC % 4 == 0) {
        SEP_UNROLL
        for (int a = 0; a < LPC; a += 4) {
            const double4 q = *reinterpret_cast<const double4*>(p + a);
            v[a] = q.x; v[a + 1] = q.y; v[a + 2] = q.z; v[a + 3] = q.w;
        }
    } else if constexpr (LPC == 2) {
        const double2 q = *reinterpret_cast<const double2*>(p);
        v[0] = q.x; v[1] = q.y;
    } else {
        v[0] = p[0];
    }
}

template <int LPC>
__global__ __launch_bounds__(WAVE * NB_DAYS_PER_BLOCK) void nb_ll_rows_kernel(const DevProblem pb, const double* __restrict__ theta, const int B,
                                                                              const EvalOutputs out, const NbDispersion disp, const int cum_chains) {
    const bool fused = disp.fused_poisson != 0;
    stage_log_table(threadIdx.x, WAVE * NB_DAYS_PER_BLOCK);
    __syncthreads();
    const int chain = blockIdx.x * WAVE + threadIdx.x % WAVE;
    const int k = pb.runup_offset + blockIdx.y * NB_DAYS_PER_BLOCK + threadIdx.x / WAVE;  // outputs before t = 0 carry no observation
    if (k >= pb.T || chain >= B) return;
    if (out.wstatus[chain] != 0) return;  // no value: the reduce kernel writes lowest() without reading this chain's rows
    const double* th = theta + (size_t)chain * pb.P;
    nb::SeriesK sk[3];
    SEP_UNROLL
    for (int s = 0; s < 3; ++s) sk[s] = nb::series_k(disp.src[s] >= 0 ? constrained_theta(pb, th, disp.src[s]) : disp.fixed[s]);
    const double* rec = pb.grid + (size_t)k * LPC * 4;  // {obs_H, obs_ICU, obs_D, t_{k+1}} of age a at rec[4 a]
    SEP_UNROLL
    for (int s = 0; s < 3; ++s) {
        const int comp = (s == 0) ? 1 : (s == 1) ? 2 : 0;  // cum rows are D, CumH, CumICU; series are H, ICU, D
        const double* p = out.cum + cum_index(pb.T, (size_t)chain * LPC, k, comp);
        double row = 0.0;
        // ages ascending, the first cell starting the sum; padded ages carry NaN observations: their cells are 0
        auto add = [&](int a, double increment) {
            const double sim = nb::sim_of(increment);
            const double c = nb::cell(rec[4 * a + s], sim, log_pos(sim), sk[s], fused);
            row = (a == 0) ? c : row + c;
        };
        constexpr int GROUP = LPC < 4 ? LPC : 4;  // the ages one vector load brings
        for (int a0 = 0; a0 < LPC; a0 += GROUP) {
            double inc[GROUP];
            load_ages<GROUP>(p + a0, inc);
            SEP_UNROLL
            for (int j = 0; j < GROUP; ++j) add(a0 + j, inc[j]);
        }
        out.rows[((size_t)k * 3 + s) * cum_chains + chain] = row;
    }
}

__global__ __launch_bounds__(WAVE) void nb_ll_reduce_kernel(const DevProblem pb, const int B, const EvalOutputs out, const int cum_chains) {
    // lane = 4 * chain_in_block + series (series 3 idles): 16 chains per wave
    const int lane = threadIdx.x;
    const int series = lane & 3;
    const int chain = blockIdx.x * 16 + (lane >> 2);
    const bool live = chain < B && series < 3;
    const int ch = chain < B ? chain : 0;
    const int status0 = out.wstatus[ch];
    double acc = 0.0;
    if (live && status0 == 0) {
        const double* src = out.rows + (size_t)series * cum_chains + ch;
        const size_t step = (size_t)3 * cum_chains;
        int k = pb.runup_offset;
        constexpr int IN_FLIGHT = 16;  // the additions are a dependent chain, the loads are not
        for (; k + IN_FLIGHT <= pb.T; k += IN_FLIGHT) {
            double v[IN_FLIGHT];
            SEP_UNROLL
            for (int j = 0; j < IN_FLIGHT; ++j) v[j] = src[(size_t)(k + j) * step];
            SEP_UNROLL
            for (int j = 0; j < IN_FLIGHT; ++j) acc += v[j];
        }
        for (; k < pb.T; ++k) acc += src[(size_t)k * step];
    }
    const int base = lane & ~3;
    const double h = __shfl(acc, base), i = __shfl(acc, base + 1), d = __shfl(acc, base + 2);
    if (!(chain < B) || series != 0) return;
    int status = status0;
    double total = (h + i) + d;
    if (status == 0 && (isnan(total) || isinf(total))) status = 1;
    if (status != 0) total = -DBL_MAX;
    out.loglik[chain] = total;
    if (out.status) out.status[chain] = status;
    if (out.ll_parts) {
        const bool ok = status0 == 0;
        out.ll_parts[3 * chain + 0] = ok ? h : 0.0;
        out.ll_parts[3 * chain + 1] = ok ? i : 0.0;
        out.ll_parts[3 * chain + 2] = ok ? d : 0.0;
    }
}

__global__ __launch_bounds__(256) void lgamma_probe_kernel(const double* x, int n, double* out) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) out[i] = sepaihrd_lgamma::lgamma_pos(x[i]);
}

template <int LPC>
int launch_pass(const DevProblem& pb, const double* d_theta, int B, const EvalOutputs& out, const NbDispersion& disp, hipStream_t st) {
    constexpr int CPW = WAVE / LPC;
    const int cum_chains = (B + CPW - 1) / CPW * CPW;  // the stride the integrator's launch gave the parked columns
    const int days = pb.T - pb.runup_offset;
    if (days > 0)
        hipLaunchKernelGGL((nb_ll_rows_kernel<LPC>), dim3((unsigned)((B + WAVE - 1) / WAVE), (unsigned)((days + NB_DAYS_PER_BLOCK - 1) / NB_DAYS_PER_BLOCK)),
                           dim3(WAVE * NB_DAYS_PER_BLOCK), 0, st, pb, d_theta, B, out, disp, cum_chains);
    hipLaunchKernelGGL(nb_ll_reduce_kernel, dim3((unsigned)((B + 15) / 16)), dim3(WAVE), 0, st, pb, B, out, cum_chains);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <int LPC>
int info_pass(LaunchInfo* info) {
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&nb_ll_rows_kernel<LPC>)) != hipSuccess) return -3;
    info->vgprs = attr.numRegs;
    info->sgprs = 0;
    info->lds_static = (int)attr.sharedSizeBytes;
    info->lds_dynamic = 0;
    info->scratch = (int)attr.localSizeBytes;
    int nb_blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb_blocks, nb_ll_rows_kernel<LPC>, WAVE * NB_DAYS_PER_BLOCK, 0) != hipSuccess) nb_blocks = -1;
    info->max_blocks_per_cu = nb_blocks;
    info->lanes_per_chain = LPC;
    info->likelihood_form = LL_FORM_SEPARATE_PASS;
    info->name = NB_PASS_KERNEL_NAME;
    return 0;
}

}  // namespace

int launch_nb_objective_pass(const DevProblem& pb, const double* d_theta, int B, const EvalOutputs& out, const NbDispersion& disp, void* stream) {
    if (B <= 0) return 0;
    if (out.cum == nullptr || out.rows == nullptr || out.wstatus == nullptr || out.loglik == nullptr || d_theta == nullptr) return -5;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (pb.lpc) {
        case 1: return launch_pass<1>(pb, d_theta, B, out, disp, st);
        case 2: return launch_pass<2>(pb, d_theta, B, out, disp, st);
        case 4: return launch_pass<4>(pb, d_theta, B, out, disp, st);
        case 8: return launch_pass<8>(pb, d_theta, B, out, disp, st);
        case 16: return launch_pass<16>(pb, d_theta, B, out, disp, st);
        default: return -4;
    }
}

int kernel_info_nb_pass(const DevProblem& pb, LaunchInfo* info) {
    switch (pb.lpc) {
        case 1: return info_pass<1>(info);
        case 2: return info_pass<2>(info);
        case 4: return info_pass<4>(info);
        case 8: return info_pass<8>(info);
        case 16: return info_pass<16>(info);
        default: return -4;
    }
}

}  // namespace sepaihrd

using namespace sepaihrd;
namespace nbo = sepaihrd_nb_objective;

extern "C" int sepaihrd_dispersion_validate(int n_params, const int32_t* param_field, const int32_t* param_index, const double* lower,
                                            const double* upper, const uint8_t* has_bounds, int32_t* series_param, char* err, int errlen) {
    if (n_params < 0 || (n_params > 0 && (!param_field || !param_index))) {
        set_err(err, errlen, "dispersion: param_field and param_index are required");
        return SEPAIHRD_E_INVALID_ARG;
    }
    int32_t src[3] = {-1, -1, -1};
    for (int p = 0; p < n_params; ++p) {
        if (param_field[p] != SEPAIHRD_F_DISPERSION) continue;
        const std::string who = "param " + std::to_string(p) + ": ";
        auto refuse = [&](const std::string& what) { set_err(err, errlen, who + what); return SEPAIHRD_E_INVALID_ARG; };
        const int s = param_index[p];
        if (s < 0 || s > 2) return refuse("dispersion index out of range (0 = H, 1 = ICU, 2 = D)");
        const std::string name = std::string("dispersion of series ") + (s == 0 ? "H" : s == 1 ? "ICU" : "D");
        if (src[s] >= 0) return refuse(name + " is already calibrated by param " + std::to_string(src[s]));
        const bool has = has_bounds ? has_bounds[p] != 0 : (lower && upper);
        if (!has || !lower || !upper) return refuse(name + " needs bounds: a calibrated k must stay finite in [1e-3, 1e6]");
        if (!(lower[p] >= nbo::K_MIN && lower[p] <= upper[p] && upper[p] <= nbo::K_MAX)) {
            char val[96];
            std::snprintf(val, sizeof(val), "[%.17g, %.17g]", lower[p], upper[p]);
            return refuse(name + " has bounds " + val + ": they must satisfy 1e-3 <= lower <= upper <= 1e6");
        }
        src[s] = p;
    }
    if (series_param)
        for (int s = 0; s < 3; ++s) series_param[s] = src[s];
    return SEPAIHRD_OK;
}

extern "C" int sepaihrd_nb_objective_host(const double* increments, const double* obs_H, const double* obs_ICU, const double* obs_D, const double* k,
                                          int B, int T, int n_age, double* loglik, double* ll_parts, int32_t* status) {
    if (!increments || !obs_H || !obs_ICU || !obs_D || !k || !loglik || B < 0 || T < 0 || n_age < 1) return SEPAIHRD_E_INVALID_ARG;
    const size_t Tn = (size_t)T * n_age;
    std::vector<double> obs(3 * Tn);
    std::copy(obs_H, obs_H + Tn, obs.begin());
    std::copy(obs_ICU, obs_ICU + Tn, obs.begin() + Tn);
    std::copy(obs_D, obs_D + Tn, obs.begin() + 2 * Tn);
    for (int b = 0; b < B; ++b) {
        double parts[3];
        const int st = nbo::chain_loglik(increments + (size_t)b * 3 * Tn, obs.data(), k + 3 * (size_t)b, T, n_age,
                                         [](double sim) { return std::log(sim); }, loglik + b, parts);
        if (status) status[b] = st;
        if (ll_parts)
            for (int s = 0; s < 3; ++s) ll_parts[3 * (size_t)b + s] = parts[s];
    }
    return SEPAIHRD_OK;
}

extern "C" double sepaihrd_lgamma_host(double x) { return sepaihrd_lgamma::lgamma_pos(x); }

extern "C" int sepaihrd_lgamma_device(int device, const double* x, int n, double* out, char* err, int errlen) {
    if (!x || !out || n < 1) {
        set_err(err, errlen, "lgamma_device: need x, out and n >= 1");
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (const int drc = select_device(device, err, errlen)) return drc;
    Probe pr;
    const double* d_x = pr.in(x, (size_t)n);
    double* d_out = pr.out<double>((size_t)n);
    if (pr.ready()) {
        const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n + 255) / 256, 1024);
        hipLaunchKernelGGL(lgamma_probe_kernel, dim3(blocks), dim3(256), 0, nullptr, d_x, n, d_out);
        pr.fetch(out, d_out, (size_t)n);
    }
    return pr.status("lgamma_device", err, errlen);
}
