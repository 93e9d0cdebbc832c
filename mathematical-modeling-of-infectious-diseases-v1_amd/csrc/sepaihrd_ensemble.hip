// =============================================================================
// csrc/sepaihrd_ensemble.hip -- posterior-ensemble summaries on gfx950.
//
// Second consumer of the integrator: one simulation per stored
// posterior sample, then per-time quantiles across the samples.
//
// Reference behaviour followed (paths under /root/reference):
//   series     src/model/ResultAggregator.cpp:297-345   daily = max(0, X(t) - X(t_prev)) for the
//              output times t >= 0 (previous point = last run-up point or the initial state),
//              cumulative = running sum of the daily values in time order; X in {CumH, CumICU, D}
//   sero       src/model/MetricsCalculator.cpp:199-226  (sum N - sum_a S_a(t)) / sum N, every time
//   Rt         src/model/ReproductionNumberCalculator.cpp:55-171  spectral radius of F V^-1 (below)
//   quantile   src/model/PostCalibrationAnalyser.cpp:303-340  exact sort, then the rule of csrc/sepaihrd_quantile.inc
// The reference feeds the six incidence series through Boost.Accumulators' P^2 estimator
// (ResultAggregator.cpp:226-244, order-dependent, third-party); here every series uses the exact
// sort rule of PostCalibrationAnalyser, as SURVEY 8f prescribes.
//
// Layout: the integrator leaves the increments in cum[T][3][S*lpc] (sample-major columns).  Pass 1
// (one lane per (sample, age)) walks the days and writes every series value into
// vals[segment][S_pad] with the SAMPLE index contiguous, so that pass 2 (one workgroup per segment)
// loads its segment coalesced, sorts it in LDS (bitonic, up to 16384 doubles = 128 KiB) and
// interpolates the quantiles.  Samples whose integration failed are +inf and sort to the end; the
// quantile positions use the count of valid samples.  How a segment is padded and when it is sorted
// in global memory instead: csrc/sepaihrd_segments.h; the one dispatch (sort_segments_and_pick), the one kernel pair
// (segment_sort_pick_kernel, segment_pick_sorted_kernel) and the one launcher (launch_sort_pick), with their scored forms, are
// the text of csrc/sepaihrd_segment_sort.inc, which every summary here instantiates with its own pick: EnsemblePick,
// ScenarioPick, StochSirPick.
// Compiled with -ffp-contract=off: the interpolation is the CPU build's operation sequence.
// =============================================================================
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cstring>

#include "sepaihrd_device.h"
#include "sepaihrd_predictive_device.h"
#include "sepaihrd_segment_sort.inc"
#include "sepaihrd_sir_device.h"
#include "sepaihrd_stoch_device.h"
#include "sepaihrd_stoch.inc"

namespace sepaihrd {
namespace {

__global__ __launch_bounds__(256) void ensemble_count_valid_kernel(const int32_t* wstatus, int S, int32_t* n_valid) {
    __shared__ int part[256];
    int c = 0;
    for (int s = threadIdx.x; s < S; s += 256) c += (wstatus[s] == 0);
    part[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_valid = part[0];
}

// Pass 1: lane = (sample, age) column of the integrator workspace.
__global__ __launch_bounds__(WAVE) void ensemble_series_kernel(const EnsembleArgs a) {
    const size_t col = (size_t)blockIdx.x * WAVE + threadIdx.x;
    const int s = (int)(col / a.lpc);
    const int age = (int)(col % a.lpc);
    if (s >= a.S_pad || age >= a.n) return;
    const bool ok = s < a.S && a.wstatus[s] == 0;
    const double inf = INFINITY;
    const size_t seg_stride = (size_t)a.S_pad;
    // series order: daily H, daily ICU, daily D, cumulative H, cumulative ICU, cumulative D
    // cum rows are D, CumH, CumICU
    const int comp_of[3] = {1, 2, 0};
    double run[3] = {0.0, 0.0, 0.0};
    // the running sums are a dependent chain, the loads are not: 8 days are requested at a time
    constexpr int DAYS = 8;
    for (int t0 = 0; t0 < a.Tp; t0 += DAYS) {
        double inc[DAYS][3];
#pragma unroll
        for (int d = 0; d < DAYS; ++d) {
            const size_t k = (size_t)(a.runup_offset + (t0 + d < a.Tp ? t0 + d : a.Tp - 1));
#pragma unroll
            for (int ser = 0; ser < 3; ++ser) inc[d][ser] = ok ? a.cum[cum_index(a.T, col, k, comp_of[ser])] : 0.0;
        }
#pragma unroll
        for (int d = 0; d < DAYS; ++d) {
            const int t = t0 + d;
            if (t >= a.Tp) break;
#pragma unroll
            for (int ser = 0; ser < 3; ++ser) {
                double daily = inf, cumulative = inf;
                if (ok) {
                    daily = (0.0 < inc[d][ser]) ? inc[d][ser] : 0.0;  // std::max(0.0, cur - prev)
                    run[ser] = (t == 0) ? daily : run[ser] + daily;   // row(t) = row(t-1) + daily.row(t)
                    cumulative = run[ser];
                }
                a.vals[(((size_t)ser * a.Tp + t) * a.n + age) * seg_stride + s] = daily;
                a.vals[(((size_t)(ser + 3) * a.Tp + t) * a.n + age) * seg_stride + s] = cumulative;
            }
        }
    }
    if (a.traj != nullptr && a.sero_out != nullptr && age == 0) {
        double* sero = a.vals + (size_t)6 * a.Tp * a.n * seg_stride;
        for (int k = 0; k < a.T; ++k) {
            double v = inf;
            if (ok) {
                const double* row = a.traj + ((size_t)s * a.T + k) * (NUM_COMP * a.n);  // S block first
                double tot = 0.0;
                for (int j = 0; j < a.n; ++j) tot += row[j];
                v = (a.total_pop - tot) / a.total_pop;
            }
            sero[(size_t)k * seg_stride + s] = v;
        }
    }
}

#include "sepaihrd_constrain.inc"  // slot_scalar, slot_vec: theta decoded under the text the evaluation kernels compile

// Effective reproduction number of sample s at output time k
// (ReproductionNumberCalculator::calculateRt, src/model/ReproductionNumberCalculator.cpp:55-92,95-171):
// spectral radius of the next-generation matrix K = F V^-1 over the states (E, P, A, I) x age.
// F has entries only in its E rows: F(E_i, {P_j, A_j}) = T_ij, F(E_i, I_j) = theta T_ij with
// T_ij = max(0, beta(t) kappa(t) M_ij a_i h_infec_j S_i / N_j); V is block lower-triangular
// (sigma, gamma_p, p gamma_p, (1-p) gamma_p, gamma_A, gamma_I + h), so V^-1 restricted to the E columns is
// closed form and the non-zero spectrum of K is that of the n x n block
//   K_EE(i, j) = T_ij (1/gamma_p + p_j/gamma_A + theta (1 - p_j)/(gamma_I + h_j)).
// K_EE is non-negative: its spectral radius is its Perron root, taken by power iteration in the
// max-norm (the reference calls Eigen::EigenSolver on the full 4n x 4n matrix: same number to rounding).
constexpr int RT_MAX_AGE = 16;
__global__ __launch_bounds__(WAVE) void ensemble_rt_kernel(const EnsembleArgs a, const DevProblem pb, const double* theta) {
    const size_t idx = (size_t)blockIdx.x * WAVE + threadIdx.x;
    const int s = (int)(idx % a.S_pad);  // sample fastest: the segment row is written coalesced
    const int k = (int)(idx / a.S_pad);
    if (k >= a.T) return;
    double* out = a.vals + ((size_t)a.rt_segment0 + k) * a.S_pad;
    if (!(s < a.S && a.wstatus[s] == 0)) { out[s] = INFINITY; return; }
    const double* th = theta + (size_t)s * pb.P;
    const int n = a.n;
    const double t = pb.times[k];
    int seg = 0;
    for (int j = 0; j < pb.nm; ++j) seg += (pb.mends[j] < t) ? 1 : 0;
    const double beta = (pb.nb > 0) ? slot_scalar(pb, th, SS_SCHEDULE0 + pb.seg_ib[seg]) : slot_scalar(pb, th, SS_BETA);
    const double kappa = slot_scalar(pb, th, SS_SCHEDULE0 + pb.nb + pb.seg_ik[seg]);
    const double theta_i = slot_scalar(pb, th, SS_THETA);
    const double gamma_p = slot_scalar(pb, th, SS_GAMMA_P), gamma_A = slot_scalar(pb, th, SS_GAMMA_A),
                 gamma_I = slot_scalar(pb, th, SS_GAMMA_I);
    const double* row = a.traj + ((size_t)s * a.T + k) * (NUM_COMP * n);  // S block first
    double ci[RT_MAX_AGE], gj[RT_MAX_AGE], v[RT_MAX_AGE], w[RT_MAX_AGE];
    for (int i = 0; i < n; ++i) {
        ci[i] = beta * kappa * slot_vec(pb, th, VF_A, i) * row[i];  // beta kappa a_i S_i
        const double Nj = pb.N[i];
        const double pj = slot_vec(pb, th, VF_P, i), hj = slot_vec(pb, th, VF_H, i);
        const double dwell = 1.0 / gamma_p + pj / gamma_A + theta_i * (1.0 - pj) / (gamma_I + hj);
        gj[i] = (Nj < 1e-9) ? 0.0 : slot_vec(pb, th, VF_H_INFEC, i) / Nj * dwell;
        v[i] = 1.0;
    }
    double lambda = 0.0;
    for (int it = 0; it < 2000; ++it) {
        double m = 0.0;
        for (int i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int j = 0; j < n; ++j) {
                const double tij = ci[i] * pb.Mrow[i * pb.lpc + j] * gj[j];
                acc += ((0.0 < tij) ? tij : 0.0) * v[j];
            }
            w[i] = acc;
            m = (acc > m) ? acc : m;
        }
        if (!(m > 0.0)) { lambda = 0.0; break; }
        for (int i = 0; i < n; ++i) v[i] = w[i] / m;
        const bool done = fabs(m - lambda) <= 1e-15 * m;
        lambda = m;
        if (done) break;
    }
    out[s] = lambda;
}

// Per-sample summary metrics, one thread per sample
// (MetricsCalculator::calculateEssentialMetrics, src/model/MetricsCalculator.cpp:8-170).  Row layout:
//   [0] R0  [1] overall_IFR  [2] overall_attack_rate  [3] peak_hospital  [4] peak_ICU
//   [5] time_to_peak_hospital  [6] time_to_peak_ICU  [7] total_deaths  [8] max_Rt  [9] min_Rt  [10] final_Rt
//   [11] seroprevalence at the output time closest to day 64, then per age: IFR, IHR, IICUR, attack rate
// Quirks kept: cumulative infections = the non-S part of the initial state + sum_t lambda_t S_t dt with
// lambda_t = beta kappa(t) M (P + A + theta I)/N using the CONSTANT beta (no schedule, no a_i, no h_infec) and
// dt = 1 for the first time point (:103-113); max_Rt starts at 0, min_Rt at 1e6 (AnalysisTypes.hpp:26-27);
// peaks move on strict ">" only (:91-98); ratios need more than one infection and are clipped to [0, 1]
// (:139-157).  R0 = spectral radius of F V^-1 with S = N, beta(0), kappa(0) and no clipping of F (:22-52).
constexpr int METRIC_SCALARS = 12;
__global__ __launch_bounds__(WAVE) void ensemble_metrics_kernel(const EnsembleArgs a, const DevProblem pb, const double* theta) {
    const int s = blockIdx.x * WAVE + threadIdx.x;
    if (s >= a.S) return;
    const int n = a.n, width = METRIC_SCALARS + 4 * n;
    double* out = a.metrics_out + (size_t)s * width;
    if (a.wstatus[s] != 0) {
        for (int i = 0; i < width; ++i) out[i] = NAN;
        return;
    }
    const double* th = theta + (size_t)s * pb.P;
    const double beta_c = slot_scalar(pb, th, SS_BETA), theta_i = slot_scalar(pb, th, SS_THETA);
    const double gamma_p = slot_scalar(pb, th, SS_GAMMA_P), gamma_A = slot_scalar(pb, th, SS_GAMMA_A),
                 gamma_I = slot_scalar(pb, th, SS_GAMMA_I);
    const double* traj = a.traj + (size_t)s * a.T * (NUM_COMP * n);
    const double* rt = a.vals + (size_t)a.rt_segment0 * a.S_pad + s;  // Rt(s, k) at stride S_pad
    double total_pop = 0.0;
    for (int i = 0; i < n; ++i) total_pop += pb.N[i];

    // R0
    double r0 = 0.0;
    {
        int seg = 0;
        for (int j = 0; j < pb.nm; ++j) seg += (pb.mends[j] < 0.0) ? 1 : 0;
        const double beta0 = (pb.nb > 0) ? slot_scalar(pb, th, SS_SCHEDULE0 + pb.seg_ib[seg]) : beta_c;
        const double kappa0 = slot_scalar(pb, th, SS_SCHEDULE0 + pb.nb + pb.seg_ik[seg]);
        double ci[RT_MAX_AGE], gj[RT_MAX_AGE], v[RT_MAX_AGE], w[RT_MAX_AGE];
        for (int i = 0; i < n; ++i) {
            ci[i] = beta0 * kappa0 * slot_vec(pb, th, VF_A, i) * pb.N[i];
            const double pj = slot_vec(pb, th, VF_P, i), hj = slot_vec(pb, th, VF_H, i);
            const double dwell = 1.0 / gamma_p + pj / gamma_A + theta_i * (1.0 - pj) / (gamma_I + hj);
            gj[i] = (pb.N[i] < 1e-9) ? 0.0 : slot_vec(pb, th, VF_H_INFEC, i) / pb.N[i] * dwell;
            v[i] = 1.0;
        }
        for (int it = 0; it < 2000; ++it) {
            double m = 0.0;
            for (int i = 0; i < n; ++i) {
                double acc = 0.0;
                for (int j = 0; j < n; ++j) acc += ci[i] * pb.Mrow[i * pb.lpc + j] * gj[j] * v[j];
                w[i] = acc;
                m = (fabs(acc) > m) ? fabs(acc) : m;
            }
            if (!(m > 0.0)) { r0 = 0.0; break; }
            for (int i = 0; i < n; ++i) v[i] = w[i] / m;
            const bool done = fabs(m - r0) <= 1e-15 * m;
            r0 = m;
            if (done) break;
        }
    }

    double cum_inf[RT_MAX_AGE];
    for (int i = 0; i < n; ++i) {
        double c = 0.0;
        for (int comp = 1; comp <= 7; ++comp) c += pb.init_state[comp * pb.lpc + i];  // E0 + P0 + ... + R0
        cum_inf[i] = c;
    }
    int target = 0;
    {
        double best = INFINITY;
        for (int k = 0; k < a.T; ++k) {
            const double d = fabs(pb.times[k] - 64.0);
            if (d < best) { best = d; target = k; }
        }
    }
    double peak_h = 0.0, peak_icu = 0.0, t_peak_h = 0.0, t_peak_icu = 0.0;
    double max_rt = 0.0, min_rt = 1e6, final_rt = 0.0, sero64 = 0.0;
    for (int k = 0; k < a.T; ++k) {
        const double* row = traj + (size_t)k * (NUM_COMP * n);
        const double t = pb.times[k];
        const double dt = (k > 0) ? (t - pb.times[k - 1]) : 1.0;
        const double r = rt[(size_t)k * a.S_pad];
        max_rt = (max_rt < r) ? r : max_rt;
        min_rt = (r < min_rt) ? r : min_rt;
        if (k == a.T - 1) final_rt = r;
        double tot_h = 0.0, tot_icu = 0.0, tot_s = 0.0;
        for (int i = 0; i < n; ++i) { tot_h += row[5 * n + i]; tot_icu += row[6 * n + i]; tot_s += row[i]; }
        if (tot_h > peak_h) { peak_h = tot_h; t_peak_h = t; }
        if (tot_icu > peak_icu) { peak_icu = tot_icu; t_peak_icu = t; }
        int seg = 0;
        for (int j = 0; j < pb.nm; ++j) seg += (pb.mends[j] < t) ? 1 : 0;
        const double kappa = slot_scalar(pb, th, SS_SCHEDULE0 + pb.nb + pb.seg_ik[seg]);
        for (int i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int j = 0; j < n; ++j) {
                const double load = (pb.N[j] > 1e-9) ? (row[2 * n + j] + row[3 * n + j] + theta_i * row[4 * n + j]) / pb.N[j] : 0.0;
                acc += pb.Mrow[i * pb.lpc + j] * load;
            }
            cum_inf[i] += (beta_c * kappa) * acc * row[i] * dt;
        }
        if (k == target) sero64 = (total_pop - tot_s) / total_pop;
    }
    const double* last = traj + (size_t)(a.T - 1) * (NUM_COMP * n);
    double sum_inf = 0.0, sum_deaths = 0.0;
    for (int i = 0; i < n; ++i) {
        const double deaths = last[8 * n + i] - pb.init_state[8 * pb.lpc + i];
        const double hosp = last[9 * n + i] - pb.init_state[9 * pb.lpc + i];
        const double icu = last[10 * n + i] - pb.init_state[10 * pb.lpc + i];
        sum_inf += cum_inf[i];
        sum_deaths += deaths;
        double ifr = 0.0, ihr = 0.0, iicur = 0.0;
        if (cum_inf[i] > 1.0) {
            ifr = fmax(0.0, fmin(deaths / cum_inf[i], 1.0));
            ihr = fmax(0.0, fmin(hosp / cum_inf[i], 1.0));
            iicur = fmax(0.0, fmin(icu / cum_inf[i], 1.0));
        }
        out[METRIC_SCALARS + 4 * i + 0] = ifr;
        out[METRIC_SCALARS + 4 * i + 1] = ihr;
        out[METRIC_SCALARS + 4 * i + 2] = iicur;
        out[METRIC_SCALARS + 4 * i + 3] = (pb.N[i] > 0) ? cum_inf[i] / pb.N[i] : 0.0;
    }
    out[0] = r0;
    out[1] = (sum_inf > 1e-9) ? sum_deaths / sum_inf : 0.0;
    out[2] = sum_inf / total_pop;
    out[3] = peak_h; out[4] = peak_icu; out[5] = t_peak_h; out[6] = t_peak_icu;
    out[7] = sum_deaths;
    out[8] = max_rt; out[9] = min_rt; out[10] = final_rt; out[11] = sero64;
}

// ---- the picks of the summaries here (the kernels and launchers that take them: csrc/sepaihrd_segment_sort.inc) ----

// quantile p of sorted segment `sid` (*n_valid valid values first, +inf after them) into its output slot
struct EnsemblePick {
    static constexpr int SORTED_BLOCK = 256;
    EnsembleArgs a;
    int n_series_segments;
    __host__ __device__ int picks() const { return a.n_probs; }
    __device__ void operator()(size_t sid, int p, const double* seg) const {
        const int nv = *a.n_valid;
        const double r = nv > 0 ? sepaihrd_quantile::sorted_quantile(seg, (size_t)nv, a.probs[p]) : NAN;
        if ((int)sid < n_series_segments) {
            const int age = (int)(sid % a.n);
            const int t = (int)((sid / a.n) % a.Tp);
            const int ser = (int)(sid / ((size_t)a.n * a.Tp));
            a.q_out[(((size_t)ser * a.n_probs + p) * a.Tp + t) * a.n + age] = r;
        } else if (a.rt_out != nullptr && (int)sid >= a.rt_segment0) {
            a.rt_out[(size_t)p * a.T + (sid - (size_t)a.rt_segment0)] = r;
        } else {
            const size_t k = sid - (size_t)n_series_segments;
            a.sero_out[(size_t)p * a.T + k] = r;
        }
    }
};

// ---- scenario analysis (sepaihrd_scenario_ensemble): metric table [K][S][W] -> per-scenario summaries ----
// Segment (k, col) of the metric values and of the paired differences metric[k][s] - metric[0][s]; samples that failed
// (in scenario k, or for a difference in k or in the baseline) are +inf and sort to the end.
__global__ __launch_bounds__(256) void scenario_gather_kernel(const ScenarioArgs a) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = (int)(idx % a.S_pad);
    const size_t seg = idx / a.S_pad;  // k W + col
    if (seg >= (size_t)a.K * a.W) return;
    const int k = (int)(seg / a.W), col = (int)(seg % a.W);
    double v = INFINITY, d = INFINITY;
    if (s < a.S) {
        const bool ok = a.wstatus[(size_t)k * a.status_stride + s] == 0, ok0 = a.wstatus[s] == 0;
        const double x = a.metrics[((size_t)k * a.S + s) * a.W + col];
        if (ok) v = x;
        if (ok && ok0) d = x - a.metrics[(size_t)s * a.W + col];
    }
    a.vals[seg * a.S_pad + s] = v;
    a.vals[((size_t)a.K * a.W + seg) * a.S_pad + s] = d;
}

// valid samples per scenario ([0, K)) and valid in both the scenario and the baseline ([K, 2K)): one block each
__global__ __launch_bounds__(256) void scenario_count_kernel(const ScenarioArgs a) {
    __shared__ int part[256];
    const int k = blockIdx.x % a.K;
    const bool paired = (int)blockIdx.x >= a.K;
    int c = 0;
    for (int s = threadIdx.x; s < a.S; s += 256)
        c += a.wstatus[(size_t)k * a.status_stride + s] == 0 && (!paired || a.wstatus[s] == 0);
    part[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.counts[blockIdx.x] = part[0];
}

// mean and population standard deviation of every (k, col) over the valid samples in sample order: the operation
// sequence of HipPosteriorEnsemble::aggregateMetrics (ResultAggregator::aggregateBatchMetrics, lazy variance).  Reads the
// gathered segment (sample order, contiguous) before it is sorted; the loads of 8 samples are issued ahead of their sums.
constexpr int MOMENT_BATCH = 8;
__global__ __launch_bounds__(64) void scenario_moments_kernel(const ScenarioArgs a) {
    const int seg = blockIdx.x * blockDim.x + threadIdx.x;
    if (seg >= a.K * a.W) return;
    const int k = seg / a.W;
    const int32_t* st = a.wstatus + (size_t)k * a.status_stride;
    const double* v = a.vals + (size_t)seg * a.S_pad;  // +inf where the sample failed
    double* out = a.summary_out + (size_t)seg * (2 + a.n_probs);
    const int nv = a.counts[k];
    if (nv == 0) { out[0] = NAN; out[1] = NAN; return; }
    double mean = 0.0;
    for (int s0 = 0; s0 < a.S; s0 += MOMENT_BATCH) {
        double x[MOMENT_BATCH];
        bool ok[MOMENT_BATCH];
#pragma unroll
        for (int d = 0; d < MOMENT_BATCH; ++d) {
            ok[d] = s0 + d < a.S && st[s0 + d] == 0;
            x[d] = ok[d] ? v[s0 + d] : 0.0;
        }
#pragma unroll
        for (int d = 0; d < MOMENT_BATCH; ++d)
            if (ok[d]) mean += x[d];
    }
    mean /= (double)(size_t)nv;
    double var = 0.0;
    for (int s0 = 0; s0 < a.S; s0 += MOMENT_BATCH) {
        double x[MOMENT_BATCH];
        bool ok[MOMENT_BATCH];
#pragma unroll
        for (int d = 0; d < MOMENT_BATCH; ++d) {
            ok[d] = s0 + d < a.S && st[s0 + d] == 0;
            x[d] = ok[d] ? v[s0 + d] : 0.0;
        }
#pragma unroll
        for (int d = 0; d < MOMENT_BATCH; ++d)
            if (ok[d]) var += (x[d] - mean) * (x[d] - mean);
    }
    var /= (double)(size_t)nv;
    out[0] = mean;
    out[1] = sqrt(var);
}

// quantile p of sorted segment `sid` (metric segments first, then the paired differences) into its output slot
struct ScenarioPick {
    static constexpr int SORTED_BLOCK = 256;
    ScenarioArgs a;
    __host__ __device__ int picks() const { return a.n_probs; }
    __device__ void operator()(size_t sid, int p, const double* seg) const {
        const bool paired = sid >= (size_t)a.K * a.W;
        const size_t cell = paired ? sid - (size_t)a.K * a.W : sid;
        const int nv = a.counts[(paired ? a.K : 0) + (int)(cell / a.W)];
        const double r = nv > 0 ? sepaihrd_quantile::sorted_quantile(seg, (size_t)nv, a.probs[p]) : NAN;
        if (paired) {
            if (a.diff_out != nullptr) a.diff_out[cell * a.n_probs + p] = r;
        } else if (a.summary_out != nullptr) {
            a.summary_out[cell * (2 + a.n_probs) + 2 + p] = r;
        }
    }
};

// ---- age-structured SIR: posterior ensemble and intervention scenarios (sepaihrd_sir_scenario_ensemble) ----
// The ensemble build of the SIR integrator (csrc/sepaihrd_sir.hip) has stored the series of every valid chain in
// vals[((k 3 + series) T + t) (n + 1) + column][S_pad].  Fix-up: the rows of samples that failed (at any point of the run)
// and of the padding s >= S become +inf, so they sort last.  One thread per (scenario, sample) and block of rows; threads
// of valid samples leave at once.  The scenario is folded into the grid's x dimension (K is bounded by the chain count, not
// by 65 535) and the row blocks go round the y dimension.
constexpr int SIR_FIX_ROWS = 64;
__global__ __launch_bounds__(256) void sir_ens_fixup_kernel(const SirEnsSummaryArgs a) {
    const int xblocks = (a.S_pad + 255) / 256;
    const int k = blockIdx.x / xblocks;
    const int s = (blockIdx.x % xblocks) * 256 + threadIdx.x;
    if (s >= a.S_pad) return;
    if (s < a.S && a.status[(size_t)k * a.S + s] == 0) return;
    const int rows = SIR_ENS_SERIES * a.T * (a.n + 1);
    double* col = a.vals + (size_t)k * rows * a.S_pad + s;
    for (int r0 = blockIdx.y * SIR_FIX_ROWS; r0 < rows; r0 += gridDim.y * SIR_FIX_ROWS) {
        const int r1 = (r0 + SIR_FIX_ROWS < rows) ? r0 + SIR_FIX_ROWS : rows;
        for (int r = r0; r < r1; ++r) col[(size_t)r * a.S_pad] = INFINITY;
    }
}

// R0 of every sample: spectral radius of K_ij = q scale C_ij N_i / (N_j gamma_j) with the sample's parameters before any event
// (columns with N_j <= 1e-9 dropped, gamma_j = 0: +inf), by Perron iteration in the max-norm with the stopping rule of
// ensemble_rt_kernel.  Mapped as the integrator maps a chain: one lane per (sample, age), lpc lanes per sample, 64 / lpc
// samples per one-wavefront block; the baseline matrix sits in LDS, the iterate goes round through LDS.  A sample's iteration
// is frozen at the first iteration that meets the rule; the block runs until all of its samples have.
constexpr int SIR_MAX_AGE = 64;
__global__ __launch_bounds__(WAVE) void sir_ens_r0_kernel(const SirEnsSummaryArgs a, const SirDevProblem pb, double* r0_out) {
    extern __shared__ double r0_lds[];  // [lpc][lpc] C, [WAVE] g_j v_j
    const int lpc = pb.lpc, n = pb.n, lane = threadIdx.x;
    double* sC = r0_lds;
    double* su = r0_lds + lpc * lpc;
    for (int i = lane; i < lpc * lpc; i += WAVE) sC[i] = pb.C[i];
    const int cpw = WAVE / lpc;
    const int age = lane % lpc, grp = lane / lpc;
    const int s_raw = blockIdx.x * cpw + grp;
    const bool valid = s_raw < a.S;
    const int s = valid ? s_raw : 0;
    // SIRParameterManager::applyConstraints + updateModelParameters, as the integrator's prologue
    double q = pb.q, scale = pb.scale, gamma = pb.gamma[age];
    const double* th = a.theta + (size_t)s * pb.P;
    for (int p = 0; p < pb.P; ++p) {
        const int f = pb.param_field[p];
        const double x = th[p];
        if (f == 0) q = (1e-12 < x) ? x : 1e-12;
        else if (f == 1) scale = (0.0 < x) ? x : 0.0;
        else if (pb.param_index[p] == age) gamma = (0.0 < x) ? x : 0.0;
    }
    const double Ni = pb.N[age];
    const bool has_pop = age < n && Ni > 1e-9;
    const double ci = q * scale * Ni;
    const double gj = has_pop ? 1.0 / (Ni * gamma) : 0.0;
    su[lane] = (has_pop && gamma == 0.0) ? 1.0 : 0.0;
    __syncthreads();
    bool unbounded = false;
    for (int j = 0; j < lpc; ++j) unbounded |= su[grp * lpc + j] != 0.0;
    double v = 1.0, r0 = 0.0;
    bool done = unbounded;
    for (int it = 0; it < 2000; ++it) {
        if (__ballot(!done) == 0ull) break;
        __syncthreads();  // the readers of the previous iterate are done
        su[lane] = gj * v;
        __syncthreads();
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc += ci * sC[age * lpc + j] * su[grp * lpc + j];
        if (age >= n) acc = 0.0;
        __syncthreads();
        su[lane] = acc;
        __syncthreads();
        double m = 0.0;
        for (int j = 0; j < n; ++j) {
            const double w = su[grp * lpc + j];
            m = (w > m) ? w : m;
        }
        if (!done) {
            if (!(m > 0.0)) {
                r0 = 0.0;
                done = true;
            } else {
                v = acc / m;
                done = fabs(m - r0) <= 1e-15 * m;
                r0 = m;
            }
        }
    }
    if (valid && age == 0) r0_out[s] = unbounded ? (double)INFINITY : r0;
}

// Per-sample metrics of scenario k from the stored series and R0, one thread per (scenario, sample).  Row layout:
//   [0] R0  [1] peak total prevalence  [2] its output time  [3] peak total incidence  [4] its output time
//   [5] overall attack rate sum_i (S_i(t0) - S_i(t_last)) / sum N, then per age: attack rate, peak prevalence
// R0 is the sample's (sir_ens_r0_kernel), whatever the scenario.  Peaks: the first maximal row counts.  The per-age peaks are
// one more walk over the output times per age (the same loads, coalesced over the samples), so nothing is indexed at run time
// and nothing lives in scratch.  The scenario is folded into the grid's x dimension, as in the fix-up.
__global__ __launch_bounds__(WAVE) void sir_ens_metrics_kernel(const SirEnsSummaryArgs a, const SirDevProblem pb, const double* r0_in) {
    const int sblocks = (a.S + WAVE - 1) / WAVE;
    const int k = blockIdx.x / sblocks;
    const int s = (blockIdx.x % sblocks) * WAVE + threadIdx.x;
    if (s >= a.S) return;
    const int n = a.n, T = a.T, width = SIR_ENS_SCALARS + 2 * n;
    double* out = a.metrics + ((size_t)k * a.S + s) * width;
    if (a.status[(size_t)k * a.S + s] != 0) {
        for (int i = 0; i < width; ++i) out[i] = NAN;
        return;
    }
    double total_pop = 0.0;
    for (int i = 0; i < n; ++i) total_pop += pb.N[i];
    const size_t row = (size_t)(n + 1) * a.S_pad;  // doubles between output times
    const double* inc = a.vals + ((size_t)(k * SIR_ENS_SERIES + 0) * T) * row + s;
    const double* prev = a.vals + ((size_t)(k * SIR_ENS_SERIES + 1) * T) * row + s;
    const double* cumi = a.vals + ((size_t)(k * SIR_ENS_SERIES + 2) * T) * row + s;
    double peak_prev = prev[(size_t)n * a.S_pad], peak_inc = inc[(size_t)n * a.S_pad];
    int k_prev = 0, k_inc = 0;
    for (int t = 1; t < T; ++t) {
        const double tp = prev[(size_t)t * row + (size_t)n * a.S_pad], ti = inc[(size_t)t * row + (size_t)n * a.S_pad];
        if (tp > peak_prev) { peak_prev = tp; k_prev = t; }
        if (ti > peak_inc) { peak_inc = ti; k_inc = t; }
    }
    const double* last = cumi + (size_t)(T - 1) * row;
    out[0] = r0_in[s];
    out[1] = peak_prev; out[2] = pb.times[k_prev];
    out[3] = peak_inc; out[4] = pb.times[k_inc];
    out[5] = last[(size_t)n * a.S_pad] / total_pop;
    for (int i = 0; i < n; ++i) {
        const double* pa = prev + (size_t)i * a.S_pad;
        double w = pa[0];  // peak prevalence of age i
        for (int t = 1; t < T; ++t) {
            const double x = pa[(size_t)t * row];
            w = (x > w) ? x : w;
        }
        out[SIR_ENS_SCALARS + 2 * i] = (pb.N[i] > 0) ? last[(size_t)i * a.S_pad] / pb.N[i] : 0.0;
        out[SIR_ENS_SCALARS + 2 * i + 1] = w;
    }
}

}  // namespace

int launch_scenario_summaries(const ScenarioArgs& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.K <= 0 || a.S <= 0 || a.W <= 0 || !pad_legal((size_t)a.S, a.S_pad)) return -4;
    const int segments = 2 * a.K * a.W;
    hipLaunchKernelGGL(scenario_count_kernel, dim3(2 * a.K), dim3(256), 0, st, a);
    const size_t cells = (size_t)a.K * a.W * a.S_pad;
    hipLaunchKernelGGL(scenario_gather_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a);
    if (a.summary_out != nullptr)
        hipLaunchKernelGGL(scenario_moments_kernel, dim3((unsigned)((a.K * a.W + 63) / 64)), dim3(64), 0, st, a);
    return launch_sort_pick(ScenarioPick{a}, a.vals, a.S_pad, segments, a.sort_scratch, a.sort_scratch_doubles, st);
}

int launch_ensemble_summaries(const EnsembleArgs& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.S <= 0 || !pad_legal((size_t)a.S, a.S_pad)) return -4;
    hipLaunchKernelGGL(ensemble_count_valid_kernel, dim3(1), dim3(256), 0, st, a.wstatus, a.S, a.n_valid);
    const size_t cols = (size_t)a.S_pad * a.lpc;
    hipLaunchKernelGGL(ensemble_series_kernel, dim3((unsigned)((cols + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a);
    const int n_series_segments = 6 * a.Tp * a.n;
    const bool sero = a.traj != nullptr && a.sero_out != nullptr;
    const bool rt = a.traj != nullptr && a.rt_out != nullptr;
    if (rt && (a.n > RT_MAX_AGE || a.rt_segment0 != n_series_segments + (sero ? a.T : 0))) return -4;
    if (rt) {
        const size_t cells = (size_t)a.S_pad * a.T;
        hipLaunchKernelGGL(ensemble_rt_kernel, dim3((unsigned)((cells + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a, *a.pb, a.theta);
    }
    if (a.metrics_out != nullptr) {
        if (!rt) return -4;  // the table needs the Rt values
        hipLaunchKernelGGL(ensemble_metrics_kernel, dim3((unsigned)((a.S + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a, *a.pb, a.theta);
    }
    const int segments = n_series_segments + (sero ? a.T : 0) + (rt ? a.T : 0);
    return launch_sort_pick(EnsemblePick{a, n_series_segments}, a.vals, a.S_pad, segments, a.sort_scratch, a.sort_scratch_doubles, st);
}

}  // namespace sepaihrd

namespace sepaihrd {

int launch_sir_ensemble_summaries(const SirEnsSummaryArgs& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.K <= 0 || a.S <= 0 || a.n < 1 || a.n > SIR_MAX_AGE || a.T < 1 || !pad_legal((size_t)a.S, a.S_pad)) return -4;
    const int rows = SIR_ENS_SERIES * a.T * (a.n + 1);  // sortable segments per scenario
    // K x S fits a 32-bit chain count (checked by the caller), so K x (blocks of samples) fits the grid's x dimension
    const int row_blocks = (rows + SIR_FIX_ROWS - 1) / SIR_FIX_ROWS;
    hipLaunchKernelGGL(sir_ens_fixup_kernel, dim3((unsigned)((a.S_pad + 255) / 256) * (unsigned)a.K, (unsigned)(row_blocks < 65535 ? row_blocks : 65535)),
                       dim3(256), 0, st, a);
    if (a.metrics != nullptr) {
        const int cpw = WAVE / a.lpc;
        hipLaunchKernelGGL(sir_ens_r0_kernel, dim3((unsigned)((a.S + cpw - 1) / cpw)), dim3(WAVE), (size_t)(a.lpc * a.lpc + WAVE) * sizeof(double), st,
                           a, *a.pb, a.r0);
        hipLaunchKernelGGL(sir_ens_metrics_kernel, dim3((unsigned)((a.S + WAVE - 1) / WAVE) * (unsigned)a.K), dim3(WAVE), 0, st, a, *a.pb, a.r0);
    }
    if (a.ev_after_metrics != nullptr && hipEventRecord(static_cast<hipEvent_t>(a.ev_after_metrics), st) != hipSuccess) return -3;
    // the series' quantiles: the segment sort and the interpolation of sepaihrd_ensemble_quantiles, per scenario (each has
    // its own count of valid samples), with (T, n + 1) in the place of (Tp, n) and no seroprevalence / Rt block; the LDS
    // limit is raised once for all scenarios
    if (raise_lds_limit(plan_of_pad((size_t)a.S_pad), reinterpret_cast<const void*>(&segment_sort_pick_kernel<EnsemblePick>)) != 0) return -3;
    for (int k = 0; k < a.K; ++k) {
        EnsembleArgs e{};
        e.S = a.S; e.S_pad = a.S_pad; e.lpc = a.lpc; e.n = a.n + 1; e.T = a.T; e.Tp = a.T;
        e.n_probs = a.n_probs; e.probs = a.probs;
        e.vals = a.vals + (size_t)k * rows * a.S_pad;
        e.q_out = a.q_out + (size_t)k * SIR_ENS_SERIES * a.n_probs * a.T * (a.n + 1);
        e.n_valid = a.n_valid + k;
        e.rt_segment0 = rows;
        hipLaunchKernelGGL(ensemble_count_valid_kernel, dim3(1), dim3(256), 0, st, a.status + (size_t)k * a.S, a.S, e.n_valid);
        if (a.q_out == nullptr) continue;
        const int rc = launch_sort_pick(EnsemblePick{e, rows}, e.vals, e.S_pad, rows, a.sort_scratch, a.sort_scratch_doubles, st,
                                        /*lds_limit_raised=*/true);
        if (rc != 0) return rc;  // a failed sort of scenario k ends the call at once
    }
    if (hipGetLastError() != hipSuccess) return -3;
    if (a.metrics == nullptr || (a.summary_out == nullptr && a.diff_out == nullptr)) return 0;
    ScenarioArgs sa{};
    sa.K = a.K; sa.S = a.S; sa.S_pad = a.S_pad; sa.W = SIR_ENS_SCALARS + 2 * a.n; sa.n_probs = a.n_probs; sa.probs = a.probs;
    sa.metrics = a.metrics; sa.wstatus = a.status; sa.status_stride = (size_t)a.S;
    sa.vals = a.svals; sa.counts = a.counts;
    sa.summary_out = a.summary_out; sa.diff_out = a.diff_out;
    sa.sort_scratch = a.sort_scratch; sa.sort_scratch_doubles = a.sort_scratch_doubles;
    return launch_scenario_summaries(sa, stream);
}

}  // namespace sepaihrd

// ---- stochastic SIR ensembles (sepaihrd_stoch_sir_run): mean, median, 5 % and 95 % of every (group, compartment, step)
// segment across the replicates, with the segment sorts above ----
namespace sepaihrd {
namespace {

// statistic `stat` of sorted segment `sid` of the chunk into stats[g][stat][compartment][step0 + local step]: one thread per
// statistic (the mean's recurrence is serial)
struct StochSirPick {
    static constexpr int SORTED_BLOCK = 64;
    StochSummaryArgs a;
    __host__ __device__ int picks() const { return 4; }
    __device__ void operator()(size_t sid, int stat, const double* seg) const {
        const int s = (int)(sid % (size_t)a.chunk_steps);
        const size_t gc = sid / (size_t)a.chunk_steps;  // group 3 + compartment
        const size_t g = gc / 3, comp = gc % 3;
        a.stats[((g * 4 + (size_t)stat) * 3 + comp) * (size_t)a.steps + (size_t)(a.step0 + s)] = sepaihrd_stoch::sorted_stat(seg, a.R, stat);
    }
};

}  // namespace

int launch_stoch_sir_summaries(const StochSummaryArgs& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t segments = (size_t)a.G * 3 * (size_t)a.chunk_steps;
    if (a.G <= 0 || a.R <= 0 || a.chunk_steps <= 0 || a.step0 < 0 || a.step0 + a.chunk_steps > a.steps || segments >= ((size_t)1 << 31) ||
        !pad_legal((size_t)a.R, a.R_pad))
        return -4;
    // summary_ms takes the sorted pick of every group (the LDS route is one launch and is not timed here)
    const PickTimer timer{static_cast<hipEvent_t>(a.ev[0]), static_cast<hipEvent_t>(a.ev[1]), a.summary_ms};
    const bool timed = a.summary_ms != nullptr && a.ev[0] != nullptr && a.ev[1] != nullptr;
    return launch_sort_pick(StochSirPick{a}, a.vals, a.R_pad, (int)segments, a.sort_scratch, a.sort_scratch_doubles, st,
                            /*lds_limit_raised=*/false, timed ? &timer : nullptr);
}

}  // namespace sepaihrd

// ---- posterior predictive draws (sepaihrd_ensemble_predictive): the quantiles of the 6 Tp n segments of S R replicated
// counts, with the segment sorts and the interpolation of sepaihrd_ensemble_quantiles; the count of values per segment is
// the number of valid samples times R.  With scores (sepaihrd_ensemble_predictive_scores) every cell of
// the three daily series is, from the same sorted segment, scored by the rules of csrc/sepaihrd_predictive_score.inc ----
namespace sepaihrd {
namespace {

bool predictive_segments_ok(const PredictiveArgs& a) {
    return a.S > 0 && a.R > 0 && (size_t)6 * a.Tp * a.n < ((size_t)1 << 31) && pad_legal((size_t)a.S * a.R, a.N_pad);
}

EnsemblePick predictive_pick(const PredictiveArgs& a) {
    const int segments = 6 * a.Tp * a.n;
    EnsembleArgs e{};
    e.S = a.S * a.R; e.S_pad = a.N_pad; e.lpc = a.lpc; e.n = a.n; e.T = a.T; e.Tp = a.Tp;
    e.n_probs = a.n_probs; e.probs = a.probs;
    e.vals = a.vals; e.q_out = a.q_out;
    e.n_valid = a.counts + 1;
    e.rt_segment0 = segments;
    return EnsemblePick{e, segments};
}

// the observations of every daily cell as predictive_pit_kernel reads them from the context's grid
__global__ __launch_bounds__(256) void score_observed_kernel(const PredictiveArgs a, double* obs) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;  // (series Tp + t) n + age
    if (cell >= (size_t)3 * a.Tp * a.n) return;
    const int age = (int)(cell % a.n);
    const int t = (int)((cell / a.n) % a.Tp);
    const int ser = (int)(cell / ((size_t)a.n * a.Tp));
    obs[cell] = a.grid[((size_t)(a.runup_offset + t) * a.lpc + age) * 4 + ser];
}

// One lane per (series, age or pooled, field): the walk of csrc/sepaihrd_predictive_score.inc over the cell scores in its stated
// order, the sum in a register.  A lane per field instead of one per entry: an entry's 4 + 2 L sums are independent chains of
// additions, and a lane that carried them all would serve each in turn.
__global__ __launch_bounds__(WAVE) void score_summary_kernel(const ScoreArgs sc, const int Tp, const int n, double* summary) {
    const int SW = sepaihrd_score::summary_width(sc.L);
    const int idx = (int)(blockIdx.x * (unsigned)WAVE + threadIdx.x);
    if (idx >= 3 * (n + 1) * SW) return;
    const int e = idx / SW, f = idx % SW;
    summary[idx] = sepaihrd_score::summary_field(sc.scores, sc.obs, (size_t)sc.counts[1], Tp, n, sc.L, e / (n + 1), e % (n + 1), f);
}

}  // namespace

int launch_predictive_quantiles(const PredictiveArgs& a, void* stream) {
    if (!predictive_segments_ok(a)) return -4;
    return launch_sort_pick(predictive_pick(a), a.vals, a.N_pad, 6 * a.Tp * a.n, a.sort_scratch, a.sort_scratch_doubles,
                            static_cast<hipStream_t>(stream));
}

int launch_predictive_scores(const PredictiveArgs& a, const PredictiveScoreArgs& sa, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!predictive_segments_ok(a) || sa.n_levels < 0 || sa.n_levels > sepaihrd_score::MAX_LEVELS || !sa.obs || !sa.cell_scores || !sa.summary ||
        !sa.exact || (sa.n_levels > 0 && !sa.levels))
        return -4;
    const int cells = 3 * a.Tp * a.n;  // the daily segments come first in the segment table
    const ScoreArgs sc{cells, sa.n_levels, a.counts, sa.obs, sa.levels, sa.cell_scores, sa.pit_out, sa.exact};
    if (sa.obs_from_grid) hipLaunchKernelGGL(score_observed_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a, sa.obs);
    const int rc = launch_sort_pick_score(predictive_pick(a), sc, a.vals, a.N_pad, 2 * cells, a.sort_scratch, a.sort_scratch_doubles, st);
    if (rc != 0) return rc;
    const int fields = 3 * (a.n + 1) * sepaihrd_score::summary_width(sa.n_levels);
    hipLaunchKernelGGL(score_summary_kernel, dim3((unsigned)((fields + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, sc, a.Tp, a.n, sa.summary);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd

