// csrc/sepaihrd_predictive_targets.hip -- scores of the posterior predictive draws on weekly and age-group totals on gfx950
// (sepaihrd_ensemble_predictive_targets).  The rule is csrc/sepaihrd_predictive_targets.inc, the text the
// host twin compiles too.  The draw kernel is predictive_nb_draw_kernel's mapping -- one lane per (draw, age, series), the same
// variates at the same stream coordinates -- with the window total and its running sum held in two registers and added into the
// target table; the sort, the picks and the scores are the texts of csrc/sepaihrd_bitonic.inc, csrc/sepaihrd_quantile.inc and
// csrc/sepaihrd_predictive_score.inc over the 6 W G target segments.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sepaihrd_bitonic.inc"
#include "sepaihrd_device.h"
#include "sepaihrd_nb_draw.inc"
#include "sepaihrd_predictive_targets.inc"
#include "sepaihrd_predictive_targets_device.h"
#include "sepaihrd_segments.h"

namespace sepaihrd {
namespace {

constexpr int DRAW_BLOCK = 256;

// One lane per (sample s, replicate r, launched age, series): predictive_nb_draw_kernel's lanes and its draw, bit for bit.  The
// lane sums the rows of a window in `win` and the windows in `run`; at a window's last row it adds both into the slots of its
// group's two targets.  The lanes of a group's ages sit in different workgroups and meet there: the sums are of integers, exact
// below 2^53, so the order the adds arrive in does not show.  The table was zeroed before the launch.  Consecutive lanes add to
// consecutive doubles, nothing is returned.  A failed or padding slot receives +inf from every lane that owns it.  The daily draw
// goes to memory only where a.draws is wanted; rows of no window are drawn only then, and a lane of an age outside every group
// (launched only where means or draws are wanted) adds nothing.
__global__ __launch_bounds__(DRAW_BLOCK) void predictive_target_draw_kernel(const PredictiveArgs a, const PredictiveTargetArgs tg,
                                                                            const double* __restrict__ k_used) {
    const size_t idx = (size_t)blockIdx.x * DRAW_BLOCK + threadIdx.x;
    if (idx >= (size_t)a.N_pad) return;
    const int age = tg.launch_age[blockIdx.y], ser = (int)blockIdx.z;
    const int g = tg.age_group[age];
    const size_t s = idx / (size_t)a.R;
    const uint32_t r = (uint32_t)(idx % (size_t)a.R);
    const bool in_range = s < (size_t)a.S;
    const bool ok = in_range && a.wstatus[s] == 0;
    const size_t seg_stride = (size_t)a.N_pad;
    const int comp = (ser == 0) ? 1 : (ser == 1) ? 2 : 0;  // cum rows are D, CumH, CumICU; series are H, ICU, D
    const double k = ok ? k_used[s * 3 + (size_t)ser] : INFINITY;
    const size_t col = s * (size_t)a.lpc + (size_t)age;
    const bool daily = a.draws != nullptr && in_range;
    double win = ok ? 0.0 : INFINITY, run = win;
    int v = 0, rows = 0;  // the window the next target row belongs to, and its rows already summed
    for (int t = 0; t < a.Tp; ++t) {
        const bool in_target = g >= 0 && t >= tg.origin && v < tg.W;
        const size_t cell = ((size_t)ser * a.Tp + t) * a.n + age;
        double m = NAN, y = NAN;
        if (ok) {
            const double inc = a.cum[cum_index(a.T, col, a.runup_offset + t, comp)];
            m = (0.0 < inc) ? inc : 0.0;
            if (in_target || daily) y = sepaihrd_nb_draw::nb_variate(a.seed, (uint32_t)s, r, (uint32_t)cell, m + 1e-10, k);
        }
        if (in_range) {
            if (a.means != nullptr && r == 0) a.means[((s * 3 + ser) * a.Tp + t) * a.n + age] = m;
            if (daily) a.draws[((idx * 3 + ser) * a.Tp + t) * a.n + age] = y;
        }
        if (in_target) {
            if (ok) win += y;
            if (++rows == tg.window) {
                run += win;
                unsafeAtomicAdd(tg.tvals + sepaihrd_targets::target_index(ser, v, g, tg.W, tg.G) * seg_stride + idx, win);
                unsafeAtomicAdd(tg.tvals + sepaihrd_targets::target_index(ser + 3, v, g, tg.W, tg.G) * seg_stride + idx, run);
                win = ok ? 0.0 : INFINITY;
                rows = 0;
                ++v;
            }
        }
    }
}

// target_draws [S][R][3][W][G] from the table before it is sorted: the window totals of the three daily series, NaN for a failed
// sample.  One lane per output value.
__global__ __launch_bounds__(DRAW_BLOCK) void predictive_target_gather_kernel(const PredictiveArgs a, const PredictiveTargetArgs tg) {
    const size_t o = (size_t)blockIdx.x * DRAW_BLOCK + threadIdx.x;
    const size_t per_draw = (size_t)3 * tg.W * tg.G;
    if (o >= (size_t)a.S * a.R * per_draw) return;
    const size_t idx = o / per_draw, seg = o % per_draw;
    tg.target_draws[o] = a.wstatus[idx / (size_t)a.R] == 0 ? tg.tvals[seg * (size_t)a.N_pad + idx] : (double)NAN;
}

// the daily observation table the targets are formed from: the caller's, or the context's grid as predictive_pit_kernel reads it
struct DailyObs {
    const double* table;  // [3][Tp][n] or null
    const double* grid;
    int Tp, n, lpc, runup_offset;
    __host__ __device__ double operator()(int k, int t, int age) const {
        return table != nullptr ? table[((size_t)k * Tp + t) * n + age] : grid[((size_t)(runup_offset + t) * lpc + age) * 4 + k];
    }
};

// one lane per (daily series, group): the walk of csrc/sepaihrd_predictive_targets.inc over the windows in its stated order
__global__ __launch_bounds__(WAVE) void predictive_target_observed_kernel(const PredictiveArgs a, const PredictiveTargetArgs tg) {
    const int i = (int)(blockIdx.x * (unsigned)WAVE + threadIdx.x);
    if (i >= 3 * tg.G) return;
    const DailyObs obs{tg.obs_daily, a.grid, a.Tp, a.n, a.lpc, a.runup_offset};
    sepaihrd_targets::observed_targets(obs, tg.age_group, a.n, tg.window, tg.origin, tg.W, tg.G, i / tg.G, i % tg.G, tg.target_obs);
}

// ---- sort, pick and score: the siblings of segment_sort_score_kernel and segment_score_sorted_kernel of
// csrc/sepaihrd_ensemble.hip over the target table, where every one of the 6 W G segments is scored and the picks go to
// [6][n_probs][W][G] ----

struct TargetCells {
    int segments, WG, L, n_probs;
    const int32_t* counts;  // PredictiveArgs::counts: [1] = draws per segment
    const double* probs;    // [n_probs]
    const double* obs;      // [segments]
    const double* levels;   // [L]
    double* q_out;          // [6][n_probs][W][G]
    double* scores;         // [segments][5 + 4 L]
    double* pit_out;        // [segments] or null
    int32_t* exact;
};

constexpr int SCORE_MAX_WAVES = 16;  // of a 1024-lane workgroup
constexpr int SCORE_SUMS = 6;        // S1, S2, S_less, G, n_less, n_eq
constexpr size_t SCORE_RED_BYTES = SCORE_MAX_WAVES * SCORE_SUMS * sizeof(double);

// quantile p of sorted target segment `sid` by the rule of pred_quantiles
__device__ __forceinline__ void pick_target_quantile(const TargetCells& tc, const size_t sid, const int p, const double* seg) {
    const int m = tc.counts[1];
    const size_t k = sid / (size_t)tc.WG, vg = sid % (size_t)tc.WG;
    tc.q_out[(k * tc.n_probs + p) * (size_t)tc.WG + vg] = m > 0 ? sepaihrd_quantile::sorted_quantile(seg, (size_t)m, tc.probs[p]) : (double)NAN;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v, const int lane, const int active) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const T o = __shfl_down(v, off, WAVE);
        if (lane + off < active) v += o;
    }
    return v;
}

// The sums of sorted segment `seg` (LDS or device memory; m valid draws first) against the target's observation, reduced by the
// whole workgroup, then the cell rule by one lane: score_sorted_segment of csrc/sepaihrd_ensemble.hip for a target.  Every partial
// sum is a sum of integers and exact below 2^53, so the shape of the reduction does not show; where sums_exact fails the target
// says so in *exact.  red: SCORE_RED_BYTES of LDS.
__device__ __forceinline__ void score_sorted_target(const TargetCells& tc, const size_t sid, const double* seg, double* red) {
    const int tid = threadIdx.x, BS = blockDim.x;
    const int m = tc.counts[1];
    const double y = tc.obs[sid];
    sepaihrd_score::SegmentSums s = {0, 0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < m; i += BS) sepaihrd_score::add_draw(s, seg[i], i, m, y);
    const int lane = tid % WAVE, wave = tid / WAVE;
    const int active = (BS - wave * WAVE < WAVE) ? BS - wave * WAVE : WAVE;
    const double S1 = wave_sum(s.S1, lane, active), S2 = wave_sum(s.S2, lane, active), S_less = wave_sum(s.S_less, lane, active),
                 G = wave_sum(s.G, lane, active);
    const int n_less = wave_sum((int)s.n_less, lane, active), n_eq = wave_sum((int)s.n_eq, lane, active);
    if (lane == 0) {
        double* r = red + wave * SCORE_SUMS;
        r[0] = S1; r[1] = S2; r[2] = S_less; r[3] = G; r[4] = (double)n_less; r[5] = (double)n_eq;
    }
    __syncthreads();
    if (tid != 0) return;
    double t[SCORE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int waves = (BS + WAVE - 1) / WAVE;
    for (int w = 0; w < waves; ++w)
#pragma unroll
        for (int k = 0; k < SCORE_SUMS; ++k) t[k] += red[w * SCORE_SUMS + k];
    const sepaihrd_score::SegmentSums total = {(int64_t)t[4], (int64_t)t[5], t[0], t[1], t[2], t[3]};
    sepaihrd_score::cell_rule(seg, (size_t)m, y, total, tc.levels, tc.L, tc.scores + sid * (size_t)sepaihrd_score::cell_width(tc.L));
    if (tc.pit_out != nullptr) tc.pit_out[sid] = sepaihrd_score::pit_of(total, (size_t)m, y);
    if (m > 0 && !sepaihrd_score::sums_exact((size_t)m, seg[m - 1])) *tc.exact = 0;
}

// one workgroup per target segment of Np doubles: the sort in LDS, the picks, the scores.  Dynamic LDS: Np doubles, then
// SCORE_RED_BYTES.
__global__ void target_sort_score_kernel(const TargetCells tc, const double* vals, const int Np) {
    extern __shared__ double seg[];
    const size_t sid = blockIdx.x;
    lds_bitonic_sort(seg, vals + sid * (size_t)Np, Np);
    for (int p = threadIdx.x; p < tc.n_probs; p += blockDim.x) pick_target_quantile(tc, sid, p, seg);
    score_sorted_target(tc, sid, seg, seg + Np);
}

// beyond the LDS sort: one workgroup per segment of a group the radix sort has left in `sorted`
constexpr int SCORE_SORTED_BLOCK = 256;
__global__ __launch_bounds__(SCORE_SORTED_BLOCK) void target_score_sorted_kernel(const TargetCells tc, const double* sorted, const int Np,
                                                                                 const int first_segment) {
    __shared__ double red[SCORE_MAX_WAVES * SCORE_SUMS];
    const size_t sid = (size_t)first_segment + blockIdx.x;
    const double* seg = sorted + (size_t)blockIdx.x * Np;
    for (int p = threadIdx.x; p < tc.n_probs; p += SCORE_SORTED_BLOCK) pick_target_quantile(tc, sid, p, seg);
    score_sorted_target(tc, sid, seg, red);
}

// One lane per (series of 6, group or pooled, field), as score_summary_kernel: the walk of summary_field over the series' targets,
// windows ascending and, for the pooled entry, groups ascending within a window.
__global__ __launch_bounds__(WAVE) void target_summary_kernel(const TargetCells tc, const int W, const int G, double* summary) {
    const int SW = sepaihrd_score::summary_width(tc.L);
    const int idx = (int)(blockIdx.x * (unsigned)WAVE + threadIdx.x);
    if (idx >= sepaihrd_targets::N_SERIES * (G + 1) * SW) return;
    const int e = idx / SW, f = idx % SW;
    summary[idx] = sepaihrd_targets::target_summary_field(tc.scores, tc.obs, (size_t)tc.counts[1], W, G, tc.L, e / (G + 1), e % (G + 1), f);
}

bool target_args_ok(const PredictiveArgs& a, const PredictiveTargetArgs& t) {
    return a.S > 0 && a.R > 0 && a.n > 0 && a.Tp > 0 && a.N_pad > 0 && segment_pad_valid((size_t)a.S * a.R, (size_t)a.N_pad) && t.G >= 1 &&
           t.G <= a.n && t.window >= 1 && t.origin >= 0 && t.W >= 1 && t.W == sepaihrd_targets::window_count(a.Tp, t.window, t.origin) &&
           (size_t)6 * t.W * t.G < ((size_t)1 << 31) && t.tvals != nullptr && t.age_group != nullptr;
}

}  // namespace

int launch_predictive_target_draws(const PredictiveArgs& a, const PredictiveTargetArgs& t, const double* d_k_used, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the grid's y dimension holds at most 65 535 blocks
    if (!target_args_ok(a, t) || t.n_launch < 1 || t.n_launch > a.n || a.n > 65535 || t.launch_age == nullptr || d_k_used == nullptr ||
        (uint64_t)3 * a.Tp * a.n >= ((uint64_t)1 << 32))
        return -4;
    const size_t segments = (size_t)6 * t.W * t.G;
    if (hipMemsetAsync(t.tvals, 0, segments * (size_t)a.N_pad * sizeof(double), st) != hipSuccess) return -3;
    hipLaunchKernelGGL(predictive_target_draw_kernel, dim3((unsigned)((a.N_pad + DRAW_BLOCK - 1) / DRAW_BLOCK), (unsigned)t.n_launch, 3u),
                       dim3(DRAW_BLOCK), 0, st, a, t, d_k_used);
    if (t.target_draws != nullptr) {
        const size_t work = (size_t)a.S * a.R * 3 * t.W * t.G;
        hipLaunchKernelGGL(predictive_target_gather_kernel, dim3((unsigned)((work + DRAW_BLOCK - 1) / DRAW_BLOCK)), dim3(DRAW_BLOCK), 0, st, a, t);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_predictive_target_scores(const PredictiveArgs& a, const PredictiveTargetArgs& t, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!target_args_ok(a, t) || t.n_levels < 0 || t.n_levels > sepaihrd_score::MAX_LEVELS || (t.n_levels > 0 && !t.levels) || !t.q_out ||
        !t.target_obs || !t.target_scores || !t.summary || !t.exact || a.n_probs < 1 || !a.probs)
        return -4;
    const int segments = 6 * t.W * t.G, pad = a.N_pad;
    const TargetCells tc{segments, t.W * t.G, t.n_levels, a.n_probs, a.counts, a.probs, t.target_obs, t.levels,
                         t.q_out, t.target_scores, t.pit_out, t.exact};
    hipLaunchKernelGGL(predictive_target_observed_kernel, dim3((unsigned)((3 * t.G + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a, t);
    const SegmentPlan plan = plan_of_pad((size_t)pad);
    if (plan.in_lds) {
        const size_t lds = plan.pad * sizeof(double) + SCORE_RED_BYTES;
        if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(&target_sort_score_kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return -3;
        const int threads = plan.pad / 2 < 1024 ? (int)(plan.pad / 2) : 1024;
        hipLaunchKernelGGL(target_sort_score_kernel, dim3((unsigned)segments), dim3(threads), lds, st, tc, t.tvals, pad);
        if (hipGetLastError() != hipSuccess) return -3;
    } else {
        const int rc = sort_segments_global_for(t.tvals, segments, pad, a.sort_scratch, a.sort_scratch_doubles, stream, [&](int first, int ng) {
            hipLaunchKernelGGL(target_score_sorted_kernel, dim3((unsigned)ng), dim3(SCORE_SORTED_BLOCK), 0, st, tc, a.sort_scratch, pad, first);
        });
        if (rc != 0) return rc;
    }
    const int fields = sepaihrd_targets::N_SERIES * (t.G + 1) * sepaihrd_score::summary_width(t.n_levels);
    hipLaunchKernelGGL(target_summary_kernel, dim3((unsigned)((fields + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, tc, t.W, t.G, t.summary);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd
