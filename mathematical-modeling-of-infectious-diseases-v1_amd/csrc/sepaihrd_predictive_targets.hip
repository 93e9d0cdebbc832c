// csrc/sepaihrd_predictive_targets.hip -- scores of the posterior predictive draws on weekly and age-group totals on gfx950
// (sepaihrd_ensemble_predictive_targets).  The rule is csrc/sepaihrd_predictive_targets.inc, the text the
// host twin compiles too.  The draw kernel takes its lanes and its draw from csrc/sepaihrd_predictive_draw.inc, as the daily draw
// kernel does, and holds the window total and its running sum in two registers that it adds into the target table; the sort, the
// picks and the scores over the 6 W G target segments are the kernels and the launcher of csrc/sepaihrd_segment_sort.inc with this
// unit's pick.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sepaihrd_device.h"
#include "sepaihrd_predictive_draw.inc"
#include "sepaihrd_predictive_targets.inc"
#include "sepaihrd_predictive_targets_device.h"
#include "sepaihrd_segment_sort.inc"

namespace sepaihrd {
namespace {

// The lanes and the draw of csrc/sepaihrd_predictive_draw.inc with the launched ages on the grid's y dimension.  The lane sums the
// rows of a window in `win` and the windows in `run`; at a window's last row it adds both into the slots of its group's two
// targets.  The lanes of a group's ages sit in different workgroups and meet there: the sums are of integers, exact below 2^53,
// so the order the adds arrive in does not show.  The table was zeroed before the launch.  Consecutive lanes add to consecutive
// doubles, nothing is returned.  A failed or padding slot receives +inf from every lane that owns it.  Rows of no window are
// drawn only where a.draws is wanted, and a lane of an age outside every group (launched only where means or draws are wanted)
// adds nothing.
__global__ __launch_bounds__(DRAW_BLOCK) void predictive_target_draw_kernel(const PredictiveArgs a, const PredictiveTargetArgs tg,
                                                                            const double* __restrict__ k_used) {
    DrawLane l;
    if (!draw_lane(a, k_used, tg.launch_age[blockIdx.y], l)) return;
    const int g = tg.age_group[l.age];
    const size_t seg_stride = (size_t)a.N_pad;
    double win = l.ok ? 0.0 : INFINITY, run = win;
    int v = 0, rows = 0;  // the window the next target row belongs to, and its rows already summed
    for (int t = 0; t < a.Tp; ++t) {
        const bool in_target = g >= 0 && t >= tg.origin && v < tg.W;
        const double y = draw_row(a, l, t, in_target);
        if (in_target) {
            if (l.ok) win += y;
            if (++rows == tg.window) {
                run += win;
                unsafeAtomicAdd(tg.tvals + sepaihrd_targets::target_index(l.ser, v, g, tg.W, tg.G) * seg_stride + l.idx, win);
                unsafeAtomicAdd(tg.tvals + sepaihrd_targets::target_index(l.ser + 3, v, g, tg.W, tg.G) * seg_stride + l.idx, run);
                win = l.ok ? 0.0 : INFINITY;
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

// quantile p of sorted target segment `sid` by the rule of pred_quantiles, into q_out [6][n_probs][W][G]
struct TargetPick {
    static constexpr int SORTED_BLOCK = 256;
    int WG, n_probs;
    const int32_t* counts;  // PredictiveArgs::counts: [1] = draws per segment
    const double* probs;    // [n_probs]
    double* q_out;
    __host__ __device__ int picks() const { return n_probs; }
    __device__ void operator()(size_t sid, int p, const double* seg) const {
        const int m = counts[1];
        const size_t k = sid / (size_t)WG, vg = sid % (size_t)WG;
        q_out[(k * n_probs + p) * (size_t)WG + vg] = m > 0 ? sepaihrd_quantile::sorted_quantile(seg, (size_t)m, probs[p]) : (double)NAN;
    }
};

// One lane per (series of 6, group or pooled, field), as score_summary_kernel: the walk of target_summary_field over the series'
// targets, windows ascending and, for the pooled entry, groups ascending within a window.
__global__ __launch_bounds__(WAVE) void target_summary_kernel(const ScoreArgs sc, const int W, const int G, double* summary) {
    const int SW = sepaihrd_score::summary_width(sc.L);
    const int idx = (int)(blockIdx.x * (unsigned)WAVE + threadIdx.x);
    if (idx >= sepaihrd_targets::N_SERIES * (G + 1) * SW) return;
    const int e = idx / SW, f = idx % SW;
    summary[idx] = sepaihrd_targets::target_summary_field(sc.scores, sc.obs, (size_t)sc.counts[1], W, G, sc.L, e / (G + 1), e % (G + 1), f);
}

bool target_args_ok(const PredictiveArgs& a, const PredictiveTargetArgs& t) {
    return a.S > 0 && a.R > 0 && a.n > 0 && a.Tp > 0 && pad_legal((size_t)a.S * a.R, a.N_pad) && t.G >= 1 && t.G <= a.n && t.window >= 1 &&
           t.origin >= 0 && t.W >= 1 && t.W == sepaihrd_targets::window_count(a.Tp, t.window, t.origin) &&
           (size_t)6 * t.W * t.G < ((size_t)1 << 31) && t.tvals != nullptr && t.age_group != nullptr;
}

}  // namespace

int launch_predictive_target_draws(const PredictiveArgs& a, const PredictiveTargetArgs& t, const double* d_k_used, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!target_args_ok(a, t) || !draw_args_ok(a) || t.n_launch < 1 || t.n_launch > a.n || t.launch_age == nullptr || d_k_used == nullptr) return -4;
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
    const int segments = 6 * t.W * t.G;  // every one of them is scored
    const TargetPick pick{t.W * t.G, a.n_probs, a.counts, a.probs, t.q_out};
    const ScoreArgs sc{segments, t.n_levels, a.counts, t.target_obs, t.levels, t.target_scores, t.pit_out, t.exact};
    hipLaunchKernelGGL(predictive_target_observed_kernel, dim3((unsigned)((3 * t.G + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a, t);
    const int rc = launch_sort_pick_score(pick, sc, t.tvals, a.N_pad, segments, a.sort_scratch, a.sort_scratch_doubles, st);
    if (rc != 0) return rc;
    const int fields = sepaihrd_targets::N_SERIES * (t.G + 1) * sepaihrd_score::summary_width(t.n_levels);
    hipLaunchKernelGGL(target_summary_kernel, dim3((unsigned)((fields + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, sc, t.W, t.G, t.summary);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd
