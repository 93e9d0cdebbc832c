// csrc/sepaihrd_segment_sort.inc -- sort and pick, and sort, pick and score: the one text of the segment kernels and their
// drivers, compiled by csrc/sepaihrd_ensemble.hip and csrc/sepaihrd_predictive_targets.hip.  Every summary across samples sorts
// segments of values (+inf padding last) and picks a few numbers from each.  A pick is a functor passed to the kernels by value,
// carrying its caller's arguments: picks() numbers per segment, operator()(sid, p, sorted segment) stores number p of segment
// sid, SORTED_BLOCK is the workgroup of the sorted kernel.  The scored form (DESIGN.md sections 6q, 6r) also takes the scoring
// rules of csrc/sepaihrd_predictive_score.inc from the leading segments while they are still sorted.  How a segment is padded and
// when it is sorted in global memory instead of LDS: csrc/sepaihrd_segments.h.  Everything here is local to the including unit,
// which is compiled with -ffp-contract=off (sepaihrd_quantile.inc and sepaihrd_predictive_score.inc need it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "sepaihrd_bitonic.inc"  // lds_bitonic_sort: the load into LDS and the network
#include "sepaihrd_device.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_predictive_score.inc"
#include "sepaihrd_quantile.inc"
#include "sepaihrd_segments.h"

namespace sepaihrd {
namespace {

// one workgroup per segment of Np doubles: bitonic sort in LDS, then thread p stores pick p
template <class Pick>
__global__ void segment_sort_pick_kernel(const Pick pick, const double* vals, const int Np) {
    extern __shared__ double seg[];
    const size_t sid = blockIdx.x;
    lds_bitonic_sort(seg, vals + sid * (size_t)Np, Np);
    for (int p = threadIdx.x; p < pick.picks(); p += blockDim.x) pick(sid, p, seg);
}

// Segments beyond the LDS sort: those of a group were sorted in global memory by the library's segmented radix sort; one
// thread per (segment of the group, pick).
template <class Pick>
__global__ __launch_bounds__(Pick::SORTED_BLOCK) void segment_pick_sorted_kernel(const Pick pick, const double* sorted, const int Np,
                                                                                 const int first_segment, const int n_group) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int picks = pick.picks();
    if (idx >= (size_t)n_group * picks) return;
    const int g = (int)(idx / picks), p = (int)(idx % picks);
    pick((size_t)(first_segment + g), p, sorted + (size_t)g * Np);
}

// its launch over the `ng` segments from `first` on that the radix sort has left in `sorted`
template <class Pick>
void launch_pick_sorted(const Pick& pick, const double* sorted, int pad, int first, int ng, hipStream_t st) {
    constexpr int BLOCK = Pick::SORTED_BLOCK;
    const size_t work = (size_t)ng * pick.picks();
    hipLaunchKernelGGL(segment_pick_sorted_kernel<Pick>, dim3((unsigned)((work + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, pick, sorted, pad,
                       first, ng);
}

// Segments of S_pad doubles (more than the LDS sort holds) sorted in groups by rocPRIM's segmented radix sort into
// `scratch`; pick(first, n_group) launches the interpolation of each sorted group.  Synchronises the stream.
template <class Pick>
int sort_segments_global(const double* vals, int segments, int S_pad, double* scratch, size_t scratch_doubles, hipStream_t st,
                         Pick pick) {
    // group size bounded by the scratch buffer
    int group = (int)(scratch_doubles / (size_t)S_pad);
    if (group > segments) group = segments;
    if (group < 1 || (size_t)group * S_pad >= (size_t)1 << 31) return -4;
    std::vector<unsigned> offs((size_t)group + 1);
    for (int g = 0; g <= group; ++g) offs[(size_t)g] = (unsigned)((size_t)g * S_pad);
    DeviceBuf offs_buf, tmp;  // freed on return, after the stream has been synchronised
    unsigned* d_offs = nullptr;
    if (!offs_buf.get(&d_offs, offs.size())) return -3;
    int rc = 0;
    if (hipMemcpyAsync(d_offs, offs.data(), offs.size() * sizeof(unsigned), hipMemcpyHostToDevice, st) != hipSuccess) rc = -3;
    for (int first = 0; first < segments && rc == 0; first += group) {
        const int ng = (segments - first < group) ? segments - first : group;
        const double* in = vals + (size_t)first * S_pad;
        const unsigned size = (unsigned)((size_t)ng * S_pad);
        size_t need = 0;
        if (rocprim::segmented_radix_sort_keys(nullptr, need, in, scratch, size, (unsigned)ng, d_offs, d_offs + 1, 0, 64,
                                               st) != hipSuccess) { rc = -3; break; }
        if (!tmp.reserve(need)) { rc = -3; break; }
        size_t tmp_bytes = tmp.cap;
        if (rocprim::segmented_radix_sort_keys(tmp.p, tmp_bytes, in, scratch, size, (unsigned)ng, d_offs, d_offs + 1, 0, 64,
                                               st) != hipSuccess) { rc = -3; break; }
        pick(first, ng);
    }
    (void)hipStreamSynchronize(st);
    return (rc == 0 && hipGetLastError() == hipSuccess) ? 0 : -3;
}

// what every launcher asks of the segments it is handed: `count` values each, in a pad the plan gives (sepaihrd_segments.h)
bool pad_legal(size_t count, int pad) { return pad > 0 && segment_pad_valid(count, (size_t)pad); }

// the LDS sort of plan.pad doubles (and `extra_bytes` the kernel keeps next to them) needs the kernel's dynamic-LDS limit raised
// above 48 KiB; 0 or -3
int raise_lds_limit(const SegmentPlan& plan, const void* lds_kernel, size_t extra_bytes = 0) {
    const size_t lds = plan.pad * sizeof(double) + extra_bytes;
    if (!plan.in_lds || lds <= 48 * 1024) return 0;
    return hipFuncSetAttribute(lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess ? 0 : -3;
}

// Sort every segment, then pick from it, by the plan's route.  In LDS: launch_lds(threads, lds_bytes) launches `lds_kernel`
// with one workgroup per segment (null: the caller has raised its LDS limit already).  In global memory:
// sort_segments_global with pick(first, n_group).  0, -3 (HIP failure) or -4 (no segment fits the scratch).
template <class LaunchLds, class Pick>
int sort_segments_and_pick(const SegmentPlan& plan, int segments, const double* vals, double* scratch, size_t scratch_doubles,
                           hipStream_t st, const void* lds_kernel, LaunchLds launch_lds, Pick pick) {
    if (!plan.in_lds) return sort_segments_global(vals, segments, (int)plan.pad, scratch, scratch_doubles, st, pick);
    if (lds_kernel != nullptr && raise_lds_limit(plan, lds_kernel) != 0) return -3;
    launch_lds(plan.pad / 2 < 1024 ? (int)(plan.pad / 2) : 1024, plan.pad * sizeof(double));
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// events and the sum that time every sorted pick of a call (launch_stoch_sir_summaries); null: untimed
struct PickTimer {
    hipEvent_t ev0, ev1;
    double* ms;
};

// The one launcher: `segments` segments of vals, `pad` doubles apart, are sorted and `pick` takes its numbers from each.
// lds_limit_raised: the caller has raised the LDS limit of this pick's segment_sort_pick_kernel already.
template <class Pick>
int launch_sort_pick(const Pick& pick, const double* vals, int pad, int segments, double* scratch, size_t scratch_doubles, hipStream_t st,
                     bool lds_limit_raised = false, const PickTimer* timer = nullptr) {
    return sort_segments_and_pick(
        plan_of_pad((size_t)pad), segments, vals, scratch, scratch_doubles, st,
        lds_limit_raised ? nullptr : reinterpret_cast<const void*>(&segment_sort_pick_kernel<Pick>),
        [&](int threads, size_t lds) {
            hipLaunchKernelGGL(segment_sort_pick_kernel<Pick>, dim3((unsigned)segments), dim3(threads), lds, st, pick, vals, pad);
        },
        [&](int first, int ng) {
            if (timer) (void)hipEventRecord(timer->ev0, st);
            launch_pick_sorted(pick, scratch, pad, first, ng, st);
            if (timer) {
                float ms = 0.0f;
                (void)hipEventRecord(timer->ev1, st);
                if (hipEventSynchronize(timer->ev1) == hipSuccess && hipEventElapsedTime(&ms, timer->ev0, timer->ev1) == hipSuccess)
                    *timer->ms += (double)ms;
            }
        });
}

// ---- the scored form: the leading `scored` segments of the table are, still sorted, scored against their observations ----

// what the score kernels take by value: the scored segments, the draw count and where the scores go
struct ScoreArgs {
    int scored, L;          // segments 0 .. scored - 1 are scored; interval levels
    const int32_t* counts;  // PredictiveArgs::counts: [1] = draws per segment
    const double* obs;      // [scored]
    const double* levels;   // [L]
    double* scores;         // [scored][5 + 4 L]
    double* pit_out;        // [scored] or null
    int32_t* exact;
};

constexpr int SCORE_MAX_WAVES = 16;                                                // of a 1024-lane workgroup
constexpr int SCORE_SUMS = 6;                                                      // S1, S2, S_less, G, n_less, n_eq
constexpr size_t SCORE_RED_BYTES = SCORE_MAX_WAVES * SCORE_SUMS * sizeof(double);  // 768: the cross-wave step

// v of lane + off added down to lane 0 of the wave; lanes past `active` (a workgroup of 32 lanes is half a wave) add nothing
template <class T>
__device__ __forceinline__ T wave_sum(T v, const int lane, const int active) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const T o = __shfl_down(v, off, WAVE);
        if (lane + off < active) v += o;
    }
    return v;
}

// The sums of sorted segment `seg` (LDS or device memory; m valid draws first) against the segment's observation, reduced by the
// whole workgroup -- lane-strided reads of consecutive doubles: conflict-free in LDS, coalesced in device memory -- then the cell
// rule by one lane.  Every partial sum is a sum of integers and exact below 2^53, so the shape of the reduction does not show;
// where sums_exact fails the segment says so in *exact.  red: SCORE_RED_BYTES of LDS.
__device__ __forceinline__ void score_sorted_segment(const ScoreArgs& sc, const size_t sid, const double* seg, double* red) {
    const int tid = threadIdx.x, BS = blockDim.x;
    const int m = sc.counts[1];
    const double y = sc.obs[sid];
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
    sepaihrd_score::cell_rule(seg, (size_t)m, y, total, sc.levels, sc.L, sc.scores + sid * (size_t)sepaihrd_score::cell_width(sc.L));
    if (sc.pit_out != nullptr) sc.pit_out[sid] = sepaihrd_score::pit_of(total, (size_t)m, y);
    if (m > 0 && !sepaihrd_score::sums_exact((size_t)m, seg[m - 1])) *sc.exact = 0;
}

// segment_sort_pick_kernel that then scores a scored segment while it is still in LDS.  Dynamic LDS: Np doubles, then
// SCORE_RED_BYTES.
template <class Pick>
__global__ void segment_sort_score_kernel(const Pick pick, const ScoreArgs sc, const double* vals, const int Np) {
    extern __shared__ double seg[];
    const size_t sid = blockIdx.x;
    lds_bitonic_sort(seg, vals + sid * (size_t)Np, Np);
    for (int p = threadIdx.x; p < pick.picks(); p += blockDim.x) pick(sid, p, seg);
    if (sid < (size_t)sc.scored) score_sorted_segment(sc, sid, seg, seg + Np);
}

// beyond the LDS sort: one workgroup per scored segment of a group the radix sort has left in `sorted`
constexpr int SCORE_SORTED_BLOCK = 256;
__global__ __launch_bounds__(SCORE_SORTED_BLOCK) void segment_score_sorted_kernel(const ScoreArgs sc, const double* sorted, const int Np,
                                                                                  const int first_segment) {
    __shared__ double red[SCORE_MAX_WAVES * SCORE_SUMS];
    score_sorted_segment(sc, (size_t)first_segment + blockIdx.x, sorted + (size_t)blockIdx.x * Np, red);
}

// launch_sort_pick with the scores: each segment is sorted once; in LDS the workgroup that sorted it reduces its sums before it
// leaves, beyond the LDS sort the picks of a group are followed by a workgroup per scored segment over the radix sort's scratch.
template <class Pick>
int launch_sort_pick_score(const Pick& pick, const ScoreArgs& sc, const double* vals, int pad, int segments, double* scratch,
                           size_t scratch_doubles, hipStream_t st) {
    const SegmentPlan plan = plan_of_pad((size_t)pad);
    if (raise_lds_limit(plan, reinterpret_cast<const void*>(&segment_sort_score_kernel<Pick>), SCORE_RED_BYTES) != 0) return -3;
    return sort_segments_and_pick(
        plan, segments, vals, scratch, scratch_doubles, st, nullptr,
        [&](int threads, size_t lds) {
            hipLaunchKernelGGL(segment_sort_score_kernel<Pick>, dim3((unsigned)segments), dim3(threads), lds + SCORE_RED_BYTES, st, pick, sc,
                               vals, pad);
        },
        [&](int first, int ng) {
            launch_pick_sorted(pick, scratch, pad, first, ng, st);
            const int scored = (first + ng < sc.scored ? first + ng : sc.scored) - first;  // the group's segments that are scored
            if (scored > 0)
                hipLaunchKernelGGL(segment_score_sorted_kernel, dim3((unsigned)scored), dim3(SCORE_SORTED_BLOCK), 0, st, sc, scratch, pad, first);
        });
}

}  // namespace
}  // namespace sepaihrd
