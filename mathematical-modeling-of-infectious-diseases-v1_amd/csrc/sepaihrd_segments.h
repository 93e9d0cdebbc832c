// csrc/sepaihrd_segments.h -- how the ensemble entry points pad and sort their segments.  Host only, no HIP type: the one
// statement of the rule for the C ABI code that sizes the buffers (sepaihrd_capi.cpp, sepaihrd_sir_capi.cpp,
// sepaihrd_stoch_sir.hip) and for the launchers that check what they are handed (sepaihrd_segment_sort.inc and its includers).
//
// A segment holds `count` values of one (series, time, age) cell, one per sample or replicate, padded with +inf to `pad`:
//   count <= ENSEMBLE_MAX_SAMPLES   pad = the power of two >= max(count, 64); one workgroup sorts the segment in LDS
//   beyond                          pad = count rounded up to whole wavefronts; the segments are sorted in global memory by
//                                   the segmented radix sort, in groups that fit a scratch buffer
#pragma once
#include <algorithm>
#include <cstddef>

#include "sepaihrd_device.h"

namespace sepaihrd {

struct SegmentPlan {
    size_t pad;   // doubles between two segments
    bool in_lds;  // sorted in LDS; otherwise in global memory
};

inline SegmentPlan plan_segments(size_t count) {
    if (count > (size_t)ENSEMBLE_MAX_SAMPLES) return {(count + WAVE - 1) / WAVE * WAVE, false};
    size_t pad = WAVE;
    while (pad < count) pad <<= 1;
    return {pad, true};
}

// the plan a launcher reads back from the pad it was handed
inline SegmentPlan plan_of_pad(size_t pad) { return {pad, pad <= (size_t)ENSEMBLE_MAX_SAMPLES}; }

// is `pad` one that plan_segments gives for some count >= `count`
inline bool segment_pad_valid(size_t count, size_t pad) {
    if (pad < (size_t)WAVE || count > pad) return false;
    return plan_of_pad(pad).in_lds ? (pad & (pad - 1)) == 0 : pad % WAVE == 0;
}

// scratch of the global sort for a table of `largest_table_doubles`: whole segments, up to 2 GiB, at least one; none in LDS
inline size_t sort_scratch_doubles(const SegmentPlan& plan, size_t largest_table_doubles) {
    if (plan.in_lds) return 0;
    return std::max(plan.pad, std::min(largest_table_doubles, (size_t)1 << 28) / plan.pad * plan.pad);
}

}  // namespace sepaihrd
