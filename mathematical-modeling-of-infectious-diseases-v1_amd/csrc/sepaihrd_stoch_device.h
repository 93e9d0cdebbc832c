// csrc/sepaihrd_stoch_device.h -- what csrc/sepaihrd_stoch_sir.hip (step kernel, C ABI) and csrc/sepaihrd_ensemble.hip (the
// segment sorts and the summaries) share.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sepaihrd {

// One chunk of the time axis: vals [segments][R_pad], segment = (group 3 + compartment) chunk_steps + local step, the
// replicates first and +inf after them.  R_pad: plan_segments(R).pad (csrc/sepaihrd_segments.h); beyond the LDS sort the
// segments are sorted into sort_scratch by the segmented radix sort.
struct StochSummaryArgs {
    int G, R, R_pad;
    int chunk_steps, step0, steps;  // this chunk's rows are step0 .. step0 + chunk_steps - 1 of `steps`
    const double* vals;
    double* stats;                  // [G][4][3][steps]
    double* sort_scratch;
    size_t sort_scratch_doubles;
    void* ev[2];                    // two hipEvent_t and an accumulator: the global path times its summary kernels with
    double* summary_ms;             // them (one wait per sorted group); all null: not timed
};
int launch_stoch_sir_summaries(const StochSummaryArgs& a, void* stream);

}  // namespace sepaihrd
