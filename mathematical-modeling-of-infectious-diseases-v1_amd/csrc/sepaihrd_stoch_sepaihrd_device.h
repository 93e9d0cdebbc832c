// csrc/sepaihrd_stoch_sepaihrd_device.h -- what csrc/sepaihrd_capi.cpp (sepaihrd_ensemble_stochastic) and
// csrc/sepaihrd_stoch_sepaihrd.hip (the decode and step kernels) share.  The quantiles are launch_predictive_quantiles' over the
// segment table the step kernel fills (csrc/sepaihrd_predictive_device.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_device.h"

namespace sepaihrd {

struct StochEpiArgs {
    int S, R, N_pad;          // samples, replicates per sample, slots of a segment (PredictiveArgs::N_pad)
    int m, keep, W;           // steps per output interval, replicates whose rows go to traj, width of a model-values row
    uint64_t seed;
    const double* theta;      // [S][P] device
    double* values;           // [S][W] device: the rows the replicates run with (csrc/sepaihrd_stoch_sepaihrd.inc RowLayout)
    int32_t* status;          // [S] device: 0, or SEPAIHRD_STATUS_INVALID
    int32_t* counts;          // [2] device: valid samples, valid samples x R
    int32_t* extinct_count;   // [S] device, zeroed by the launch: replicates with E + P + A + I = 0 in every age at the last time
    double* vals;             // [6 Tp n][N_pad] the segment table: replicate r of sample s in slot s R + r
    double* traj;             // [S][keep][T][11][n] device or null
    double* final_state;      // [S][R][11][n] device or null
};
// theta -> model values, rounded initial state and status of every sample; then counts
int launch_stoch_epi_decode(const DevProblem& pb, const StochEpiArgs& a, void* stream);
// the step kernel: one lane per (replicate, age class)
int launch_stoch_epi_steps(const DevProblem& pb, const StochEpiArgs& a, void* stream);
// What sepaihrd_stochastic_validate and sepaihrd_particle_validate check alike -- the steps per interval, the output times, the
// age classes and the 2^22 bound of the step coordinate: the first refusal's text (without the caller's prefix), or nullptr.
const char* stoch_epi_grid_refusal(int steps_per_interval, int n_times, int T_pos, int n_age);

}  // namespace sepaihrd
