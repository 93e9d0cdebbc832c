// csrc/sepaihrd_predictive_targets_device.h -- what csrc/sepaihrd_capi.cpp (sepaihrd_ensemble_predictive_targets) and
// csrc/sepaihrd_predictive_targets.hip share.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_predictive_device.h"

namespace sepaihrd {

// The targets of one call (the rule: csrc/sepaihrd_predictive_targets.inc).  Draw (s, r) sits in slot
// s R + r of every target segment of tvals[6 W G][N_pad]; the slots of failed samples and the padding hold +inf.  The fields of
// PredictiveArgs the call still uses are its sizes, seed, cum, wstatus, grid, means, draws, probs, counts and sort scratch; its
// vals, q_out and pit_out are not read.
struct PredictiveTargetArgs {
    int W, G, window, origin;
    int n_launch;               // ages the draw kernel launches
    const int32_t* launch_age;  // [n_launch] device: every age where means or draws are wanted, else the ages of a group
    const int32_t* age_group;   // [n] device
    double* tvals;              // [6 W G][N_pad] device
    double* q_out;              // [6][n_probs][W][G] device
    double* obs_daily;          // [3][Tp][n] device: the caller's table, or null for the context's observations (PredictiveArgs::grid)
    double* target_obs;         // [6][W][G] device
    const double* levels;       // [n_levels] device
    int n_levels;
    double* target_scores;      // [6][W][G][5 + 4 n_levels] device
    double* summary;            // [6][G + 1][4 + 2 n_levels] device
    double* pit_out;            // [6][W][G] device or null
    double* target_draws;       // [S][R][3][W][G] device or null
    int32_t* exact;             // [1] device, 1 on entry
};
// Step 3 of a draw phase (sepaihrd_predictive_device.h) for the targets: the table zeroed, then the draws of
// sepaihrd_ensemble_predictive_scores summed into it, and target_draws gathered from it where wanted.  0, -3, -4.
int launch_predictive_target_draws(const PredictiveArgs& a, const PredictiveTargetArgs& t, const double* d_k_used, void* stream);
// the observed targets, every segment sorted once with its quantile picks and scores, and the summary walk.  0, -3, -4.
int launch_predictive_target_scores(const PredictiveArgs& a, const PredictiveTargetArgs& t, void* stream);

}  // namespace sepaihrd
