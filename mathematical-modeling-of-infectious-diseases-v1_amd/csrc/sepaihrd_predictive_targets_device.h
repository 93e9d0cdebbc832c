// csrc/sepaihrd_predictive_targets_device.h -- what csrc/sepaihrd_capi.cpp (sepaihrd_ensemble_predictive_targets) and
// csrc/sepaihrd_predictive_targets.hip share, and the two launchers that unit borrows from its neighbours.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>

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
// the table zeroed, then the draws of sepaihrd_ensemble_predictive_scores summed into it (a.counts and k_used must be ready:
// launch_predictive_nb_k, launch_predictive_counts), and target_draws gathered from it where wanted.  0, -3, -4.
int launch_predictive_target_draws(const PredictiveArgs& a, const PredictiveTargetArgs& t, const double* d_k_used, void* stream);
// the observed targets, every segment sorted once with its quantile picks and scores, and the summary walk.  0, -3, -4.
int launch_predictive_target_scores(const PredictiveArgs& a, const PredictiveTargetArgs& t, void* stream);

// csrc/sepaihrd_predictive_nb.hip: the first step of launch_predictive_draws_nb alone, every sample's dispersion into d_k_used
// (a sample with a NaN k becomes a failed one in d_wstatus)
int launch_predictive_nb_k(const PredictiveArgs& a, const DevProblem& pb, const double* d_theta, const NbDispersion& disp, double* d_k_used,
                           int32_t* d_wstatus, void* stream);
// csrc/sepaihrd_ensemble.hip: its sort_segments_global (the segmented radix sort of segments beyond the LDS sort, in groups that fit
// the scratch) for a caller outside that unit; pick(first, n_group) launches what reads each sorted group from `scratch`
int sort_segments_global_for(const double* vals, int segments, int S_pad, double* scratch, size_t scratch_doubles, void* stream,
                             const std::function<void(int, int)>& pick);

}  // namespace sepaihrd
