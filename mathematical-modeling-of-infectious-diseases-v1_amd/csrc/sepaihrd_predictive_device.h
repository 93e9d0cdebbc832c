// csrc/sepaihrd_predictive_device.h -- what csrc/sepaihrd_capi.cpp (sepaihrd_ensemble_predictive and its dispersed and scored
// forms), csrc/sepaihrd_predictive.hip (the counts, the mid-PIT counts), csrc/sepaihrd_predictive_nb.hip (the dispersions, the draw
// kernel) and csrc/sepaihrd_ensemble.hip (the segment sorts, the quantiles and the scores) share.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sepaihrd {

// Replicated data of a posterior ensemble: draw (s, r) sits in slot s R + r of every (series, time, age) segment of
// vals[6 Tp n][N_pad]; slots of samples whose integration failed and slots S R .. N_pad - 1 hold +inf and sort last.
// N_pad: as EnsembleArgs::S_pad for a segment of S R values.
struct PredictiveArgs {
    int S, R, N_pad;
    int lpc, n, T, Tp, runup_offset;  // lanes per chain, ages, output times, output times >= 0, index of the first of them
    uint64_t seed;
    const double* cum;         // the integrator's parked daily increments: cum_index()
    const int32_t* wstatus;    // [S] integrator status
    const double* grid;        // DevProblem::grid: the observations of output time k and age i at grid[(k lpc + i) 4 + series]
    double* vals;              // [6 Tp n][N_pad]
    double* means;             // [S][3][Tp][n] device or null
    double* draws;             // [S][R][3][Tp][n] device or null
    int n_probs;
    const double* probs;       // [n_probs] device
    double* q_out;             // [6][n_probs][Tp][n] device
    double* pit_out;           // [3][Tp][n] device or null
    int32_t* counts;           // [2] device: valid samples, valid samples x R (the draws of a segment)
    double* sort_scratch;      // as EnsembleArgs
    size_t sort_scratch_doubles;
};
// The steps of a draw phase, in the order sepaihrd_capi.cpp's predictive_call issues them.  Each returns 0, -3 (launch failure)
// or -4 (arguments).
// 1. the dispersed calls only (csrc/sepaihrd_predictive_nb.hip): the dispersion of every sample into d_k_used
//    [S][3] (sepaihrd_nb_ll_rows_kernel's rule; a sample with a NaN k becomes a failed one in d_wstatus = a.wstatus)
struct DevProblem;
struct NbDispersion;
int launch_predictive_nb_k(const PredictiveArgs& a, const DevProblem& pb, const double* d_theta, const NbDispersion& disp, double* d_k_used,
                           int32_t* d_wstatus, void* stream);
// 2. the counts of valid samples and draws (csrc/sepaihrd_predictive.hip)
int launch_predictive_counts(const PredictiveArgs& a, void* stream);
// 3. the draws into vals / means / draws, one lane per (draw, age, series) (csrc/sepaihrd_predictive_nb.hip): negative-binomial
//    with the dispersions of d_k_used, Poisson where it is null -- or launch_predictive_target_draws
//    (sepaihrd_predictive_targets_device.h)
int launch_predictive_draws(const PredictiveArgs& a, const double* d_k_used, void* stream);
// 4. where a.pit_out: the mid-PIT of every usable observation from the unsorted daily table (csrc/sepaihrd_predictive.hip)
int launch_predictive_pit(const PredictiveArgs& a, void* stream);
// the quantiles of every segment with the ensemble's sorts and interpolation (csrc/sepaihrd_ensemble.hip)
int launch_predictive_quantiles(const PredictiveArgs& a, void* stream);

// What sepaihrd_ensemble_predictive_scores adds to the quantiles: every daily segment, still sorted, is
// scored against its observation by the rules of csrc/sepaihrd_predictive_score.inc.
struct PredictiveScoreArgs {
    double* obs;             // [3][Tp][n] device: the table the scores are taken against
    bool obs_from_grid;      // obs is filled here with the context's observations (PredictiveArgs::grid, as the PIT kernel reads them)
    const double* levels;    // [n_levels] device
    int n_levels;
    double* cell_scores;     // [3][Tp][n][5 + 4 n_levels] device
    double* summary;         // [3][n + 1][4 + 2 n_levels] device
    double* pit_out;         // [3][Tp][n] device or null: the mid-PIT from the sorted segment's counts
    int32_t* exact;          // [1] device, 1 on entry: set to 0 by a cell whose sums may round
};
// launch_predictive_quantiles with the scores: the same sorts and picks (each segment sorted once), the cell rule on every daily
// segment -- in LDS after the picks, or over the radix sort's scratch -- and the summary walk.  a.pit_out is not read.
int launch_predictive_scores(const PredictiveArgs& a, const PredictiveScoreArgs& sa, void* stream);

}  // namespace sepaihrd
