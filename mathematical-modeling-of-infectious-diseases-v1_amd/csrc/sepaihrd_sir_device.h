// csrc/sepaihrd_sir_device.h -- structures shared by the C-ABI host code of the age-structured SIR objective
// (sepaihrd_sir_capi.cpp) and its kernels (sepaihrd_sir.hip).  Internal: not part of the C ABI.
#pragma once
#include <stdint.h>

namespace sepaihrd {

constexpr int SIR_COMP = 3;  // S, I, R

// Problem data resident in HBM (uploaded once per ctx).  Per-age tables are padded to `lpc` (n rounded up to a power of
// two): padded ages have N = 0, zero state, zero rates, a zero contact row and column and zero observations; their
// Poisson terms are masked.
struct SirDevProblem {
    int32_t n, lpc, T, P, max_attempts;
    int32_t obs_not_finite;      // max(obs, 0) holds a non-finite entry: every evaluation is -inf, status 1
    double abs_tol, rel_tol, dt_hint, max_gap;
    double q, scale;             // the values of the fields that are not calibrated
    const double* times;         // [T]
    const double* N;             // [lpc]
    const double* C;             // [lpc][lpc] baseline contact matrix, row i at C + i lpc
    const double* gamma;         // [lpc]
    const double* init_state;    // [3][lpc]
    const double* obs;           // [T][lpc]  max(observed, 0)
    const int32_t* param_field;  // [P] SEPAIHRD_SIR_F_*
    const int32_t* param_index;  // [P] age class of a gamma entry
};

struct SirOutputs {
    double* loglik;     // [B]
    int32_t* status;    // [B] or null
    int32_t* n_accept;  // [B] or null
    int32_t* n_reject;  // [B] or null
    double* traj;       // [B][T][3 n] or null, state layout [S(n), I(n), R(n)]
};

struct SirLaunchInfo {
    int vgprs, sgprs, lds_static, scratch;
    const char* name;
};

// implemented twice, once per arithmetic mode (separate translation units of sepaihrd_sir.hip).
// 0, -3 launch failure, -4 lanes-per-chain or solver not built
int launch_sir_eval_strict(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, void* stream);
int launch_sir_eval_fma(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, void* stream);

// ---- posterior ensemble and intervention scenarios (sepaihrd_sir_scenario_ensemble) ----
constexpr int SIR_MAX_EVENTS = 8;                    // include/sepaihrd_hip.h SEPAIHRD_SIR_MAX_EVENTS
constexpr int SIR_EV_CONTACT = 0, SIR_EV_TRANSMISSION = 1;  // SEPAIHRD_SIR_EV_*
constexpr int SIR_ENS_SERIES = 3;                    // incidence, prevalence, cumulative infections
constexpr int SIR_ENS_SCALARS = 6;                   // metric columns before the per-age pairs
struct SirEvent {                                    // layout of struct sepaihrd_sir_event
    int32_t time_index, kind;
    double value;
};
// What the ensemble build of the integrator (csrc/Makefile sir_ens_*.o, -DSEPAIHRD_SIR_ENSEMBLE=1) takes on top of the
// problem: chain c is sample c % S of scenario c / S; its observer stores the three series of every output time into
//   vals[((scenario 3 + series) T + t) (n + 1) + column][S_pad],   column n = the age total
// (sample-minor: every sortable segment is contiguous, the chains of a wavefront write adjacent doubles of a row).
struct SirEnsArgs {
    int32_t S, S_pad;
    const SirEvent* events;    // [K][SIR_MAX_EVENTS] device, sorted by time_index
    const int32_t* n_events;   // [K] device
    double* vals;
};
// 0, -3, -4 as above.  out.loglik and out.traj are not written by this build.
int launch_sir_ens_strict(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, const SirEnsArgs& ens,
                          void* stream);
int launch_sir_ens_fma(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, const SirEnsArgs& ens,
                       void* stream);

// The passes over the stored series (csrc/sepaihrd_ensemble.hip): rows of failed samples and of the padding become +inf,
// the metric table is formed from the series and theta, every segment is sorted and interpolated (the quantile kernels of
// sepaihrd_ensemble_quantiles), then the scenario summaries (launch_scenario_summaries).
struct SirEnsSummaryArgs {
    int K, S, S_pad, n, lpc, T, P, n_probs;
    const SirDevProblem* pb;   // host pointer to the ctx's problem (kernel argument by value)
    const double* theta;       // [S][P] device (scenario 0's block)
    const int32_t* status;     // [K][S] device, the integrator's
    double* vals;              // as SirEnsArgs
    const double* probs;       // [n_probs] device
    double* q_out;             // [K][3][n_probs][T][n + 1] device
    int32_t* n_valid;          // [K] device
    double* metrics;           // [K][S][6 + 2 n] device
    double* r0;                // [S] device scratch: R0 of every sample
    double* svals;             // [2 K W][S_pad] scratch of the scenario summaries
    int32_t* counts;           // [2 K]
    double* summary_out;       // [K][W][2 + n_probs]
    double* diff_out;          // [K][W][n_probs]
    double* sort_scratch;      // as EnsembleArgs
    size_t sort_scratch_doubles;
    void* ev_after_metrics;    // optional hipEvent_t recorded between the fix-up / metric passes and the sorts
};
int launch_sir_ensemble_summaries(const SirEnsSummaryArgs& a, void* stream);

}  // namespace sepaihrd
