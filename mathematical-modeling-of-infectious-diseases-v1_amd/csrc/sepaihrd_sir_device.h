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

}  // namespace sepaihrd
