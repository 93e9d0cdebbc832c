// csrc/sepaihrd_nb_objective_device.h -- what the C ABI (csrc/sepaihrd_capi.cpp) asks of the negative-binomial likelihood pass
// (csrc/sepaihrd_nb_objective.hip).  Internal: not part of the C ABI.
#pragma once
#include <stdint.h>

#include "sepaihrd_device.h"

namespace sepaihrd {

// One dispersion per observed series (H, ICU, D): the theta index that calibrates it (found at create time), or -1 and the
// context's fixed value (+inf: that series keeps the Poisson cell).  A kernel argument by value.
struct NbDispersion {
    int32_t src[3];
    int32_t fused_poisson;  // the context's arithmetic is fma: a Poisson series' cell is one fma, as in that build's Poisson kernels
    double fixed[3];
};
inline bool nb_any_dispersed(const NbDispersion& d) {
    for (int s = 0; s < 3; ++s)
        if (d.src[s] >= 0 || d.fixed[s] <= 1.7976931348623157e308) return true;
    return false;
}

constexpr const char* NB_PASS_KERNEL_NAME = "sepaihrd_nb_ll_rows_kernel";

// The pass over the increments an integrator launch with EvalOutputs::force_split = FORCE_SPLIT_PARK_ONLY parked for B chains:
// writes out.loglik, out.status and out.ll_parts.  0, -3 (launch failure), -4 (lanes per chain), -5 (no workspace).
int launch_nb_objective_pass(const DevProblem& pb, const double* d_theta, int B, const EvalOutputs& out, const NbDispersion& disp, void* stream);
int kernel_info_nb_pass(const DevProblem& pb, LaunchInfo* info);

}  // namespace sepaihrd
