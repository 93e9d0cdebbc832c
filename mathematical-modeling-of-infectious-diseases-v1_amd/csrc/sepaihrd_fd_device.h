// csrc/sepaihrd_fd_device.h -- launch interface of csrc/sepaihrd_fd_gradient.hip (sepaihrd_fd_gradient_batch).
// Internal: not part of the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sepaihrd {

// Largest number of perturbed rows (wanted centres x parameters) one call evaluates: the workspace is
// rows x (P + 2) doubles (2.1 GB at the shipped P = 62) and the evaluator takes the row count as an int.
constexpr size_t FD_MAX_PERTURBED_ROWS = (size_t)1 << 22;

// G wanted centres rows[0..G) (indices into the C centres), P parameters each; every pointer is a device pointer.
struct FdQuotientArgs {
    int32_t C, G, P, n, lpc;
    int32_t mult_index[8];         // parameter index of the E0..D0 multiplier, -1 = not calibrated (1.0)
    const int32_t* rows;           // [G]
    const double* plus;            // [G P][P] the perturbed vectors as evaluated
    const double* eps;             // [G P]
    const double* f_plus;          // [G P] values of the perturbed evaluations
    const int32_t* plus_status;    // [G P]
    const double* value;           // [C] centre values
    const int32_t* centre_status;  // [C]
    const double* init_state;      // [11][lpc] (DevProblem::init_state)
    const double* N;               // [lpc]
    double* grad;                  // [G][P] out
    int32_t* status;               // [C] out, zeroed before the launch
};

// 0, or -3 when the launch failed
int launch_fd_build(const double* d_theta, const int32_t* d_rows, int G, int P, double fd_epsilon, double* d_plus, double* d_eps,
                    void* stream);
int launch_fd_quotient(const FdQuotientArgs& a, void* stream);

}  // namespace sepaihrd
