// csrc/sepaihrd_fd_gradient.hip -- the two small kernels around the evaluator launches of sepaihrd_fd_gradient_batch:
// the builder of the perturbed parameter matrix and the forward-difference quotient.  Both are memory-shaped (one thread
// per element, consecutive lanes on consecutive addresses, grid-stride); neither synchronises anything.
//
// Compiled with -ffp-contract=off in BOTH arithmetic modes of the contexts (csrc/Makefile): the step
// eps_i = fd_epsilon * max(|theta_i|, fd_epsilon) is a product rounded on its own before it is added to theta_i and before
// it divides, as the host computes it (HipSEPAIHRDGradientObjectiveFunction::evaluate_with_gradient) -- the quotient
// magnifies a last-bit difference of the step by 1 / eps.
#include <hip/hip_runtime.h>

#include "sepaihrd_fd_device.h"

namespace sepaihrd {
namespace {

constexpr int FD_BLOCK = 256;
constexpr unsigned FD_MAX_GRID = 2048;  // grid-stride beyond it

unsigned fd_grid(size_t work) {
    const size_t blocks = (work + FD_BLOCK - 1) / FD_BLOCK;
    return (unsigned)(blocks < 1 ? 1 : blocks > FD_MAX_GRID ? FD_MAX_GRID : blocks);
}

// plus[(g P + i) P + k] = theta[rows[g]][k], + eps where k == i; eps[g P + i] written by the thread of the diagonal element.
// The element index runs along k: a wave writes 512 contiguous bytes of `plus` and reads theta rows that sit in cache.
__global__ __launch_bounds__(FD_BLOCK) void fd_build_kernel(const double* __restrict__ theta, const int32_t* __restrict__ rows, int G,
                                                            int P, double fd_epsilon, double* __restrict__ plus,
                                                            double* __restrict__ eps) {
    const size_t total = (size_t)G * P * P;
    for (size_t e = (size_t)blockIdx.x * FD_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * FD_BLOCK) {
        const int k = (int)(e % (size_t)P);
        const size_t row = e / (size_t)P;  // g P + i
        const int i = (int)(row % (size_t)P);
        const int c = rows[row / (size_t)P];
        double v = theta[(size_t)c * P + k];
        if (k == i) {
            const double a = fabs(v);
            const double scale = a < fd_epsilon ? fd_epsilon : a;  // std::max(|theta_i|, fd_epsilon), NaN kept
            const double step = fd_epsilon * scale;
            eps[row] = step;
            v = v + step;
        }
        plus[e] = v;
    }
}

// One thread per (row g, parameter i): the initialStateValid rule on the perturbed vector, the finite tests and the IEEE
// division.  status[c]: maximum over the centre's and the row's perturbed evaluations (zeroed before the launch; the
// atomics fire only for statuses > 0, which are rare).
__global__ __launch_bounds__(FD_BLOCK) void fd_quotient_kernel(FdQuotientArgs a) {
    const size_t total = (size_t)a.G * a.P;
    const size_t first = (size_t)blockIdx.x * FD_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * FD_BLOCK;
    for (size_t c = first; c < (size_t)a.C; c += stride) {
        const int32_t st = a.centre_status[c];
        if (st > 0) atomicMax(&a.status[c], st);
    }
    for (size_t e = first; e < total; e += stride) {
        const int c = a.rows[e / (size_t)a.P];
        const int32_t st = a.plus_status[e];
        if (st > 0) atomicMax(&a.status[c], st);
        const double fc = a.value[c];
        double q = 0.0;
        if (isfinite(fc)) {
            const double* row = a.plus + e * (size_t)a.P;
            bool valid = true;
            for (int k = 0; k < a.n; ++k) {
                double sum = 0.0;
                for (int j = 1; j <= 8; ++j) {  // E .. D
                    const int idx = a.mult_index[j - 1];
                    const double mult = idx >= 0 ? row[idx] : 1.0;
                    sum += a.init_state[j * a.lpc + k] * mult;
                }
                if (sum > a.N[k] || sum < 0) valid = false;
            }
            const double fp = a.f_plus[e];
            if (valid && isfinite(fp)) q = (fp - fc) / a.eps[e];
        }
        a.grad[e] = q;
    }
}

}  // namespace

int launch_fd_build(const double* d_theta, const int32_t* d_rows, int G, int P, double fd_epsilon, double* d_plus, double* d_eps,
                    void* stream) {
    if (G <= 0) return 0;
    hipLaunchKernelGGL(fd_build_kernel, dim3(fd_grid((size_t)G * P * P)), dim3(FD_BLOCK), 0, static_cast<hipStream_t>(stream), d_theta,
                       d_rows, G, P, fd_epsilon, d_plus, d_eps);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_fd_quotient(const FdQuotientArgs& a, void* stream) {
    const size_t work = (size_t)a.G * a.P > (size_t)a.C ? (size_t)a.G * a.P : (size_t)a.C;
    hipLaunchKernelGGL(fd_quotient_kernel, dim3(fd_grid(work)), dim3(FD_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd
