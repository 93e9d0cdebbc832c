// csrc/sepaihrd_predictive.hip -- what every posterior predictive call on gfx950 runs around its draw kernel
// (sepaihrd_ensemble_predictive and its dispersed and scored forms): the counts of valid samples and the
// mid-PIT counts, with the argument rules and the probe of the Poisson sampler.  That sampler is csrc/sepaihrd_poisson.inc, the
// text the host twin compiles too; the draw kernel is csrc/sepaihrd_predictive_nb.hip's (the Poisson draw is its k = +inf), the
// segment sorts and the quantiles are csrc/sepaihrd_ensemble.hip's.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cstdio>
#include <string>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_poisson.inc"
#include "sepaihrd_predictive_device.h"

namespace sepaihrd {
namespace {

constexpr int DRAW_BLOCK = 256;

// counts[0] = valid samples, counts[1] = valid samples x R
__global__ __launch_bounds__(256) void predictive_count_kernel(const int32_t* wstatus, int S, int R, int32_t* counts) {
    __shared__ int part[256];
    int c = 0;
    for (int s = threadIdx.x; s < S; s += 256) c += (wstatus[s] == 0);
    part[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) { counts[0] = part[0]; counts[1] = part[0] * R; }
}

// One workgroup per cell of the three daily series: the draws below and at the observation, counted before the sort (the
// padding is +inf and counts as neither).  Usable observation: finite and >= 0, the likelihood's rule; elsewhere NaN.
__global__ __launch_bounds__(256) void predictive_pit_kernel(const PredictiveArgs a) {
    __shared__ int less_part[256], equal_part[256];
    const size_t cell = blockIdx.x;  // (series Tp + t) n + age
    const int age = (int)(cell % a.n);
    const int t = (int)((cell / a.n) % a.Tp);
    const int ser = (int)(cell / ((size_t)a.n * a.Tp));
    const double obs = a.grid[((size_t)(a.runup_offset + t) * a.lpc + age) * 4 + ser];
    if (!(obs >= 0.0 && obs <= 0x1.fffffffffffffp+1023)) {
        if (threadIdx.x == 0) a.pit_out[cell] = NAN;
        return;
    }
    const double* seg = a.vals + cell * (size_t)a.N_pad;
    const size_t N = (size_t)a.S * a.R;
    int less = 0, equal = 0;
    for (size_t i = threadIdx.x; i < N; i += 256) {
        const double y = seg[i];
        less += (y < obs);
        equal += (y == obs);
    }
    less_part[threadIdx.x] = less;
    equal_part[threadIdx.x] = equal;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            less_part[threadIdx.x] += less_part[threadIdx.x + w];
            equal_part[threadIdx.x] += equal_part[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.pit_out[cell] = sepaihrd_poisson::mid_pit(less_part[0], equal_part[0], a.counts[1]);
}

__global__ __launch_bounds__(DRAW_BLOCK) void poisson_probe_kernel(uint64_t seed, const double* lambda, int count, double* out) {
    const int i = (int)(blockIdx.x * (unsigned)DRAW_BLOCK + threadIdx.x);
    if (i >= count) return;
    out[i] = sepaihrd_poisson::poisson(seed, (uint32_t)i, 0u, 0u, lambda[i]);
}

}  // namespace

int launch_predictive_counts(const PredictiveArgs& a, void* stream) {
    hipLaunchKernelGGL(predictive_count_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a.wstatus, a.S, a.R, a.counts);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
int launch_predictive_pit(const PredictiveArgs& a, void* stream) {
    if (a.pit_out != nullptr)
        hipLaunchKernelGGL(predictive_pit_kernel, dim3((unsigned)((size_t)3 * a.Tp * a.n)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd

using namespace sepaihrd;

extern "C" int sepaihrd_predictive_validate(int S, int R, int T_pos, int n_age, const double* probs, int n_probs, char* err, int errlen) {
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, "ensemble_predictive: " + msg); return SEPAIHRD_E_INVALID_ARG; };
    if (S < 1) return refuse("S must be >= 1 (samples)");
    if (R < 1) return refuse("R must be >= 1 (replicates per sample)");
    if ((uint64_t)S * (uint64_t)R >= ((uint64_t)1 << 31)) return refuse("S x R must stay below 2^31 (draws per segment)");
    if (T_pos < 1 || n_age < 1) return refuse("T_pos and n_age must be >= 1");
    if ((uint64_t)3 * (uint64_t)T_pos * (uint64_t)n_age >= ((uint64_t)1 << 32))
        return refuse("3 x T_pos x n_age must stay below 2^32 (the third stream coordinate)");
    if (!probs || n_probs < 1 || n_probs > 1024) return refuse("need probs (1..1024)");
    for (int p = 0; p < n_probs; ++p)
        if (!(probs[p] >= 0.0 && probs[p] <= 1.0)) return refuse("probabilities must lie in [0, 1]");
    return SEPAIHRD_OK;
}

extern "C" int sepaihrd_poisson_device(int device, uint64_t seed, const double* lambda, int count, double* out, char* err, int errlen) {
    if (!lambda || !out || count < 1) { set_err(err, errlen, "poisson_device: need lambda, out and count >= 1"); return SEPAIHRD_E_INVALID_ARG; }
    if (const int drc = select_device(device, err, errlen)) return drc;
    Probe pr;
    const double* d_lambda = pr.in(lambda, (size_t)count);
    double* d_out = pr.out<double>((size_t)count);
    if (pr.ready()) {
        hipLaunchKernelGGL(poisson_probe_kernel, dim3((unsigned)((count + DRAW_BLOCK - 1) / DRAW_BLOCK)), dim3(DRAW_BLOCK), 0, nullptr, seed,
                           d_lambda, count, d_out);
        pr.fetch(out, d_out, (size_t)count);
    }
    return pr.status("poisson_device", err, errlen);
}
