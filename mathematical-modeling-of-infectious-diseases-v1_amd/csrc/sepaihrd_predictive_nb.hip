// csrc/sepaihrd_predictive_nb.hip -- the daily posterior predictive draws on gfx950, under the negative-binomial observation
// model (sepaihrd_ensemble_predictive_nb) and, with no dispersion table, under the Poisson one
// (sepaihrd_ensemble_predictive; section 6i): the per-sample dispersions, the draw kernel over the integrator's parked increments
// and the probes of the gamma and negative-binomial samplers.  The draw is csrc/sepaihrd_predictive_draw.inc, the sampler
// csrc/sepaihrd_nb_draw.inc, the text the host twin compiles too; the counts and the mid-PIT are csrc/sepaihrd_predictive.hip's,
// the segment sorts and the quantiles csrc/sepaihrd_ensemble.hip's.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_nb_objective_device.h"
#include "sepaihrd_predictive_device.h"
#include "sepaihrd_predictive_draw.inc"

namespace sepaihrd {
namespace {

#include "sepaihrd_constrain.inc"  // constrained_theta: a calibrated dispersion under the text the likelihood pass compiles

// One lane per (sample, series): k as sepaihrd_nb_ll_rows_kernel resolves it, the constrained theta entry of a calibrated series
// and the context's fixed value otherwise (`fixed` alone where the call brought its own three values: src = -1).  A sample whose
// k is NaN (a NaN theta entry) has no draw: it becomes a failed sample (status 1), as its likelihood is a failed evaluation.
__global__ __launch_bounds__(DRAW_BLOCK) void predictive_nb_k_kernel(const DevProblem pb, const double* __restrict__ theta, const int S,
                                                                     const NbDispersion disp, double* __restrict__ k_used, int32_t* wstatus) {
    const int s = (int)(blockIdx.x * (unsigned)DRAW_BLOCK + threadIdx.x);
    if (s >= S) return;
    const double* th = theta + (size_t)s * pb.P;
    bool nan_k = false;
    for (int ser = 0; ser < 3; ++ser) {
        const double k = disp.src[ser] >= 0 ? constrained_theta(pb, th, disp.src[ser]) : disp.fixed[ser];
        k_used[(size_t)s * 3 + ser] = k;
        nan_k = nan_k || k != k;
    }
    if (nan_k && wstatus[s] == 0) wstatus[s] = 1;
}

// The daily table: the lanes and the draw of csrc/sepaihrd_predictive_draw.inc with the age on the grid's y dimension.  The lane
// stores y into the row of its (series, time, age) and the running sum of y (exact integers in double) into the row of series
// 3 .. 5; failed and padding slots hold +inf in both and sort last.
__global__ __launch_bounds__(DRAW_BLOCK) void predictive_draw_kernel(const PredictiveArgs a, const double* __restrict__ k_used) {
    DrawLane l;
    if (!draw_lane(a, k_used, (int)blockIdx.y, l)) return;
    const size_t seg_stride = (size_t)a.N_pad;
    double run = l.ok ? 0.0 : INFINITY;
    for (int t = 0; t < a.Tp; ++t) {
        const double y = draw_row(a, l, t, true);
        if (l.ok) run += y;
        const size_t cell = draw_cell(a, l, t);
        a.vals[cell * seg_stride + l.idx] = l.ok ? y : (double)INFINITY;
        a.vals[(cell + (size_t)3 * a.Tp * a.n) * seg_stride + l.idx] = run;
    }
}

__global__ __launch_bounds__(DRAW_BLOCK) void gamma_probe_kernel(uint64_t seed, const double* shape, int count, double* out) {
    const int i = (int)(blockIdx.x * (unsigned)DRAW_BLOCK + threadIdx.x);
    if (i >= count) return;
    out[i] = sepaihrd_nb_draw::gamma(seed, (uint32_t)i, 0u, 0u, shape[i]);
}

__global__ __launch_bounds__(DRAW_BLOCK) void nb_draw_probe_kernel(uint64_t seed, const double* mu, const double* k, int count, double* out) {
    const int i = (int)(blockIdx.x * (unsigned)DRAW_BLOCK + threadIdx.x);
    if (i >= count) return;
    out[i] = sepaihrd_nb_draw::nb_variate(seed, (uint32_t)i, 0u, 0u, mu[i], k[i]);
}

// the shapes and dispersions a probe may be asked for: what sepaihrd_particle_nb_validate accepts for one series, a finite
// value in [1e-3, 1e6] (and +inf for a dispersion)
bool probe_values_ok(const double* v, int count, bool allow_inf) {
    for (int i = 0; i < count; ++i) {
        const bool finite_ok = v[i] >= 1e-3 && v[i] <= 1e6;
        if (!finite_ok && !(allow_inf && v[i] > 0x1.fffffffffffffp+1023)) return false;
    }
    return true;
}

}  // namespace

int launch_predictive_nb_k(const PredictiveArgs& a, const DevProblem& pb, const double* d_theta, const NbDispersion& disp, double* d_k_used,
                           int32_t* d_wstatus, void* stream) {
    if (a.S <= 0 || d_theta == nullptr || d_k_used == nullptr || d_wstatus == nullptr || a.wstatus != d_wstatus) return -4;
    hipLaunchKernelGGL(predictive_nb_k_kernel, dim3((unsigned)((a.S + DRAW_BLOCK - 1) / DRAW_BLOCK)), dim3(DRAW_BLOCK), 0, static_cast<hipStream_t>(stream),
                       pb, d_theta, a.S, disp, d_k_used, d_wstatus);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_predictive_draws(const PredictiveArgs& a, const double* d_k_used, void* stream) {
    if (!draw_args_ok(a)) return -4;
    hipLaunchKernelGGL(predictive_draw_kernel, dim3((unsigned)((a.N_pad + DRAW_BLOCK - 1) / DRAW_BLOCK), (unsigned)a.n, 3u), dim3(DRAW_BLOCK), 0,
                       static_cast<hipStream_t>(stream), a, d_k_used);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd

using namespace sepaihrd;

extern "C" int sepaihrd_gamma_device(int device, uint64_t seed, const double* shape, int count, double* out, char* err, int errlen) {
    if (!shape || !out || count < 1) { set_err(err, errlen, "gamma_device: need shape, out and count >= 1"); return SEPAIHRD_E_INVALID_ARG; }
    if (!probe_values_ok(shape, count, false)) { set_err(err, errlen, "gamma_device: every shape must be finite in [1e-3, 1e6]"); return SEPAIHRD_E_INVALID_ARG; }
    if (const int drc = select_device(device, err, errlen)) return drc;
    Probe pr;
    const double* d_shape = pr.in(shape, (size_t)count);
    double* d_out = pr.out<double>((size_t)count);
    if (pr.ready()) {
        hipLaunchKernelGGL(gamma_probe_kernel, dim3((unsigned)((count + DRAW_BLOCK - 1) / DRAW_BLOCK)), dim3(DRAW_BLOCK), 0, nullptr, seed, d_shape,
                           count, d_out);
        pr.fetch(out, d_out, (size_t)count);
    }
    return pr.status("gamma_device", err, errlen);
}

extern "C" int sepaihrd_nb_draw_device(int device, uint64_t seed, const double* mu, const double* k, int count, double* out, char* err, int errlen) {
    if (!mu || !k || !out || count < 1) { set_err(err, errlen, "nb_draw_device: need mu, k, out and count >= 1"); return SEPAIHRD_E_INVALID_ARG; }
    if (!probe_values_ok(k, count, true)) {
        set_err(err, errlen, "nb_draw_device: every k must be +inf or finite in [1e-3, 1e6]");
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (const int drc = select_device(device, err, errlen)) return drc;
    Probe pr;
    const double* d_mu = pr.in(mu, (size_t)count);
    const double* d_k = pr.in(k, (size_t)count);
    double* d_out = pr.out<double>((size_t)count);
    if (pr.ready()) {
        hipLaunchKernelGGL(nb_draw_probe_kernel, dim3((unsigned)((count + DRAW_BLOCK - 1) / DRAW_BLOCK)), dim3(DRAW_BLOCK), 0, nullptr, seed, d_mu, d_k,
                           count, d_out);
        pr.fetch(out, d_out, (size_t)count);
    }
    return pr.status("nb_draw_device", err, errlen);
}
