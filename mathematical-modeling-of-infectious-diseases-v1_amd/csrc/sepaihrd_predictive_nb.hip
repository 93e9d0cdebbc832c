// csrc/sepaihrd_predictive_nb.hip -- posterior predictive draws under the negative-binomial observation model on gfx950
// (sepaihrd_ensemble_predictive_nb): the per-sample dispersions, the draw kernel over the integrator's
// parked increments and the probes of the gamma and negative-binomial samplers.  The sampler is csrc/sepaihrd_nb_draw.inc, the
// text the host twin compiles too; the counts and the mid-PIT are csrc/sepaihrd_predictive.hip's, the segment sorts and the
// quantiles csrc/sepaihrd_ensemble.hip's.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_nb_draw.inc"
#include "sepaihrd_nb_objective_device.h"
#include "sepaihrd_predictive_device.h"
#include "sepaihrd_predictive_targets_device.h"

namespace sepaihrd {
namespace {

#include "sepaihrd_constrain.inc"  // constrained_theta: a calibrated dispersion under the text the likelihood pass compiles

constexpr int DRAW_BLOCK = 256;

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

// One lane per (sample s, replicate r, age, series): consecutive lanes along s R + r as in predictive_draw_kernel, the age on the
// grid's y dimension and the series on its z dimension -- 3 n_age times that kernel's wavefronts, each lane walking only the
// T_pos output times of its own running sum.  The loads of a sample's increments are broadcasts, the stores into a segment
// contiguous.  m = max(0, increment), y ~ NegativeBinomial(m + 1e-10, k_used[s][series]) at the stream coordinates of
// predictive_draw_kernel, (s, r, (series Tp + time) n + age); k = +inf is that kernel's Poisson draw, bit for bit.
__global__ __launch_bounds__(DRAW_BLOCK) void predictive_nb_draw_kernel(const PredictiveArgs a, const double* __restrict__ k_used) {
    const size_t idx = (size_t)blockIdx.x * DRAW_BLOCK + threadIdx.x;
    if (idx >= (size_t)a.N_pad) return;
    const int age = (int)blockIdx.y, ser = (int)blockIdx.z;
    const size_t s = idx / (size_t)a.R;
    const uint32_t r = (uint32_t)(idx % (size_t)a.R);
    const bool in_range = s < (size_t)a.S;
    const bool ok = in_range && a.wstatus[s] == 0;
    const size_t seg_stride = (size_t)a.N_pad;
    const int comp = (ser == 0) ? 1 : (ser == 1) ? 2 : 0;  // cum rows are D, CumH, CumICU; series are H, ICU, D
    const double k = ok ? k_used[s * 3 + (size_t)ser] : INFINITY;
    const size_t col = s * (size_t)a.lpc + (size_t)age;
    double run = 0.0;
    for (int t = 0; t < a.Tp; ++t) {
        const size_t cell = ((size_t)ser * a.Tp + t) * a.n + age;
        double m = NAN, y = INFINITY, cumulative = INFINITY;
        if (ok) {
            const double inc = a.cum[cum_index(a.T, col, a.runup_offset + t, comp)];
            m = (0.0 < inc) ? inc : 0.0;
            y = sepaihrd_nb_draw::nb_variate(a.seed, (uint32_t)s, r, (uint32_t)cell, m + 1e-10, k);
            run += y;
            cumulative = run;
        }
        a.vals[cell * seg_stride + idx] = y;
        a.vals[(cell + (size_t)3 * a.Tp * a.n) * seg_stride + idx] = cumulative;
        if (in_range) {
            if (a.means != nullptr && r == 0) a.means[((s * 3 + ser) * a.Tp + t) * a.n + age] = m;
            if (a.draws != nullptr) a.draws[((idx * 3 + ser) * a.Tp + t) * a.n + age] = ok ? y : (double)NAN;
        }
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

int launch_predictive_draws_nb(const PredictiveArgs& a, const DevProblem& pb, const double* d_theta, const NbDispersion& disp, double* d_k_used,
                               int32_t* d_wstatus, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the grid's y and z dimensions hold at most 65 535 blocks
    if (a.S <= 0 || a.R <= 0 || a.n <= 0 || a.n > 65535 || a.Tp <= 0 || (size_t)a.S * a.R > (size_t)a.N_pad || a.N_pad % WAVE != 0 ||
        (uint64_t)3 * a.Tp * a.n >= ((uint64_t)1 << 32) || d_theta == nullptr || d_k_used == nullptr || d_wstatus == nullptr || a.wstatus != d_wstatus)
        return -4;
    hipLaunchKernelGGL(predictive_nb_k_kernel, dim3((unsigned)((a.S + DRAW_BLOCK - 1) / DRAW_BLOCK)), dim3(DRAW_BLOCK), 0, st, pb, d_theta, a.S, disp,
                       d_k_used, d_wstatus);
    if (launch_predictive_counts(a, stream) != 0) return -3;
    hipLaunchKernelGGL(predictive_nb_draw_kernel, dim3((unsigned)((a.N_pad + DRAW_BLOCK - 1) / DRAW_BLOCK), (unsigned)a.n, 3u), dim3(DRAW_BLOCK), 0,
                       st, a, d_k_used);
    if (hipGetLastError() != hipSuccess) return -3;
    return launch_predictive_pit(a, stream);
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
