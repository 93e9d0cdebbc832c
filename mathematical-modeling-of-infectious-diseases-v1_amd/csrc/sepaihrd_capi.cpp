// csrc/sepaihrd_capi.cpp -- implementation of the C ABI declared in include/sepaihrd_hip.h.
// Host side only: validates the problem, resolves the theta -> field map into slot tables,
// uploads the problem to HBM once, and launches the HIP kernels.  There is no CPU
// evaluation path in this library.
#include "sepaihrd_hip.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sepaihrd_device.h"
#include "sepaihrd_fd_device.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_mh_backend.h"
#include "sepaihrd_nb_objective_device.h"
#include "sepaihrd_predictive_device.h"
#include "sepaihrd_predictive_targets.inc"
#include "sepaihrd_predictive_targets_device.h"
#include "sepaihrd_segments.h"
#include "sepaihrd_particle_device.h"
#include "sepaihrd_particle_nb_host.h"
#include "sepaihrd_particle_states_device.h"
#include "sepaihrd_particle_wide_device.h"
#include "sepaihrd_stoch_sepaihrd_device.h"

using namespace sepaihrd;

// The roles of the buffers the ensemble entry points keep with their context.  sepaihrd_ensemble_quantiles uses the first
// nine; sepaihrd_scenario_ensemble uses the same nine for the same things, sized for K scenarios, and four of its own.
enum EnsSlot {
    SLOT_THETA, SLOT_LOGLIK, SLOT_VALS, SLOT_TRAJ, SLOT_PROBS, SLOT_QUANTILES, SLOT_N_VALID, SLOT_METRICS, SLOT_SORT_SCRATCH,
    SLOT_KAPPA_MULT, SLOT_SCEN_VALS, SLOT_SCEN_SUMMARY, SLOT_SCEN_COUNTS, SLOT_COUNT
};

struct sepaihrd_ctx {
    int device = 0;
    int solver = 0;
    int arith = 0;
    int precision = 0;  // SEPAIHRD_PRECISION_F64 / _F32
    DevProblem dp{};
    // the negative-binomial observation model (sepaihrd_set_dispersion): per series the theta entry that
    // calibrates its dispersion, or the fixed value; all +inf: the Poisson objective, untouched
    NbDispersion disp{{-1, -1, -1}, 0, {std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()}};
    // Everything below that owns a HIP resource releases it in its destructor; members go in reverse order of declaration, so
    // own_stream, declared last, is drained and destroyed before any buffer it may touch is freed (sepaihrd_destroy).
    DeviceAllocs allocs;  // the problem's tables
    // host copies needed by sepaihrd_apply_constraints
    std::vector<double> lower, upper;
    std::vector<uint8_t> has_bounds;
    int n = 0, T = 0, P = 0;
    std::vector<double> host_N;  // population sizes (ensemble seroprevalence)
    // buffers of sepaihrd_ensemble_quantiles and sepaihrd_scenario_ensemble, kept between calls
    GrowSlots<SLOT_COUNT> ens;
    std::string last_error;
    // staging buffers for the host-pointer entry point (grown on demand), and the views ensure_staging lays into them
    DeviceBuf theta_buf, results_buf, traj_buf;
    PinnedBuf results_host;
    int pending_B = 0;
    double* d_theta = nullptr;
    double* d_loglik = nullptr;
    int32_t* d_status = nullptr;
    int32_t* d_nacc = nullptr;
    int32_t* d_nrej = nullptr;
    double* d_parts = nullptr;
    // d_loglik .. d_parts are views into ONE allocation (results slab: [loglik B][parts 3B][status B][accepted B][rejected B]),
    // fetched with one copy into a page-locked mirror of the same layout
    double* d_traj = nullptr;
    // likelihood-pass workspace (device), sized for ws_chains chains: three buffers, one capacity
    DeviceBuf ws_buf[3];
    size_t ws_chains = 0;
    double* ws_cum = nullptr;
    double* ws_rows = nullptr;
    int32_t* ws_status = nullptr;
    size_t ws_budget_bytes = (size_t)24 << 30;  // larger batches are evaluated in chunks of chains
    // ONE evaluation in flight per context (they share the workspace above): the last launch sequence leaves an
    // event, and a launch on a different stream waits for it first (free when the stream is the same)
    Event busy_event;
    hipStream_t busy_stream = nullptr;
    bool busy_valid = false;
    // a stream the LIBRARY owns (a sampler's) on which launches after the first record nothing: every marker between two
    // kernels of a stream is dispatch latency (3-5 us each in the sampler loop).  The event is re-recorded lazily when
    // another stream asks (fence_before); only for an owned stream, whose handle is known to be alive
    hipStream_t lazy_stream = nullptr;
    // sepaihrd_device_libm_check: -1 not run yet, else the number of self-check arguments on which the device's log / exp
    // restatements differ from this process's libm
    int libm_log_diff = -1, libm_exp_diff = -1;
    // optional per-kernel timing (HIP events on the launch stream), see sepaihrd_set_timing
    bool timing = false;
    int timing_period = 1;     // events around every timing_period-th launch sequence only
    long timing_seen = 0;
    std::vector<Event> ev;  // triples: before integrator, after integrator, after likelihood pass
    size_t ev_used = 0;
    // per-chain summary records: the table of the chains this context ran, and the gathered table of all
    DeviceBuf rec_buf[2];
    // sepaihrd_fd_gradient_batch (held by the context of the perturbed evaluations, grow-only): the perturbed matrix, steps
    // and perturbed values, then the staging of the call's inputs and results with a page-locked mirror of the results
    DeviceBuf fd_dev;
    PinnedBuf fd_host;
    Event fd_ev_uploaded, fd_ev_centre;
    // the last sepaihrd_ensemble_predictive call (or _nb, or _scores): integrator, draws and mid-PIT counts, sorts and quantiles --
    // with the scores in the scored call, which has no PIT pass (ms)
    double pred_ms[3] = {0.0, 0.0, 0.0};
    // the last sepaihrd_ensemble_stochastic call: step kernel, sorts and quantiles (ms)
    double stoch_ms[2] = {0.0, 0.0};
    // the last sepaihrd_particle_loglik call: decode, filter kernel (ms)
    double particle_ms[2] = {0.0, 0.0};
    // the last sepaihrd_particle_loglik_wide call: decode, all filter launches (ms); and the host's copy of dp.grid, from which
    // that call plans its launches (which output rows have a usable observation)
    double particle_wide_ms[2] = {0.0, 0.0};
    std::vector<double> host_grid;
    // the last sepaihrd_particle_filter_states call: decode, all launches, of these the summaries of the first chunk (ms)
    double particle_states_ms[3] = {0.0, 0.0, 0.0};
    Stream own_stream;  // sepaihrd_eval_batch_begin / _end; last: see above
};

namespace {

#include "sepaihrd_constrain.inc"  // constrain: the text the kernels compile

// chains per launch so that the cumulative-compartment workspace stays within the budget
size_t chunk_chains(const sepaihrd_ctx* c, size_t B) {
    const size_t cpw = (size_t)(WAVE / c->dp.lpc);
    const size_t per_chain = (size_t)c->dp.T * 3 * c->dp.lpc * sizeof(double);
    size_t fit = std::max<size_t>(cpw, (c->ws_budget_bytes / per_chain) / cpw * cpw);
    const size_t want = (B + cpw - 1) / cpw * cpw;
    return std::min(fit, want);
}

int ensure_workspace(sepaihrd_ctx* c, size_t chains) {
    if (chains <= c->ws_chains) return SEPAIHRD_OK;
    c->ws_chains = 0;
    for (DeviceBuf& b : c->ws_buf) b.release();  // all three before the first grows: the workspace may be most of the device
    if (!c->ws_buf[0].get(&c->ws_cum, workspace_cum_doubles(c->dp, chains)) ||
        !c->ws_buf[1].get(&c->ws_rows, workspace_rows_doubles(c->dp, chains)) || !c->ws_buf[2].get(&c->ws_status, chains)) {
        for (DeviceBuf& b : c->ws_buf) b.release();
        c->ws_cum = c->ws_rows = nullptr;
        c->ws_status = nullptr;
        c->last_error = "likelihood workspace allocation failed";
        return SEPAIHRD_E_HIP;
    }
    c->ws_chains = chains;
    return SEPAIHRD_OK;
}

// Does a launch of B chains use the ctx-owned workspace?  Decided by the kernel translation unit (the launch code
// takes the same branches); < 0: unsupported lanes-per-chain.
int needs_workspace(const sepaihrd_ctx* c, int B, int force_split) {
    if (c->precision == SEPAIHRD_PRECISION_F32 && !force_split) return c->dp.lpc >= 4 ? 0 : -4;  // likelihood inline
    return c->arith == SEPAIHRD_ARITH_FMA ? launch_needs_workspace_fma(c->dp, c->solver, B, force_split)
                                          : launch_needs_workspace_strict(c->dp, c->solver, B, force_split);
}

bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// Order this launch sequence after the previous one of the same context when it runs on another stream.
// Inside a stream capture nothing is recorded or waited for (the captured graph owns its ordering).
int fence_before(sepaihrd_ctx* c, hipStream_t st) {
    if (!c->busy_valid || c->busy_stream == st || stream_is_capturing(st)) return SEPAIHRD_OK;
    // launches after the first on a sampler's stream recorded nothing: mark the end of what is queued there now, for
    // this other stream to wait on
    if (c->lazy_stream != nullptr && c->busy_stream == c->lazy_stream) (void)hipEventRecord(c->busy_event, c->busy_stream);
    if (hipStreamWaitEvent(st, c->busy_event, 0) != hipSuccess) {
        c->last_error = "hipStreamWaitEvent on the context's previous evaluation failed";
        return SEPAIHRD_E_HIP;
    }
    return SEPAIHRD_OK;
}
void fence_after(sepaihrd_ctx* c, hipStream_t st) {
    if (c->busy_valid && c->busy_stream == st && st == c->lazy_stream) return;  // recorded lazily (fence_before)
    if (stream_is_capturing(st)) return;
    if (!c->busy_event && c->busy_event.create(hipEventDisableTiming) != hipSuccess) return;
    if (hipEventRecord(c->busy_event, st) == hipSuccess) { c->busy_stream = st; c->busy_valid = true; }
}

constexpr size_t RESULT_BYTES_PER_CHAIN = 4 * sizeof(double) + 3 * sizeof(int32_t);

// Staging of the host-pointer entry points for B chains (the trajectory buffer is sepaihrd_eval_batch's and stays).  The result
// views are laid out for THIS batch at the front of the slab, so that one copy fetches them whatever the capacity.
int ensure_staging(sepaihrd_ctx* ctx, size_t B) {
    ALLOC_TRY(ctx->theta_buf.get(&ctx->d_theta, B * ctx->P), ctx, return SEPAIHRD_E_HIP);
    ALLOC_TRY(ctx->results_buf.reserve(B * RESULT_BYTES_PER_CHAIN), ctx, return SEPAIHRD_E_HIP);
    ALLOC_TRY(ctx->results_host.reserve(B * RESULT_BYTES_PER_CHAIN), ctx, return SEPAIHRD_E_HIP);
    ctx->d_loglik = ctx->results_buf.as<double>();
    ctx->d_parts = ctx->d_loglik + B;
    ctx->d_status = reinterpret_cast<int32_t*>(ctx->d_parts + 3 * B);
    ctx->d_nacc = ctx->d_status + B;
    ctx->d_nrej = ctx->d_nacc + B;
    return SEPAIHRD_OK;
}

// One copy of the batch's results (the span up to the last array asked for) and the wait; then the caller's arrays are
// filled from the page-locked mirror.
int fetch_results(sepaihrd_ctx* ctx, hipStream_t st, int B, double* loglik, int32_t* status, int32_t* n_accept, int32_t* n_reject,
                  double* ll_parts) {
    const size_t n = (size_t)B;
    char* const h = ctx->results_host.as<char>();
    const size_t off_parts = n * sizeof(double), off_status = 4 * n * sizeof(double);
    const size_t off_nacc = off_status + n * sizeof(int32_t), off_nrej = off_nacc + n * sizeof(int32_t);
    size_t hi = n * sizeof(double);  // the log-likelihoods, always
    if (ll_parts) hi = off_status;
    if (status) hi = off_nacc;
    if (n_accept) hi = off_nrej;
    if (n_reject) hi = off_nrej + n * sizeof(int32_t);
    HIP_TRY(hipMemcpyAsync(h, ctx->results_buf.p, hi, hipMemcpyDeviceToHost, st), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipStreamSynchronize(st), ctx, return SEPAIHRD_E_HIP);
    if (loglik) std::memcpy(loglik, h, n * sizeof(double));
    if (ll_parts) std::memcpy(ll_parts, h + off_parts, n * 3 * sizeof(double));
    if (status) std::memcpy(status, h + off_status, n * sizeof(int32_t));
    if (n_accept) std::memcpy(n_accept, h + off_nacc, n * sizeof(int32_t));
    if (n_reject) std::memcpy(n_reject, h + off_nrej, n * sizeof(int32_t));
    return SEPAIHRD_OK;
}

int refuse(sepaihrd_ctx* ctx, const char* who, const std::string& msg, int rc) {
    ctx->last_error = std::string(who) + ": " + msg;
    return rc;
}

// a validator's verdict (vrc, with its text in msg) as the call's: a refusal becomes the context's last error
int validated(sepaihrd_ctx* ctx, int vrc, const char* msg) {
    if (vrc == SEPAIHRD_OK) return SEPAIHRD_OK;
    ctx->last_error = msg;
    return SEPAIHRD_E_INVALID_ARG;
}

// ms[i]: the time from ev[i] to ev[i + 1] of a call that has been synchronised
void elapsed_ms(const std::vector<Event>& ev, double* ms, int n) {
    for (int i = 0; i < n; ++i) {
        float t = 0.0f;
        (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
        ms[i] = t;
    }
}

// The opening checks the ensemble entry points share.  Always: the arguments every call needs (have_args, with the text
// `need` that names them) and n_probs in 1..1024.  Then those of `checks`, in this order; an entry point that has checks of
// its own in between asks in several steps (need == nullptr: the arguments were checked before).
enum : unsigned { CHECK_PROBS = 1, CHECK_PENDING = 2, CHECK_F64 = 4, CHECK_TP = 8 };
int ensemble_preflight(sepaihrd_ctx* ctx, const char* who, bool have_args, const char* need, unsigned checks, const double* probs = nullptr,
                       int n_probs = 0) {
    if (need != nullptr && (!have_args || n_probs <= 0 || n_probs > 1024)) return refuse(ctx, who, need, SEPAIHRD_E_INVALID_ARG);
    if ((checks & CHECK_PROBS) && !probabilities_valid(probs, n_probs))
        return refuse(ctx, who, "probabilities must lie in [0, 1]", SEPAIHRD_E_INVALID_ARG);
    if ((checks & CHECK_PENDING) && ctx->pending_B > 0)
        return refuse(ctx, who, "a sepaihrd_eval_batch_begin is pending on this context", SEPAIHRD_E_INVALID_ARG);
    if ((checks & CHECK_F64) && ctx->precision != SEPAIHRD_PRECISION_F64)
        return refuse(ctx, who, "the ensemble summaries read the fp64 integrator's parked increments (set precision F64)", SEPAIHRD_E_UNSUPPORTED);
    if ((checks & CHECK_TP) && ctx->dp.T - ctx->dp.runup_offset <= 0) return refuse(ctx, who, "no output time >= 0", SEPAIHRD_E_INVALID_ARG);
    return SEPAIHRD_OK;
}

// The integrator on B chains in the context's arithmetic, on the null stream; d_kappa_mult: the scenario build's launch, chain
// c with row c / stride of the table.  A failure becomes the context's last error (after `prefix`) and the C ABI's code.
int launch_eval_for(sepaihrd_ctx* ctx, const char* prefix, const double* d_theta, int B, const EvalOutputs& out,
                    const double* d_kappa_mult = nullptr, int stride = 0) {
    const bool fma = ctx->arith == SEPAIHRD_ARITH_FMA;
    int rc;
    if (d_kappa_mult != nullptr)
        rc = fma ? launch_eval_scenario_fma(ctx->dp, ctx->solver, d_theta, B, out, nullptr, d_kappa_mult, stride)
                 : launch_eval_scenario_strict(ctx->dp, ctx->solver, d_theta, B, out, nullptr, d_kappa_mult, stride);
    else
        rc = fma ? launch_eval_fma(ctx->dp, ctx->solver, d_theta, B, out, nullptr) : launch_eval_strict(ctx->dp, ctx->solver, d_theta, B, out, nullptr);
    if (rc == 0) return SEPAIHRD_OK;
    ctx->last_error = std::string(prefix) + (rc == -4 ? "unsupported lanes-per-chain" : "kernel launch failed");
    return rc == -4 ? SEPAIHRD_E_UNSUPPORTED : SEPAIHRD_E_HIP;
}

double total_population(const sepaihrd_ctx* ctx) {
    double total_pop = 0.0;
    for (int i = 0; i < ctx->dp.n; ++i) total_pop += ctx->host_N[(size_t)i];
    return total_pop;
}


// the six RCCL entry points the gather needs, resolved once
struct RcclApi {
    void* lib = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
const RcclApi& rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) return a;
        a.CommInitAll = reinterpret_cast<decltype(a.CommInitAll)>(dlsym(a.lib, "ncclCommInitAll"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
        a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(dlsym(a.lib, "ncclGroupStart"));
        a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(dlsym(a.lib, "ncclGroupEnd"));
        a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(a.lib, "ncclAllGather"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
        a.ok = a.CommInitAll && a.CommDestroy && a.GroupStart && a.GroupEnd && a.AllGather;
        return a;
    }();
    return api;
}
constexpr int NCCL_DOUBLE = 8;  // ncclFloat64 (rccl.h: ncclDataType_t)

}  // namespace

// ---- what a sampler asks of its context (csrc/sepaihrd_mh_backend.h)
MhBackend sepaihrd::mh_backend_of(sepaihrd_ctx* ctx) {
    return MhBackend{ctx->device, ctx->P, ctx->last_error, ctx->dp, ctx->libm_log_diff, ctx->libm_exp_diff, ctx->pending_B, ctx, nullptr};
}
void sepaihrd::ctx_adopt_lazy_stream(sepaihrd_ctx* ctx, void* stream) { ctx->lazy_stream = static_cast<hipStream_t>(stream); }
void sepaihrd::ctx_forget_stream(sepaihrd_ctx* ctx, void* stream) {
    if (ctx->lazy_stream == stream) ctx->lazy_stream = nullptr;
    if (ctx->busy_stream == stream) { ctx->busy_valid = false; ctx->busy_stream = nullptr; }
}

extern "C" {

int sepaihrd_abi_version(void) { return SEPAIHRD_ABI_VERSION; }

sepaihrd_ctx* sepaihrd_create(const sepaihrd_problem* pb, int device, char* err, int errlen) {
    if (!pb) { set_err(err, errlen, "problem is NULL"); return nullptr; }
    if (pb->abi_version != SEPAIHRD_ABI_VERSION) { set_err(err, errlen, "ABI version mismatch"); return nullptr; }
    const int n = pb->n_age, T = pb->n_times, P = pb->n_params, nb = pb->n_beta, nk = pb->n_kappa;
    if (n < 1 || n > SEPAIHRD_MAX_AGE_CLASSES) { set_err(err, errlen, "n_age out of range [1,64]"); return nullptr; }
    if (lanes_per_chain(n) > 16) {
        set_err(err, errlen, "n_age > 16 not built in this version"); return nullptr;
    }
    if (T < 1) { set_err(err, errlen, "n_times must be >= 1"); return nullptr; }
    if (T > MAX_TIMES) { set_err(err, errlen, "n_times exceeds the LDS-staged grid limit (12288)"); return nullptr; }
    if (P < 1) { set_err(err, errlen, "n_params must be >= 1"); return nullptr; }
    if (nk < 1 || nk > SEPAIHRD_MAX_SCHEDULE || nb < 0 || nb > SEPAIHRD_MAX_SCHEDULE) {
        set_err(err, errlen, "schedule lengths out of range (n_kappa >= 1)"); return nullptr;
    }
    if (!pb->times || !pb->N || !pb->M || !pb->a || !pb->h_infec || !pb->p || !pb->h || !pb->icu ||
        !pb->d_H || !pb->d_ICU || !pb->kappa_end_times || !pb->kappa_values || !pb->initial_state ||
        !pb->param_field || !pb->param_index || (nb > 0 && (!pb->beta_end_times || !pb->beta_values)) ||
        (pb->n_obs > 0 && (!pb->obs_H || !pb->obs_ICU || !pb->obs_D))) {
        set_err(err, errlen, "a required array pointer is NULL"); return nullptr;
    }
    if (pb->solver != SEPAIHRD_SOLVER_DOPRI5 && pb->solver != SEPAIHRD_SOLVER_CASH_KARP54 &&
        pb->solver != SEPAIHRD_SOLVER_FEHLBERG78) {
        set_err(err, errlen, "unknown solver"); return nullptr;
    }
    // Simulator::run grid validation (Simulator.cpp:78-88) and ctor checks (:15-44)
    for (int i = 1; i < T; ++i)
        if (!(pb->times[i] > pb->times[i - 1])) {
            set_err(err, errlen, "time points must be strictly increasing"); return nullptr;
        }
    if (pb->abs_err < 0 || pb->rel_err < 0) { set_err(err, errlen, "negative error tolerance"); return nullptr; }
    if (!(pb->dt_hint > 0)) { set_err(err, errlen, "dt_hint must be positive"); return nullptr; }
    // schedule validation: PiecewiseConstantNpiStrategy ctor (PieceWiseConstantNPIStrategy.cpp:24-54),
    // PiecewiseConstantParameterStrategy ctor (PiecewiseConstantParameterStrategy.cpp:22-34)
    if (pb->kappa_end_times[0] < 0.0) { set_err(err, errlen, "kappa baseline end time must be non-negative"); return nullptr; }
    for (int k = 1; k < nk; ++k)
        if (!(pb->kappa_end_times[k] > pb->kappa_end_times[k - 1])) {
            set_err(err, errlen, "kappa end times must be strictly increasing"); return nullptr;
        }
    for (int k = 1; k < nb; ++k)
        if (!(pb->beta_end_times[k] > pb->beta_end_times[k - 1])) {
            set_err(err, errlen, "beta end times must be strictly increasing"); return nullptr;
        }

    // the SEPAIHRD_F_DISPERSION entries: index, bounds within [1e-3, 1e6], one entry per series
    int32_t disp_src[3] = {-1, -1, -1};
    if (sepaihrd_dispersion_validate(P, pb->param_field, pb->param_index, pb->lower, pb->upper, pb->has_bounds, disp_src, err, errlen) != SEPAIHRD_OK)
        return nullptr;

    if (select_device(device, err, errlen) != SEPAIHRD_OK) return nullptr;

    auto* ctx = new sepaihrd_ctx();
    for (int s = 0; s < 3; ++s) ctx->disp.src[s] = disp_src[s];
    ctx->device = device;
    ctx->solver = pb->solver;
    ctx->arith = pb->arith == SEPAIHRD_ARITH_FMA ? SEPAIHRD_ARITH_FMA : SEPAIHRD_ARITH_STRICT;
    if (pb->precision != SEPAIHRD_PRECISION_F64 && pb->precision != SEPAIHRD_PRECISION_F32) {
        set_err(err, errlen, "unknown precision"); delete ctx; return nullptr;
    }
    if (pb->precision == SEPAIHRD_PRECISION_F32 && lanes_per_chain(n) < 4) {
        set_err(err, errlen, "the fp32-state arm is built for 3 to 16 age classes"); delete ctx; return nullptr;
    }
    if (pb->precision == SEPAIHRD_PRECISION_F32 && pb->solver == SEPAIHRD_SOLVER_FEHLBERG78) {
        set_err(err, errlen, "the fp32-state arm is built for Dopri5 and Cash-Karp only"); delete ctx; return nullptr;
    }
    ctx->precision = pb->precision;
    ctx->n = n; ctx->T = T; ctx->P = P;
    ctx->host_N.assign(pb->N, pb->N + n);
    if (const char* mb = std::getenv("SEPAIHRD_WORKSPACE_MB")) {  // likelihood-workspace budget (default 24 GiB)
        const long v = std::atol(mb);
        if (v > 0) ctx->ws_budget_bytes = (size_t)v << 20;
    }

    const int lpc = lanes_per_chain(n);
    const int ns = SS_SCHEDULE0 + nb + nk;

    // ---- slot tables: later theta entries overwrite earlier ones, as the reference's
    //      sequential loop over names does (SEPAIHRDParameterManager.cpp:197-267)
    std::vector<int32_t> src_scalar(ns, -1);
    std::vector<double> base_scalar(ns, 0.0);
    base_scalar[SS_BETA] = pb->beta; base_scalar[SS_THETA] = pb->theta; base_scalar[SS_SIGMA] = pb->sigma;
    base_scalar[SS_GAMMA_P] = pb->gamma_p; base_scalar[SS_GAMMA_A] = pb->gamma_A;
    base_scalar[SS_GAMMA_I] = pb->gamma_I; base_scalar[SS_GAMMA_H] = pb->gamma_H;
    base_scalar[SS_GAMMA_ICU] = pb->gamma_ICU;
    for (int i = 0; i < 8; ++i) base_scalar[SS_E0_MULT + i] = pb->multipliers[i];
    base_scalar[SS_RUNUP_DAYS] = pb->runup_days; base_scalar[SS_SEED_EXPOSED] = pb->seed_exposed;
    for (int k = 0; k < nb; ++k) base_scalar[SS_SCHEDULE0 + k] = pb->beta_values[k];
    for (int k = 0; k < nk; ++k) base_scalar[SS_SCHEDULE0 + nb + k] = pb->kappa_values[k];

    std::vector<int32_t> src_vec((size_t)VF_COUNT * lpc, -1);
    std::vector<double> base_vec((size_t)VF_COUNT * lpc, 0.0);
    const double* vec_base_ptr[VF_COUNT] = {pb->a, pb->h_infec, pb->p, pb->h, pb->icu, pb->d_H, pb->d_ICU,
                                            pb->d_community};
    for (int f = 0; f < VF_COUNT; ++f)
        for (int i = 0; i < n; ++i) base_vec[(size_t)f * lpc + i] = vec_base_ptr[f] ? vec_base_ptr[f][i] : 0.0;

    int kappa_calibrated = 0;
    for (int p = 0; p < P; ++p) {
        const int f = pb->param_field[p], idx = pb->param_index[p];
        auto bad = [&](const char* what) {
            set_err(err, errlen, std::string("param ") + std::to_string(p) + ": " + what);
            delete ctx;
            return static_cast<sepaihrd_ctx*>(nullptr);
        };
        if (f == SEPAIHRD_F_NONE) continue;
        if (f >= SEPAIHRD_F_BETA && f <= SEPAIHRD_F_SEED_EXPOSED) {
            src_scalar[f] = p;
        } else if (f == SEPAIHRD_F_BETA_VALUE) {
            if (idx < 0 || idx >= nb) return bad("beta index out of range");
            src_scalar[SS_SCHEDULE0 + idx] = p;
        } else if (f == SEPAIHRD_F_KAPPA_VALUE) {
            if (idx < 1 || idx >= nk) return bad("kappa index out of range (index 0 is the fixed baseline)");
            src_scalar[SS_SCHEDULE0 + nb + idx] = p;
            kappa_calibrated = 1;
        } else if (f >= SEPAIHRD_F_A && f <= SEPAIHRD_F_D_COMMUNITY) {
            if (idx < 0 || idx >= n) return bad("age index out of range");
            src_vec[(size_t)(f - SEPAIHRD_F_A) * lpc + idx] = p;
        } else if (f == SEPAIHRD_F_DISPERSION) {
            // no model slot: the likelihood pass reads the entry (ctx->disp.src, validated above)
        } else {
            return bad("unknown field code");
        }
    }

    // ---- padded per-age tables
    std::vector<double> Npad(lpc, 0.0), fracpad(lpc, 0.0), Mrow((size_t)lpc * lpc, 0.0),
        init((size_t)NUM_COMP * lpc, 0.0);
    double total_pop = 0.0;
    for (int i = 0; i < n; ++i) { Npad[i] = pb->N[i]; total_pop += pb->N[i]; }
    if (total_pop > 0.0)  // SEPAIHRDObjectiveFunction.cpp:103-108
        for (int i = 0; i < n; ++i) fracpad[i] = pb->N[i] / total_pop;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Mrow[(size_t)i * lpc + j] = pb->M[(size_t)j * n + i];
    for (int c = 0; c < NUM_COMP; ++c)
        for (int i = 0; i < n; ++i) init[(size_t)c * lpc + i] = pb->initial_state[(size_t)c * n + i];

    int runup_offset = 0;  // SEPAIHRDObjectiveFunction.cpp:39-46
    for (int i = 0; i < T; ++i)
        if (pb->times[i] >= 0.0) { runup_offset = i; break; }
    const int num_obs_points = T - runup_offset;
    const int n_obs = pb->n_obs;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    // grid records: [T][lpc][4] = {obs_H, obs_ICU, obs_D, times[k+1]}
    std::vector<double> grid((size_t)T * lpc * 4, qnan);
    const double* obs_ptr[3] = {pb->obs_H, pb->obs_ICU, pb->obs_D};
    for (int k = 0; k < T; ++k)
        for (int i = 0; i < lpc; ++i) {
            double* rec = &grid[((size_t)k * lpc + i) * 4];
            const int r = k - runup_offset;
            if (i < n && r >= 0 && r < n_obs)
                for (int s = 0; s < 3; ++s) rec[s] = obs_ptr[s][(size_t)r * n + i];
            rec[3] = pb->times[k + 1 < T ? k + 1 : T - 1];
        }

    // merged beta/kappa schedule (see DevProblem)
    std::vector<double> mends;
    for (int k = 0; k < nb; ++k) mends.push_back(pb->beta_end_times[k]);
    for (int k = 0; k < nk; ++k) mends.push_back(pb->kappa_end_times[k]);
    std::sort(mends.begin(), mends.end());
    mends.erase(std::unique(mends.begin(), mends.end()), mends.end());
    const int nm = (int)mends.size();
    std::vector<int32_t> seg_ib(nm + 1, 0), seg_ik(nm + 1, 0);
    for (int j = 0; j <= nm; ++j) {
        const double trep = j < nm ? mends[j] : std::numeric_limits<double>::infinity();
        int cb = 0, ckk = 0;
        for (int k = 0; k < nb; ++k) cb += (trep > pb->beta_end_times[k]) ? 1 : 0;
        for (int k = 0; k < nk; ++k) ckk += (trep > pb->kappa_end_times[k]) ? 1 : 0;
        seg_ib[j] = nb > 0 ? std::min(cb, nb - 1) : 0;
        seg_ik[j] = std::min(ckk, nk - 1);
    }
    if (nm & 1) mends.push_back(std::numeric_limits<double>::infinity());

    double max_gap = 0.0;
    for (int i = 1; i < T; ++i) max_gap = std::max(max_gap, pb->times[i] - pb->times[i - 1]);

    ctx->lower.assign(P, 0.0); ctx->upper.assign(P, 0.0); ctx->has_bounds.assign(P, 0);
    std::vector<int32_t> hb(P, 0);
    for (int p = 0; p < P; ++p) {
        const bool has = pb->has_bounds ? pb->has_bounds[p] != 0 : (pb->lower && pb->upper);
        ctx->has_bounds[p] = has ? 1 : 0;
        hb[p] = has ? 1 : 0;
        if (has) { ctx->lower[p] = pb->lower[p]; ctx->upper[p] = pb->upper[p]; }
    }

    DevProblem& d = ctx->dp;
    d.n = n; d.lpc = lpc; d.T = T; d.n_obs = n_obs; d.runup_offset = runup_offset; d.nb = nb; d.nk = nk;
    d.P = P; d.ns = ns;
    d.constraint_mode = pb->constraint_mode == SEPAIHRD_CONSTRAINT_REFLECT ? 1 : 0;
    d.kappa_calibrated = kappa_calibrated;
    d.max_attempts = pb->max_attempts > 0 ? pb->max_attempts : 1000000;
    d.obs_rows_match = (num_obs_points == n_obs) ? 1 : 0;
    d.abs_tol = pb->abs_err; d.rel_tol = pb->rel_err; d.dt_hint = pb->dt_hint; d.max_gap = max_gap;

    bool ok = true;
    d.times = upload(ctx->allocs, std::vector<double>(pb->times, pb->times + T), ok);
    d.grid = upload(ctx->allocs, grid, ok);
    ctx->host_grid = grid;
    d.lower = upload(ctx->allocs, ctx->lower, ok);
    d.upper = upload(ctx->allocs, ctx->upper, ok);
    d.has_bounds = upload(ctx->allocs, hb, ok);
    d.src_scalar = upload(ctx->allocs, src_scalar, ok);
    d.base_scalar = upload(ctx->allocs, base_scalar, ok);
    d.src_vec = upload(ctx->allocs, src_vec, ok);
    d.base_vec = upload(ctx->allocs, base_vec, ok);
    d.N = upload(ctx->allocs, Npad, ok);
    d.age_fraction = upload(ctx->allocs, fracpad, ok);
    d.Mrow = upload(ctx->allocs, Mrow, ok);
    d.init_state = upload(ctx->allocs, init, ok);
    d.beta_ends = upload(ctx->allocs, std::vector<double>(pb->beta_end_times, pb->beta_end_times + nb), ok);
    d.kappa_ends = upload(ctx->allocs, std::vector<double>(pb->kappa_end_times, pb->kappa_end_times + nk), ok);
    d.nm = nm; d.nm_pad = (int)mends.size();
    d.mends = upload(ctx->allocs, mends, ok);
    d.seg_ib = upload(ctx->allocs, seg_ib, ok);
    d.seg_ik = upload(ctx->allocs, seg_ik, ok);
    if (!ok) {
        set_err(err, errlen, "device allocation / upload failed");
        sepaihrd_destroy(ctx);
        return nullptr;
    }
    if (eval_lds_bytes(d) + LOG_TABLE_LDS_BYTES > 64 * 1024) {  // dynamic + the static 2 KB of the Poisson term's log table
        set_err(err, errlen, "n_params too large for the LDS staging buffer");
        sepaihrd_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void sepaihrd_destroy(sepaihrd_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    delete ctx;
}

const char* sepaihrd_last_error(const sepaihrd_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "ctx is NULL"; }

int sepaihrd_set_constraint_mode(sepaihrd_ctx* ctx, int mode) {
    if (!ctx || (mode != SEPAIHRD_CONSTRAINT_CLAMP && mode != SEPAIHRD_CONSTRAINT_REFLECT))
        return SEPAIHRD_E_INVALID_ARG;
    ctx->dp.constraint_mode = mode;
    return SEPAIHRD_OK;
}

int sepaihrd_set_arith(sepaihrd_ctx* ctx, int arith) {
    if (!ctx || (arith != SEPAIHRD_ARITH_STRICT && arith != SEPAIHRD_ARITH_FMA)) return SEPAIHRD_E_INVALID_ARG;
    ctx->arith = arith;
    return SEPAIHRD_OK;
}

int sepaihrd_set_precision(sepaihrd_ctx* ctx, int precision) {
    if (!ctx || (precision != SEPAIHRD_PRECISION_F64 && precision != SEPAIHRD_PRECISION_F32)) return SEPAIHRD_E_INVALID_ARG;
    if (precision == SEPAIHRD_PRECISION_F32 && ctx->dp.lpc < 4) {
        ctx->last_error = "the fp32-state arm is built for 3 to 16 age classes";
        return SEPAIHRD_E_UNSUPPORTED;
    }
    if (precision == SEPAIHRD_PRECISION_F32 && ctx->solver == SEPAIHRD_SOLVER_FEHLBERG78) {
        ctx->last_error = "the fp32-state arm is built for Dopri5 and Cash-Karp only";
        return SEPAIHRD_E_UNSUPPORTED;
    }
    ctx->precision = precision;
    return SEPAIHRD_OK;
}

int sepaihrd_set_dispersion(sepaihrd_ctx* ctx, const double* k) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    char msg[256] = "";
    const int rc = validated(ctx, sepaihrd_particle_nb_validate(k, msg, (int)sizeof(msg)), msg);
    if (rc != SEPAIHRD_OK) return rc;
    for (int s = 0; s < 3; ++s)
        if (ctx->disp.src[s] < 0) ctx->disp.fixed[s] = k[s];
    return SEPAIHRD_OK;
}

int sepaihrd_get_dispersion(const sepaihrd_ctx* ctx, double* k) {
    if (!ctx || !k) return SEPAIHRD_E_INVALID_ARG;
    for (int s = 0; s < 3; ++s) k[s] = ctx->disp.src[s] >= 0 ? std::numeric_limits<double>::quiet_NaN() : ctx->disp.fixed[s];
    return SEPAIHRD_OK;
}

int sepaihrd_reserve(sepaihrd_ctx* ctx, int max_B) {
    if (!ctx || max_B < 0) return SEPAIHRD_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    return ensure_workspace(ctx, chunk_chains(ctx, (size_t)max_B));
}

int sepaihrd_eval_batch_device(sepaihrd_ctx* ctx, const double* d_theta, int B, double* d_loglik,
                               int32_t* d_status, int32_t* d_n_accept, int32_t* d_n_reject,
                               double* d_ll_parts, double* d_traj, void* stream) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (B < 0 || (B > 0 && (!d_theta || !d_loglik))) {
        ctx->last_error = "eval_batch_device: NULL theta/loglik or negative B";
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (B == 0) return SEPAIHRD_OK;
    // The workspace grows on the first call for a larger batch (an allocation: call sepaihrd_reserve
    // beforehand when the launch must be allocation-free, e.g. under stream capture).
    // batches that fill the chip use the inline-likelihood kernel and need no workspace / chunking
    // a dispersed context parks its increments whatever the batch: the negative-binomial pass reads them
    const bool dispersed = nb_any_dispersed(ctx->disp);
    if (dispersed && ctx->precision == SEPAIHRD_PRECISION_F32) {
        ctx->last_error = "eval_batch_device: the negative-binomial likelihood reads the fp64 integrator's parked increments (set precision F64)";
        return SEPAIHRD_E_UNSUPPORTED;
    }
    const int force_split = dispersed ? FORCE_SPLIT_PARK_ONLY : 0;
    const int needs = needs_workspace(ctx, B, force_split);
    if (needs < 0) { ctx->last_error = "unsupported lanes-per-chain"; return SEPAIHRD_E_UNSUPPORTED; }
    const bool split = needs != 0;
    const size_t chunk = split ? chunk_chains(ctx, (size_t)B) : (size_t)B;
    if (split) {
        const int rc = ensure_workspace(ctx, chunk);
        if (rc != SEPAIHRD_OK) return rc;
    }
    {
        const int rc = fence_before(ctx, static_cast<hipStream_t>(stream));
        if (rc != SEPAIHRD_OK) return rc;
    }
    const size_t traj_per_chain = (size_t)ctx->T * NUM_COMP * ctx->n;
    for (size_t off = 0; off < (size_t)B; off += chunk) {
        const int nb = (int)std::min(chunk, (size_t)B - off);
        hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
        if (ctx->timing && (ctx->timing_seen++ % ctx->timing_period) == 0) {
            while (ctx->ev.size() < ctx->ev_used + 3) {
                Event e;
                HIP_TRY(hipEventCreate(&e), ctx, return SEPAIHRD_E_HIP);
                ctx->ev.push_back(std::move(e));
            }
            e0 = ctx->ev[ctx->ev_used]; e1 = ctx->ev[ctx->ev_used + 1]; e2 = ctx->ev[ctx->ev_used + 2];
            ctx->ev_used += 3;
            (void)hipEventRecord(e0, static_cast<hipStream_t>(stream));
        }
        EvalOutputs out{d_loglik + off,
                        d_status ? d_status + off : nullptr,
                        d_n_accept ? d_n_accept + off : nullptr,
                        d_n_reject ? d_n_reject + off : nullptr,
                        d_ll_parts ? d_ll_parts + 3 * off : nullptr,
                        d_traj ? d_traj + off * traj_per_chain : nullptr,
                        ctx->ws_cum, ctx->ws_rows, ctx->ws_status, e1, force_split};
        const double* th = d_theta + off * (size_t)ctx->P;
        int rc = ctx->precision == SEPAIHRD_PRECISION_F32 ? launch_eval_f32(ctx->dp, ctx->solver, th, nb, out, stream)
                 : ctx->arith == SEPAIHRD_ARITH_FMA       ? launch_eval_fma(ctx->dp, ctx->solver, th, nb, out, stream)
                                                          : launch_eval_strict(ctx->dp, ctx->solver, th, nb, out, stream);
        if (rc == 0 && dispersed) {
            ctx->disp.fused_poisson = ctx->arith == SEPAIHRD_ARITH_FMA ? 1 : 0;
            rc = launch_nb_objective_pass(ctx->dp, th, nb, out, ctx->disp, stream);
        }
        if (rc != 0) {
            ctx->last_error = rc == -4 ? "unsupported lanes-per-chain"
                              : rc == -5 ? "launch needs the likelihood workspace but none was sized for it"
                                         : "kernel launch failed";
            return rc == -4 ? SEPAIHRD_E_UNSUPPORTED : SEPAIHRD_E_HIP;
        }
        if (e2) (void)hipEventRecord(e2, static_cast<hipStream_t>(stream));
    }
    fence_after(ctx, static_cast<hipStream_t>(stream));
    return SEPAIHRD_OK;
}

int sepaihrd_set_timing(sepaihrd_ctx* ctx, int enable) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    ctx->timing = enable != 0;
    ctx->timing_period = enable > 1 ? enable : 1;
    ctx->timing_seen = 0;
    ctx->ev_used = 0;
    return SEPAIHRD_OK;
}

int sepaihrd_get_timing(sepaihrd_ctx* ctx, double* integrator_ms, double* likelihood_ms, int* launches) {
    if (!ctx || !integrator_ms || !likelihood_ms || !launches) return SEPAIHRD_E_INVALID_ARG;
    double a = 0.0, b = 0.0;
    const size_t n = ctx->ev_used / 3;
    for (size_t i = 0; i < n; ++i) {
        float m0 = 0.f, m1 = 0.f;
        HIP_TRY(hipEventSynchronize(ctx->ev[3 * i + 2]), ctx, return SEPAIHRD_E_HIP);
        HIP_TRY(hipEventElapsedTime(&m0, ctx->ev[3 * i], ctx->ev[3 * i + 1]), ctx, return SEPAIHRD_E_HIP);
        HIP_TRY(hipEventElapsedTime(&m1, ctx->ev[3 * i + 1], ctx->ev[3 * i + 2]), ctx, return SEPAIHRD_E_HIP);
        a += m0; b += m1;
    }
    *integrator_ms = a; *likelihood_ms = b; *launches = (int)n;
    ctx->ev_used = 0;
    return SEPAIHRD_OK;
}

int sepaihrd_eval_batch(sepaihrd_ctx* ctx, const double* theta, int B, double* loglik, int32_t* status,
                        int32_t* n_accept, int32_t* n_reject, double* ll_parts, double* traj) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (B < 0 || (B > 0 && (!theta || !loglik))) {
        ctx->last_error = "eval_batch: NULL theta/loglik or negative B";
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (B == 0) return SEPAIHRD_OK;
    if (!traj) {  // the common case: asynchronous copies on the context's stream and ONE wait
        const int rc = sepaihrd_eval_batch_begin(ctx, theta, B);
        return rc != SEPAIHRD_OK ? rc : sepaihrd_eval_batch_end(ctx, loglik, status, n_accept, n_reject, ll_parts);
    }
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    const size_t traj_elems = traj ? (size_t)B * ctx->T * NUM_COMP * ctx->n : 0;
    if (ctx->pending_B > 0) { ctx->last_error = "eval_batch: a sepaihrd_eval_batch_begin is pending"; return SEPAIHRD_E_INVALID_ARG; }
    {
        const int rc = ensure_staging(ctx, (size_t)B);
        if (rc != SEPAIHRD_OK) return rc;
    }
    ALLOC_TRY(ctx->traj_buf.get(&ctx->d_traj, traj_elems), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(ctx->d_theta, theta, (size_t)B * ctx->P * sizeof(double), hipMemcpyHostToDevice), ctx,
            return SEPAIHRD_E_HIP);
    const int rc = sepaihrd_eval_batch_device(ctx, ctx->d_theta, B, ctx->d_loglik, ctx->d_status, ctx->d_nacc,
                                              ctx->d_nrej, ctx->d_parts, traj ? ctx->d_traj : nullptr, nullptr);
    if (rc != SEPAIHRD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    {
        const int rcf = fetch_results(ctx, nullptr, B, loglik, status, n_accept, n_reject, ll_parts);
        if (rcf != SEPAIHRD_OK) return rcf;
    }
    if (traj)
        HIP_TRY(hipMemcpy(traj, ctx->d_traj, traj_elems * sizeof(double), hipMemcpyDeviceToHost), ctx,
                return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

// The host-pointer evaluation in two halves on a stream of the context's own, so that a caller with two contexts
// (the finite-difference objective: centre value and perturbed batch) has both in flight at once.
int sepaihrd_eval_batch_begin(sepaihrd_ctx* ctx, const double* theta, int B) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (B <= 0 || !theta) { ctx->last_error = "eval_batch_begin: NULL theta or B <= 0"; return SEPAIHRD_E_INVALID_ARG; }
    if (ctx->pending_B > 0) { ctx->last_error = "eval_batch_begin: the previous begin has no end yet"; return SEPAIHRD_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    if (!ctx->own_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking), ctx, return SEPAIHRD_E_HIP);
    {
        const int rc = ensure_staging(ctx, (size_t)B);
        if (rc != SEPAIHRD_OK) return rc;
    }
    if (sepaihrd_reserve(ctx, B) != SEPAIHRD_OK) return SEPAIHRD_E_HIP;  // workspace growth is not stream-ordered
    HIP_TRY(hipMemcpyAsync(ctx->d_theta, theta, (size_t)B * ctx->P * sizeof(double), hipMemcpyHostToDevice, ctx->own_stream), ctx,
            return SEPAIHRD_E_HIP);
    const int rc = sepaihrd_eval_batch_device(ctx, ctx->d_theta, B, ctx->d_loglik, ctx->d_status, ctx->d_nacc, ctx->d_nrej,
                                              ctx->d_parts, nullptr, ctx->own_stream);
    if (rc != SEPAIHRD_OK) return rc;
    ctx->pending_B = B;
    return SEPAIHRD_OK;
}

int sepaihrd_eval_batch_end(sepaihrd_ctx* ctx, double* loglik, int32_t* status, int32_t* n_accept, int32_t* n_reject,
                            double* ll_parts) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    const int B = ctx->pending_B;
    if (B <= 0) { ctx->last_error = "eval_batch_end: nothing pending"; return SEPAIHRD_E_INVALID_ARG; }
    ctx->pending_B = 0;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    return fetch_results(ctx, ctx->own_stream, B, loglik, status, n_accept, n_reject, ll_parts);
}

// Forward differences of C centres in one pass (see include/sepaihrd_hip.h): upload, builder kernel and the G P perturbed
// evaluations on the perturbed context's stream, the C centre evaluations on the centre context's stream, the quotient
// kernel behind both, one copy home and ONE wait.  The two streams are ordered by events only.
int sepaihrd_fd_gradient_batch(sepaihrd_ctx* cc, sepaihrd_ctx* pc, const double* theta, const uint8_t* want_grad, int C,
                               double fd_epsilon, const int32_t* mult_index, double* value, double* grad, int32_t* status) {
    if (!cc || !pc) return SEPAIHRD_E_INVALID_ARG;
    auto bad = [&](const char* msg, int rc) { pc->last_error = std::string("fd_gradient_batch: ") + msg; return rc; };
    if (C < 0 || (C > 0 && (!theta || !value || !grad || !status || !mult_index))) return bad("NULL argument or negative C", SEPAIHRD_E_INVALID_ARG);
    if (cc->device != pc->device || cc->P != pc->P || cc->n != pc->n)
        return bad("the two contexts are not of one problem on one device", SEPAIHRD_E_INVALID_ARG);
    if (cc->precision != SEPAIHRD_PRECISION_F64 || pc->precision != SEPAIHRD_PRECISION_F64)
        return bad("not built for contexts in SEPAIHRD_PRECISION_F32", SEPAIHRD_E_UNSUPPORTED);
    if (cc->pending_B > 0 || pc->pending_B > 0) return bad("a sepaihrd_eval_batch_begin is pending on one of the contexts", SEPAIHRD_E_INVALID_ARG);
    if (C == 0) return SEPAIHRD_OK;
    const size_t P = (size_t)pc->P, nC = (size_t)C;
    for (int j = 0; j < 8; ++j)
        if (mult_index[j] >= (int32_t)P) return bad("mult_index entry beyond the parameter count", SEPAIHRD_E_INVALID_ARG);
    std::vector<int32_t> rows;
    rows.reserve(nC);
    for (int c = 0; c < C; ++c)
        if (!want_grad || want_grad[c]) rows.push_back(c);
    const size_t G = rows.size(), GP = G * P;
    if (nC * P > FD_MAX_PERTURBED_ROWS) return bad("C x n_params above 2^22 rows: split the batch", SEPAIHRD_E_UNSUPPORTED);
    HIP_TRY(hipSetDevice(pc->device), pc, return SEPAIHRD_E_HIP);
    for (sepaihrd_ctx* c : {cc, pc})
        if (!c->own_stream) HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking), pc, return SEPAIHRD_E_HIP);
    for (hipEvent_t* e : {&pc->fd_ev_uploaded, &pc->fd_ev_centre})
        if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming), pc, return SEPAIHRD_E_HIP);
    // sized for G = C, so that the want_grad mask never makes a later call allocate
    const size_t dbl = nC * P * P + 2 * nC * P /* plus, eps, f_plus */ + nC * P /* theta */ + nC + nC * P /* value, grad */;
    const size_t i32 = nC /* status */ + nC * P /* plus_status */ + nC /* centre_status */ + nC /* rows */;
    const size_t need = dbl * sizeof(double) + i32 * sizeof(int32_t);
    const size_t result_bytes = (nC + GP) * sizeof(double) + nC * sizeof(int32_t);
    ALLOC_TRY(pc->fd_dev.reserve(need), pc, return SEPAIHRD_E_HIP);  // not stream-ordered: before anything is queued
    const size_t host_need = (nC + nC * P) * sizeof(double) + nC * sizeof(int32_t);
    ALLOC_TRY(pc->fd_host.reserve(host_need), pc, return SEPAIHRD_E_HIP);
    if (sepaihrd_reserve(cc, C) != SEPAIHRD_OK) return bad(cc->last_error.c_str(), SEPAIHRD_E_HIP);
    if (G > 0 && sepaihrd_reserve(pc, (int)GP) != SEPAIHRD_OK) return SEPAIHRD_E_HIP;
    // carve; the results [value C][grad G P][status C] are contiguous: one copy home
    double* d_plus = pc->fd_dev.as<double>();
    double* d_eps = d_plus + nC * P * P;
    double* d_fplus = d_eps + nC * P;
    double* d_theta = d_fplus + nC * P;
    double* d_value = d_theta + nC * P;
    double* d_grad = d_value + nC;
    int32_t* d_status = reinterpret_cast<int32_t*>(d_grad + GP);
    int32_t* d_pstatus = reinterpret_cast<int32_t*>(d_grad + nC * P) + nC;
    int32_t* d_cstatus = d_pstatus + nC * P;
    int32_t* d_rows = d_cstatus + nC;
    hipStream_t sp = pc->own_stream, sc = cc->own_stream;
    HIP_TRY(hipMemcpyAsync(d_theta, theta, nC * P * sizeof(double), hipMemcpyHostToDevice, sp), pc, return SEPAIHRD_E_HIP);
    if (G > 0) HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), G * sizeof(int32_t), hipMemcpyHostToDevice, sp), pc, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemsetAsync(d_status, 0, nC * sizeof(int32_t), sp), pc, return SEPAIHRD_E_HIP);
    HIP_TRY(hipEventRecord(pc->fd_ev_uploaded, sp), pc, return SEPAIHRD_E_HIP);
    if (G > 0) {  // the perturbed evaluations do not depend on the centres': queued first, they run beside them
        if (launch_fd_build(d_theta, d_rows, (int)G, (int)P, fd_epsilon, d_plus, d_eps, sp) != 0) return bad("builder launch failed", SEPAIHRD_E_HIP);
        const int rc = sepaihrd_eval_batch_device(pc, d_plus, (int)GP, d_fplus, d_pstatus, nullptr, nullptr, nullptr, nullptr, sp);
        if (rc != SEPAIHRD_OK) return rc;
    }
    if (sc != sp) HIP_TRY(hipStreamWaitEvent(sc, pc->fd_ev_uploaded, 0), pc, return SEPAIHRD_E_HIP);
    {
        const int rc = sepaihrd_eval_batch_device(cc, d_theta, C, d_value, d_cstatus, nullptr, nullptr, nullptr, nullptr, sc);
        if (rc != SEPAIHRD_OK) return bad(cc->last_error.c_str(), rc);
    }
    if (sc != sp) {
        HIP_TRY(hipEventRecord(pc->fd_ev_centre, sc), pc, return SEPAIHRD_E_HIP);
        HIP_TRY(hipStreamWaitEvent(sp, pc->fd_ev_centre, 0), pc, return SEPAIHRD_E_HIP);
    }
    FdQuotientArgs qa{};
    qa.C = C; qa.G = (int32_t)G; qa.P = (int32_t)P; qa.n = pc->dp.n; qa.lpc = pc->dp.lpc;
    for (int j = 0; j < 8; ++j) qa.mult_index[j] = mult_index[j];
    qa.rows = d_rows; qa.plus = d_plus; qa.eps = d_eps; qa.f_plus = d_fplus; qa.plus_status = d_pstatus;
    qa.value = d_value; qa.centre_status = d_cstatus; qa.init_state = pc->dp.init_state; qa.N = pc->dp.N;
    qa.grad = d_grad; qa.status = d_status;
    if (launch_fd_quotient(qa, sp) != 0) return bad("quotient launch failed", SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpyAsync(pc->fd_host.p, d_value, result_bytes, hipMemcpyDeviceToHost, sp), pc, return SEPAIHRD_E_HIP);
    HIP_TRY(hipStreamSynchronize(sp), pc, return SEPAIHRD_E_HIP);
    const char* h = pc->fd_host.as<char>();
    std::memcpy(value, h, nC * sizeof(double));
    const double* hg = reinterpret_cast<const double*>(h) + nC;
    for (size_t g = 0; g < G; ++g) std::memcpy(grad + (size_t)rows[g] * P, hg + g * P, P * sizeof(double));
    std::memcpy(status, h + (nC + GP) * sizeof(double), nC * sizeof(int32_t));
    return SEPAIHRD_OK;
}

int sepaihrd_set_initial_state_mode(sepaihrd_ctx* ctx, int mode) {
    if (!ctx || mode < SEPAIHRD_INIT_FROM_THETA || mode > SEPAIHRD_INIT_MULTIPLIERS) return SEPAIHRD_E_INVALID_ARG;
    ctx->dp.init_mode = mode;
    return SEPAIHRD_OK;
}

int sepaihrd_set_integrator_form(sepaihrd_ctx* ctx, int form) {
    if (!ctx || form < SEPAIHRD_FORM_AUTO || form > SEPAIHRD_FORM_QUAD) return SEPAIHRD_E_INVALID_ARG;
    if (form == SEPAIHRD_FORM_QUAD && ctx->dp.lpc != 4) {
        ctx->last_error = "set_integrator_form: the sixteen-lanes-per-chain form exists for problems of 3 or 4 age classes";
        return SEPAIHRD_E_UNSUPPORTED;
    }
    if (form == SEPAIHRD_FORM_QUAD && ctx->solver == SEPAIHRD_SOLVER_FEHLBERG78) {
        ctx->last_error = "set_integrator_form: the sixteen-lanes-per-chain form is not built for the Fehlberg 7(8) solver";
        return SEPAIHRD_E_UNSUPPORTED;
    }
    ctx->dp.form = form;
    return SEPAIHRD_OK;
}

int sepaihrd_ensemble_quantiles(sepaihrd_ctx* ctx, const double* theta, int S, const double* probs, int n_probs,
                                double* ppc_quantiles, double* sero_quantiles, double* rt_quantiles, double* metrics,
                                int32_t* status, int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    const char* const who = "ensemble_quantiles";
    int rc = ensemble_preflight(ctx, who, S > 0 && theta && probs && ppc_quantiles, "need S > 0, theta, probs (1..1024) and ppc_quantiles",
                                CHECK_PROBS | CHECK_PENDING | CHECK_F64 | CHECK_TP, probs, n_probs);
    if (rc != SEPAIHRD_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    // sizes
    const DevProblem& dp = ctx->dp;
    const int Tp = dp.T - dp.runup_offset;
    const SegmentPlan plan = plan_segments((size_t)S);  // a segment: the S samples of one (series, time, age)
    const int S_pad = (int)plan.pad;
    const size_t cpw = (size_t)(WAVE / dp.lpc);
    const size_t chains = ((size_t)S + cpw - 1) / cpw * cpw;
    const bool want_sero = sero_quantiles != nullptr, want_metrics = metrics != nullptr;
    const bool want_rt = rt_quantiles != nullptr || want_metrics;  // the metric table reads the Rt values
    const bool want_traj = want_sero || want_rt;
    const size_t n_ppc = (size_t)6 * n_probs * Tp * dp.n;
    const size_t n_sero = want_sero ? (size_t)n_probs * dp.T : 0;
    const size_t n_rt = want_rt ? (size_t)n_probs * dp.T : 0;
    const size_t n_vals = ((size_t)6 * Tp * dp.n + (want_sero ? dp.T : 0) + (want_rt ? dp.T : 0)) * S_pad;
    const size_t n_traj = want_traj ? (size_t)S * dp.T * NUM_COMP * dp.n : 0;
    const size_t n_scratch = sort_scratch_doubles(plan, n_vals);
    const size_t n_metrics = want_metrics ? (size_t)S * (12 + 4 * dp.n) : 0;
    // buffers: they stay with the context
    rc = ensure_workspace(ctx, chains);
    if (rc != SEPAIHRD_OK) return rc;
    if (want_rt && dp.n > 16) return refuse(ctx, who, "Rt trajectories are built for at most 16 age classes", SEPAIHRD_E_UNSUPPORTED);
    double *d_theta = nullptr, *d_ll = nullptr, *d_vals = nullptr, *d_traj = nullptr, *d_probs = nullptr, *d_q = nullptr,
           *d_metrics = nullptr, *d_scratch = nullptr;
    int32_t* d_nv = nullptr;
    auto& slots = ctx->ens;
    if (!slots.get(SLOT_THETA, &d_theta, (size_t)S * ctx->P) || !slots.get(SLOT_LOGLIK, &d_ll, (size_t)S) ||
        !slots.get(SLOT_VALS, &d_vals, n_vals) || !slots.get(SLOT_TRAJ, &d_traj, n_traj) ||
        !slots.get(SLOT_PROBS, &d_probs, (size_t)n_probs) || !slots.get(SLOT_QUANTILES, &d_q, n_ppc + n_sero + n_rt) ||
        !slots.get(SLOT_N_VALID, &d_nv, 1) || !slots.get(SLOT_METRICS, &d_metrics, n_metrics) ||
        !slots.get(SLOT_SORT_SCRATCH, &d_scratch, n_scratch))
        return refuse(ctx, who, "device allocation failed", SEPAIHRD_E_HIP);
    // uploads
    HIP_TRY(hipMemcpy(d_theta, theta, (size_t)S * ctx->P * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(d_probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    // launches
    EvalOutputs out{d_ll, nullptr, nullptr, nullptr, nullptr, want_traj ? d_traj : nullptr,
                    ctx->ws_cum, ctx->ws_rows, ctx->ws_status, nullptr, 1};
    rc = fence_before(ctx, nullptr);  // an evaluation of this context may still be running on another stream
    if (rc != SEPAIHRD_OK) return rc;
    rc = launch_eval_for(ctx, "", d_theta, S, out);
    if (rc != SEPAIHRD_OK) return rc;
    EnsembleArgs a{};
    a.S = S; a.S_pad = S_pad; a.lpc = dp.lpc; a.n = dp.n; a.T = dp.T; a.Tp = Tp; a.runup_offset = dp.runup_offset;
    a.n_probs = n_probs;
    a.cum_stride = chains * dp.lpc;
    a.cum = ctx->ws_cum; a.wstatus = ctx->ws_status; a.traj = want_traj ? d_traj : nullptr;
    a.total_pop = total_population(ctx);
    a.vals = d_vals; a.probs = d_probs; a.q_out = d_q; a.sero_out = want_sero ? d_q + n_ppc : nullptr; a.n_valid = d_nv;
    a.rt_out = want_rt ? d_q + n_ppc + n_sero : nullptr;
    a.rt_segment0 = 6 * Tp * dp.n + (want_sero ? dp.T : 0);
    a.pb = &ctx->dp;
    a.theta = d_theta;
    a.metrics_out = want_metrics ? d_metrics : nullptr;
    a.sort_scratch = plan.in_lds ? nullptr : d_scratch;
    a.sort_scratch_doubles = n_scratch;
    if (launch_ensemble_summaries(a, nullptr) != 0) {
        ctx->last_error = "ensemble summary launch failed";
        return SEPAIHRD_E_HIP;
    }
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    // fetches
    HIP_TRY(hipMemcpy(ppc_quantiles, d_q, n_ppc * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (want_sero)
        HIP_TRY(hipMemcpy(sero_quantiles, d_q + n_ppc, n_sero * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (rt_quantiles)
        HIP_TRY(hipMemcpy(rt_quantiles, d_q + n_ppc + n_sero, n_rt * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (want_metrics)
        HIP_TRY(hipMemcpy(metrics, d_metrics, n_metrics * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (status)
        HIP_TRY(hipMemcpy(status, ctx->ws_status, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (n_valid) HIP_TRY(hipMemcpy(n_valid, d_nv, sizeof(int32_t), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

// The body of sepaihrd_ensemble_predictive and sepaihrd_ensemble_predictive_nb.  nb == nullptr: the Poisson call, the draw kernel
// with no dispersion table.  Otherwise the dispersion every sample's draws take: the call's own three values (src = -1 throughout) or the
// context's (the objective's rule, per sample), resolved on the device into k_used [S][3].
// sr (sepaihrd_ensemble_predictive_scores; null: no scores): the segments are scored where they are sorted and the mid-PIT comes
// from the sorted segment, so the draw launch takes no PIT pass.
struct ScoreRequest {
    const double* observed;  // [3][T_pos][n_age] host or null: the context's observations
    const double* levels;
    int n_levels;
    double *cell_scores, *summary;
    int32_t* exact;
};
// tr (sepaihrd_ensemble_predictive_targets; null: the daily cells): the draws are summed into the 6 W G target segments of
// csrc/sepaihrd_predictive_targets.inc and those are sorted and scored; the 6 T_pos n_age table is not allocated.  Its score
// request's cell_scores and summary are the target outputs, and pred_quantiles and pit of the call are the targets' too.
struct TargetRequest {
    ScoreRequest score;
    const int32_t* age_group;  // [n_age] host
    int window, origin, W, G;
    double *target_obs, *target_draws;
};
static int predictive_call(sepaihrd_ctx* ctx, const double* theta, int S, int R, uint64_t seed, const NbDispersion* nb, const double* probs,
                           int n_probs, double* pred_quantiles, double* pit, double* means, double* draws, double* k_used, int32_t* status,
                           int32_t* n_valid, const ScoreRequest* sr = nullptr, const TargetRequest* tr = nullptr) {
    if (tr) sr = &tr->score;
    const char* const who = tr ? "ensemble_predictive_targets" : sr ? "ensemble_predictive_scores" : "ensemble_predictive";
    int rc = ensemble_preflight(ctx, who, S > 0 && theta && probs && pred_quantiles, "need S > 0, theta, probs (1..1024) and pred_quantiles",
                                CHECK_PENDING | CHECK_F64 | CHECK_TP, probs, n_probs);
    if (rc != SEPAIHRD_OK) return rc;
    const DevProblem& dp = ctx->dp;
    const int Tp = dp.T - dp.runup_offset;
    char msg[256] = "";
    rc = validated(ctx, sr ? sepaihrd_predictive_scores_validate(S, R, Tp, dp.n, probs, n_probs, sr->levels, sr->n_levels, msg, (int)sizeof(msg))
                              : sepaihrd_predictive_validate(S, R, Tp, dp.n, probs, n_probs, msg, (int)sizeof(msg)), msg);
    if (rc != SEPAIHRD_OK) return rc;
    if (sr && !sr->cell_scores) return refuse(ctx, who, tr ? "target_scores must not be NULL" : "cell_scores must not be NULL", SEPAIHRD_E_INVALID_ARG);
    if (sr && !sr->summary) return refuse(ctx, who, "summary must not be NULL", SEPAIHRD_E_INVALID_ARG);
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    // sizes
    const size_t N = (size_t)S * (size_t)R;
    const SegmentPlan plan = plan_segments(N);  // a segment: the S R draws of one (series, time, age)
    const size_t N_pad = plan.pad;
    if (N_pad >= ((size_t)1 << 31)) return refuse(ctx, who, "S x R rounded up to whole wavefronts must stay below 2^31", SEPAIHRD_E_INVALID_ARG);
    const size_t cpw = (size_t)(WAVE / dp.lpc);
    const size_t chains = ((size_t)S + cpw - 1) / cpw * cpw;
    const size_t cells = (size_t)3 * Tp * dp.n;
    // the sorted and scored cells: the daily ones and their running sums, or the targets (3 W G window totals and their running sums)
    const size_t seg_cells = tr ? (size_t)3 * tr->W * tr->G : cells;
    const size_t n_q = 2 * seg_cells * (size_t)n_probs;
    const size_t n_vals = 2 * seg_cells * N_pad;
    const size_t n_scratch = sort_scratch_doubles(plan, n_vals);
    const size_t n_means = means ? (size_t)S * cells : 0, n_draws = draws ? N * cells : 0;
    const size_t n_k = nb ? (size_t)S * 3 : 0;
    const size_t L = sr ? (size_t)sr->n_levels : 0;
    const size_t n_cs = sr ? (tr ? 2 * seg_cells : cells) * (size_t)(5 + 4 * L) : 0;
    const size_t n_sum = tr ? (size_t)6 * (tr->G + 1) * (4 + 2 * L) : sr ? (size_t)3 * (dp.n + 1) * (4 + 2 * L) : 0, n_obs = sr ? cells : 0;
    const size_t n_pit = tr ? 2 * seg_cells : cells, n_tobs = tr ? 2 * seg_cells : 0, n_tdraws = tr && tr->target_draws ? N * seg_cells : 0;
    const size_t n_ages = tr ? (size_t)dp.n : 0;
    // the rule of sepaihrd_scenario_ensemble: the buffers below plus the likelihood workspace must fit the device's memory
    // (the segment table dominates: 6 T_pos n_age segments of S R doubles)
    const size_t need_bytes = sizeof(double) * ((size_t)S * ctx->P + (size_t)S + n_vals + n_scratch + n_q + n_pit + n_means + n_draws + n_k + (size_t)n_probs +
                                               n_cs + n_sum + n_obs + L + 1 + n_tobs + n_tdraws + n_ages) +
                              sizeof(double) * (workspace_cum_doubles(dp, chains) + workspace_rows_doubles(dp, chains)) +
                              sizeof(int32_t) * (chains + 2);
    rc = require_device_memory(ctx, need_bytes, "ensemble_predictive: the segment table of S x R = " + std::to_string(N) + " draws needs",
                               "split the samples or the replicates over several calls");
    if (rc != SEPAIHRD_OK) return rc;
    // buffers and events of this call alone: the context's own (sepaihrd_ensemble_quantiles') stay as they are
    rc = ensure_workspace(ctx, chains);
    if (rc != SEPAIHRD_OK) return rc;
    CallScratch sc(4);
    double *d_theta = nullptr, *d_ll = nullptr, *d_vals = nullptr, *d_scratch = nullptr, *d_probs = nullptr, *d_q = nullptr, *d_pit = nullptr,
           *d_means = nullptr, *d_draws = nullptr, *d_k = nullptr, *d_cs = nullptr, *d_sum = nullptr, *d_obs = nullptr, *d_levels = nullptr,
           *d_tobs = nullptr, *d_tdraws = nullptr;
    int32_t *d_counts = nullptr, *d_exact = nullptr, *d_group = nullptr, *d_launch = nullptr;
    if (!sc.alloc(&d_theta, (size_t)S * ctx->P) || !sc.alloc(&d_ll, (size_t)S) || !sc.alloc(&d_vals, n_vals) ||
        !sc.alloc(&d_scratch, n_scratch) || !sc.alloc(&d_probs, (size_t)n_probs) || !sc.alloc(&d_q, n_q) || !sc.alloc(&d_pit, n_pit) ||
        !sc.alloc(&d_means, n_means) || !sc.alloc(&d_draws, n_draws) || !sc.alloc(&d_counts, 2) || !sc.alloc(&d_k, n_k) ||
        (sr && (!sc.alloc(&d_cs, n_cs) || !sc.alloc(&d_sum, n_sum) || !sc.alloc(&d_obs, n_obs) || !sc.alloc(&d_levels, L) || !sc.alloc(&d_exact, 1))) ||
        (tr && (!sc.alloc(&d_tobs, n_tobs) || !sc.alloc(&d_tdraws, n_tdraws) || !sc.alloc(&d_group, n_ages) || !sc.alloc(&d_launch, n_ages))))
        return refuse(ctx, who, "device allocation failed", SEPAIHRD_E_HIP);
    for (Event& e : sc.ev) HIP_TRY(hipEventCreate(&e), ctx, return SEPAIHRD_E_HIP);
    // uploads
    HIP_TRY(hipMemcpy(d_theta, theta, (size_t)S * ctx->P * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(d_probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    if (sr) {
        const int32_t one = 1;
        HIP_TRY(hipMemcpy(d_exact, &one, sizeof(one), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
        if (L > 0) HIP_TRY(hipMemcpy(d_levels, sr->levels, L * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
        if (sr->observed) HIP_TRY(hipMemcpy(d_obs, sr->observed, n_obs * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    }
    // the ages the target draw kernel launches: every age where the daily tables are wanted, else those of a group
    std::vector<int32_t> launch_age;
    if (tr) {
        for (int a = 0; a < dp.n; ++a)
            if (means || draws || tr->age_group[a] >= 0) launch_age.push_back(a);
        HIP_TRY(hipMemcpy(d_group, tr->age_group, n_ages * sizeof(int32_t), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
        HIP_TRY(hipMemcpy(d_launch, launch_age.data(), launch_age.size() * sizeof(int32_t), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    }
    // launches
    EvalOutputs out{d_ll, nullptr, nullptr, nullptr, nullptr, nullptr, ctx->ws_cum, ctx->ws_rows, ctx->ws_status, nullptr, 1};
    rc = fence_before(ctx, nullptr);  // an evaluation of this context may still be running on another stream
    if (rc != SEPAIHRD_OK) return rc;
    (void)hipEventRecord(sc.ev[0], nullptr);
    rc = launch_eval_for(ctx, "ensemble_predictive: ", d_theta, S, out);
    if (rc != SEPAIHRD_OK) return rc;
    (void)hipEventRecord(sc.ev[1], nullptr);
    PredictiveArgs a{};
    a.S = S; a.R = R; a.N_pad = (int)N_pad;
    a.lpc = dp.lpc; a.n = dp.n; a.T = dp.T; a.Tp = Tp; a.runup_offset = dp.runup_offset;
    a.seed = seed;
    a.cum = ctx->ws_cum; a.wstatus = ctx->ws_status; a.grid = dp.grid;
    a.vals = d_vals; a.means = means ? d_means : nullptr; a.draws = draws ? d_draws : nullptr;
    a.n_probs = n_probs; a.probs = d_probs; a.q_out = d_q; a.pit_out = pit && !sr ? d_pit : nullptr; a.counts = d_counts;
    a.sort_scratch = plan.in_lds ? nullptr : d_scratch;
    a.sort_scratch_doubles = n_scratch;
    PredictiveTargetArgs ta{};
    if (tr) {
        a.vals = nullptr; a.q_out = nullptr; a.pit_out = nullptr;
        ta.W = tr->W; ta.G = tr->G; ta.window = tr->window; ta.origin = tr->origin;
        ta.n_launch = (int)launch_age.size(); ta.launch_age = d_launch; ta.age_group = d_group;
        ta.tvals = d_vals; ta.q_out = d_q; ta.obs_daily = sr->observed ? d_obs : nullptr; ta.target_obs = d_tobs;
        ta.levels = d_levels; ta.n_levels = sr->n_levels; ta.target_scores = d_cs; ta.summary = d_sum; ta.pit_out = pit ? d_pit : nullptr;
        ta.target_draws = tr->target_draws ? d_tdraws : nullptr; ta.exact = d_exact;
    }
    // the draw phase: the dispersions (none for the Poisson call, whose null table reads k = +inf), the counts, the draws, and
    // the mid-PIT of the unsorted daily table where a.pit_out asks for it
    int drc = nb ? launch_predictive_nb_k(a, dp, d_theta, *nb, d_k, ctx->ws_status, nullptr) : 0;
    if (drc == 0) drc = launch_predictive_counts(a, nullptr);
    if (drc == 0) drc = tr ? launch_predictive_target_draws(a, ta, d_k, nullptr) : launch_predictive_draws(a, nb ? d_k : nullptr, nullptr);
    if (drc == 0) drc = launch_predictive_pit(a, nullptr);
    if (drc != 0) return refuse(ctx, who, "draw kernel launch failed", SEPAIHRD_E_HIP);
    (void)hipEventRecord(sc.ev[2], nullptr);
    if (tr) {
        if (launch_predictive_target_scores(a, ta, nullptr) != 0) return refuse(ctx, who, "score launch failed", SEPAIHRD_E_HIP);
    } else if (sr) {
        PredictiveScoreArgs sa{};
        sa.obs = d_obs; sa.obs_from_grid = sr->observed == nullptr;
        sa.levels = d_levels; sa.n_levels = sr->n_levels;
        sa.cell_scores = d_cs; sa.summary = d_sum; sa.pit_out = pit ? d_pit : nullptr; sa.exact = d_exact;
        if (launch_predictive_scores(a, sa, nullptr) != 0) return refuse(ctx, who, "score launch failed", SEPAIHRD_E_HIP);
    } else if (launch_predictive_quantiles(a, nullptr) != 0) {
        return refuse(ctx, who, "quantile launch failed", SEPAIHRD_E_HIP);
    }
    (void)hipEventRecord(sc.ev[3], nullptr);
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    elapsed_ms(sc.ev, ctx->pred_ms, 3);
    // fetches
    ResultFetch res;
    res.fetch(pred_quantiles, d_q, n_q * sizeof(double));
    res.fetch(pit, d_pit, n_pit * sizeof(double));
    res.fetch(means, d_means, n_means * sizeof(double));
    res.fetch(draws, d_draws, n_draws * sizeof(double));
    res.fetch(k_used, d_k, n_k * sizeof(double));
    res.fetch(status, ctx->ws_status, (size_t)S * sizeof(int32_t));
    res.fetch(n_valid, d_counts, sizeof(int32_t));
    if (sr) {
        res.fetch(sr->cell_scores, d_cs, n_cs * sizeof(double));
        res.fetch(sr->summary, d_sum, n_sum * sizeof(double));
        res.fetch(sr->exact, d_exact, sizeof(int32_t));
    }
    if (tr) {
        res.fetch(tr->target_obs, d_tobs, n_tobs * sizeof(double));
        res.fetch(tr->target_draws, d_tdraws, n_tdraws * sizeof(double));
    }
    if (!res.ok()) return refuse(ctx, who, "copy of the results failed", SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_ensemble_predictive(sepaihrd_ctx* ctx, const double* theta, int S, int R, uint64_t seed, const double* probs, int n_probs,
                                 double* pred_quantiles, double* pit, double* means, double* draws, int32_t* status, int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    return predictive_call(ctx, theta, S, R, seed, nullptr, probs, n_probs, pred_quantiles, pit, means, draws, nullptr, status, n_valid);
}

int sepaihrd_ensemble_predictive_nb(sepaihrd_ctx* ctx, const double* theta, int S, int R, uint64_t seed, const double* dispersion,
                                    const double* probs, int n_probs, double* pred_quantiles, double* pit, double* means, double* draws,
                                    double* k_used, int32_t* status, int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    NbDispersion nb = ctx->disp;  // NULL: what the deterministic objective would use for each theta
    if (dispersion) {
        char msg[256] = "";
        const int rc = validated(ctx, sepaihrd_particle_nb_validate(dispersion, msg, (int)sizeof(msg)), msg);
        if (rc != SEPAIHRD_OK) return rc;
        for (int s = 0; s < 3; ++s) { nb.src[s] = -1; nb.fixed[s] = dispersion[s]; }
    }
    return predictive_call(ctx, theta, S, R, seed, &nb, probs, n_probs, pred_quantiles, pit, means, draws, k_used, status, n_valid);
}

int sepaihrd_predictive_scores_validate(int S, int R, int T_pos, int n_age, const double* probs, int n_probs, const double* levels, int n_levels,
                                        char* err, int errlen) {
    const int rc = sepaihrd_predictive_validate(S, R, T_pos, n_age, probs, n_probs, err, errlen);
    if (rc != SEPAIHRD_OK) return rc;
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, "ensemble_predictive_scores: " + msg); return SEPAIHRD_E_INVALID_ARG; };
    if (n_levels < 0 || n_levels > 8) return refuse("n_levels must lie in 0..8 (central coverage levels)");
    if (n_levels > 0 && !levels) return refuse("levels must not be NULL where n_levels > 0");
    for (int l = 0; l < n_levels; ++l)
        if (!(levels[l] > 0.0 && levels[l] < 1.0)) return refuse("levels must lie strictly inside (0, 1): levels[" + std::to_string(l) + "] does not");
    return SEPAIHRD_OK;
}

int sepaihrd_ensemble_predictive_scores(sepaihrd_ctx* ctx, const double* theta, int S, int R, uint64_t seed, const double* dispersion,
                                        const double* observed, const double* probs, int n_probs, const double* levels, int n_levels,
                                        double* pred_quantiles, double* pit, double* cell_scores, double* summary, double* means, double* draws,
                                        double* k_used, int32_t* status, int32_t* n_valid, int32_t* exact) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    NbDispersion nb = ctx->disp;  // NULL: the context's, as in sepaihrd_ensemble_predictive_nb
    if (dispersion) {
        char msg[256] = "";
        const int rc = validated(ctx, sepaihrd_particle_nb_validate(dispersion, msg, (int)sizeof(msg)), msg);
        if (rc != SEPAIHRD_OK) return rc;
        for (int s = 0; s < 3; ++s) { nb.src[s] = -1; nb.fixed[s] = dispersion[s]; }
    }
    const ScoreRequest sr{observed, levels, n_levels, cell_scores, summary, exact};
    return predictive_call(ctx, theta, S, R, seed, &nb, probs, n_probs, pred_quantiles, pit, means, draws, k_used, status, n_valid, &sr);
}

int sepaihrd_predictive_targets_validate(int S, int R, int T_pos, int n_age, const int32_t* age_group, int window, int origin, const double* probs,
                                         int n_probs, const double* levels, int n_levels, int* W, int* G, char* err, int errlen) {
    const int rc = sepaihrd_predictive_scores_validate(S, R, T_pos, n_age, probs, n_probs, levels, n_levels, err, errlen);
    if (rc != SEPAIHRD_OK) return rc;
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, "ensemble_predictive_targets: " + msg); return SEPAIHRD_E_INVALID_ARG; };
    if (!age_group) return refuse("age_group must not be NULL");
    int where = 0;
    const int groups = sepaihrd_targets::group_count(age_group, n_age, &where);
    if (groups == -1)
        return refuse("age_group[" + std::to_string(where) + "] = " + std::to_string(age_group[where]) + " must be -1 or a group id in 0.." +
                      std::to_string(n_age - 1));
    if (groups == -2) return refuse("age_group puts no age in any group");
    if (groups == -3) return refuse("age_group leaves a gap: no age has group id " + std::to_string(where) + " though a larger id is in use");
    if (window < 1) return refuse("window must be >= 1 output row");
    if (origin < 0) return refuse("origin must be >= 0");
    const int windows = sepaihrd_targets::window_count(T_pos, window, origin);
    if (windows < 1)
        return refuse("origin = " + std::to_string(origin) + " and window = " + std::to_string(window) + " leave no whole window in T_pos = " +
                      std::to_string(T_pos) + " rows (W < 1)");
    if ((uint64_t)6 * windows * groups >= ((uint64_t)1 << 31)) return refuse("6 W G target segments must stay below 2^31");
    if (W) *W = windows;
    if (G) *G = groups;
    return SEPAIHRD_OK;
}

int sepaihrd_ensemble_predictive_targets(sepaihrd_ctx* ctx, const double* theta, int S, int R, uint64_t seed, const double* dispersion,
                                         const double* observed, const int32_t* age_group, int window, int origin, const double* probs, int n_probs,
                                         const double* levels, int n_levels, double* target_quantiles, double* pit, double* target_scores,
                                         double* summary, double* target_obs, double* target_draws, double* means, double* draws, double* k_used,
                                         int32_t* status, int32_t* n_valid, int32_t* exact) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    NbDispersion nb = ctx->disp;  // NULL: the context's, as in sepaihrd_ensemble_predictive_scores
    char msg[256] = "";
    if (dispersion) {
        const int rc = validated(ctx, sepaihrd_particle_nb_validate(dispersion, msg, (int)sizeof(msg)), msg);
        if (rc != SEPAIHRD_OK) return rc;
        for (int s = 0; s < 3; ++s) { nb.src[s] = -1; nb.fixed[s] = dispersion[s]; }
    }
    TargetRequest tr{{observed, levels, n_levels, target_scores, summary, exact}, age_group, window, origin, 0, 0, target_obs, target_draws};
    // the grouping and the windows, once the scored call's own rules hold (those keep their messages in predictive_call)
    const int Tp = ctx->dp.T - ctx->dp.runup_offset;
    if (S > 0 && theta && probs && target_quantiles &&
        sepaihrd_predictive_scores_validate(S, R, Tp, ctx->dp.n, probs, n_probs, levels, n_levels, nullptr, 0) == SEPAIHRD_OK) {
        const int rc = validated(ctx, sepaihrd_predictive_targets_validate(S, R, Tp, ctx->dp.n, age_group, window, origin, probs, n_probs, levels,
                                                                           n_levels, &tr.W, &tr.G, msg, (int)sizeof(msg)), msg);
        if (rc != SEPAIHRD_OK) return rc;
    } else {
        tr.W = tr.G = 1;  // predictive_call refuses before either is read
    }
    return predictive_call(ctx, theta, S, R, seed, &nb, probs, n_probs, target_quantiles, pit, means, draws, k_used, status, n_valid, nullptr, &tr);
}

int sepaihrd_predictive_timing(const sepaihrd_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SEPAIHRD_E_INVALID_ARG;
    for (int i = 0; i < 3; ++i) ms[i] = ctx->pred_ms[i];
    return SEPAIHRD_OK;
}

int sepaihrd_ensemble_stochastic(sepaihrd_ctx* ctx, const double* theta, int S, int R, int steps_per_interval, uint64_t seed,
                                 const double* probs, int n_probs, int keep, double* quantiles, double* extinct, double* model_values,
                                 double* traj, double* final_state, int32_t* status, int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    const char* const who = "ensemble_stochastic";
    int rc = ensemble_preflight(ctx, who, S > 0 && theta && probs && quantiles, "need S > 0, theta, probs (1..1024) and quantiles",
                                CHECK_PENDING, probs, n_probs);
    if (rc != SEPAIHRD_OK) return rc;
    const DevProblem& dp = ctx->dp;
    const int Tp = dp.T - dp.runup_offset;
    char msg[256] = "";
    rc = validated(ctx, sepaihrd_stochastic_validate(S, R, steps_per_interval, keep, dp.T, Tp, dp.n, probs, n_probs, msg, (int)sizeof(msg)), msg);
    if (rc != SEPAIHRD_OK) return rc;
    if (keep > 0 && !traj) return refuse(ctx, who, "keep > 0 needs traj", SEPAIHRD_E_INVALID_ARG);
    if (ctx->precision != SEPAIHRD_PRECISION_F64)
        return refuse(ctx, who, "the stochastic model is built for fp64 contexts (set precision F64)", SEPAIHRD_E_UNSUPPORTED);
    if (dp.n > 16 || dp.lpc > 16) return refuse(ctx, who, "built for at most 16 age classes", SEPAIHRD_E_UNSUPPORTED);
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    // sizes
    const size_t N = (size_t)S * (size_t)R;
    const SegmentPlan plan = plan_segments(N);  // a segment: the S R replicates of one (series, time, age)
    const size_t N_pad = plan.pad;
    const int W = sepaihrd_stochastic_values_width(dp.n, dp.nb, dp.nk);
    const size_t cells = (size_t)3 * Tp * dp.n;
    const size_t n_q = (size_t)6 * n_probs * Tp * dp.n;
    const size_t n_vals = 2 * cells * N_pad;
    const size_t n_scratch = sort_scratch_doubles(plan, n_vals);
    const size_t n_values = (size_t)S * W;
    const size_t n_traj = (traj && keep > 0) ? (size_t)S * keep * dp.T * NUM_COMP * dp.n : 0;
    const size_t n_final = final_state ? N * NUM_COMP * dp.n : 0;
    // the rule of sepaihrd_ensemble_predictive: what is allocated below must fit the device's memory (the segment table
    // dominates)
    const size_t need_bytes = sizeof(double) * ((size_t)S * ctx->P + n_vals + n_scratch + n_q + n_values + n_traj + n_final + (size_t)n_probs) +
                              sizeof(int32_t) * (2 * (size_t)S + 2);
    rc = require_device_memory(ctx, need_bytes,
                               "ensemble_stochastic: the segment table of S x R = " + std::to_string(N) + " replicates and the outputs asked for need",
                               "split the samples or the replicates over several calls");
    if (rc != SEPAIHRD_OK) return rc;
    // buffers and events of this call alone
    CallScratch sc(3);
    double *d_theta = nullptr, *d_vals = nullptr, *d_scratch = nullptr, *d_probs = nullptr, *d_q = nullptr, *d_values = nullptr, *d_traj = nullptr,
           *d_final = nullptr;
    int32_t *d_counts = nullptr, *d_status = nullptr, *d_extinct = nullptr;
    if (!sc.alloc(&d_theta, (size_t)S * ctx->P) || !sc.alloc(&d_vals, n_vals) || !sc.alloc(&d_scratch, n_scratch) ||
        !sc.alloc(&d_probs, (size_t)n_probs) || !sc.alloc(&d_q, n_q) || !sc.alloc(&d_values, n_values) || !sc.alloc(&d_traj, n_traj) ||
        !sc.alloc(&d_final, n_final) || !sc.alloc(&d_counts, 2) || !sc.alloc(&d_status, (size_t)S) || !sc.alloc(&d_extinct, (size_t)S))
        return refuse(ctx, who, "device allocation failed", SEPAIHRD_E_HIP);
    for (Event& e : sc.ev) HIP_TRY(hipEventCreate(&e), ctx, return SEPAIHRD_E_HIP);
    // uploads
    HIP_TRY(hipMemcpy(d_theta, theta, (size_t)S * ctx->P * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(d_probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    // launches
    StochEpiArgs a{};
    a.S = S; a.R = R; a.N_pad = (int)N_pad;
    a.m = steps_per_interval; a.keep = n_traj ? keep : 0; a.W = W;
    a.seed = seed;
    a.theta = d_theta; a.values = d_values; a.status = d_status; a.counts = d_counts; a.extinct_count = d_extinct;
    a.vals = d_vals; a.traj = n_traj ? d_traj : nullptr; a.final_state = final_state ? d_final : nullptr;
    if (launch_stoch_epi_decode(dp, a, nullptr) != 0) return refuse(ctx, who, "decode kernel launch failed", SEPAIHRD_E_HIP);
    (void)hipEventRecord(sc.ev[0], nullptr);
    if (launch_stoch_epi_steps(dp, a, nullptr) != 0) return refuse(ctx, who, "step kernel launch failed", SEPAIHRD_E_HIP);
    (void)hipEventRecord(sc.ev[1], nullptr);
    PredictiveArgs pa{};
    pa.S = S; pa.R = R; pa.N_pad = (int)N_pad;
    pa.lpc = dp.lpc; pa.n = dp.n; pa.T = dp.T; pa.Tp = Tp; pa.runup_offset = dp.runup_offset;
    pa.seed = seed;
    pa.wstatus = d_status;
    pa.vals = d_vals;
    pa.n_probs = n_probs; pa.probs = d_probs; pa.q_out = d_q; pa.counts = d_counts;
    pa.sort_scratch = plan.in_lds ? nullptr : d_scratch;
    pa.sort_scratch_doubles = n_scratch;
    if (launch_predictive_quantiles(pa, nullptr) != 0) return refuse(ctx, who, "quantile launch failed", SEPAIHRD_E_HIP);
    (void)hipEventRecord(sc.ev[2], nullptr);
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    elapsed_ms(sc.ev, ctx->stoch_ms, 2);
    // fetches
    ResultFetch res;
    std::vector<int32_t> h_status((size_t)S), h_extinct((size_t)S);
    res.fetch(quantiles, d_q, n_q * sizeof(double));
    res.fetch(model_values, d_values, n_values * sizeof(double));
    res.fetch(traj, d_traj, n_traj * sizeof(double));
    res.fetch(final_state, d_final, n_final * sizeof(double));
    res.fetch(h_status.data(), d_status, (size_t)S * sizeof(int32_t));
    res.fetch(h_extinct.data(), d_extinct, (size_t)S * sizeof(int32_t));
    res.fetch(n_valid, d_counts, sizeof(int32_t));
    if (!res.ok()) return refuse(ctx, who, "copy of the results failed", SEPAIHRD_E_HIP);
    if (status) std::copy(h_status.begin(), h_status.end(), status);
    if (extinct)
        for (int s = 0; s < S; ++s)
            extinct[s] = h_status[(size_t)s] == 0 ? (double)h_extinct[(size_t)s] / (double)R : std::numeric_limits<double>::quiet_NaN();
    return SEPAIHRD_OK;
}

int sepaihrd_stochastic_timing(const sepaihrd_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SEPAIHRD_E_INVALID_ARG;
    for (int i = 0; i < 2; ++i) ms[i] = ctx->stoch_ms[i];
    return SEPAIHRD_OK;
}

}  // extern "C"

namespace {

// The dispersion of a sepaihrd_particle_loglik_nb / _wide_nb call after sepaihrd_particle_nb_validate: whether some series is
// dispersed, and then the row constants G [T_pos] from the context's copy of the observation grid.
struct NbPlan {
    bool some = false;
    sepaihrd_particle::Dispersion d{};
    std::vector<double> G;
};
void nb_row_constants_of(const sepaihrd_ctx* ctx, const sepaihrd_particle::Dispersion& d, double* G) {
    const DevProblem& dp = ctx->dp;
    const double* grid = ctx->host_grid.data();  // [T][lpc][4]: {obs_H, obs_ICU, obs_D, times[k + 1]}
    sepaihrd_particle::nb_row_constants(d, dp.n, dp.T - dp.runup_offset,
                                        [&](int series, int t, int age) { return grid[((size_t)(dp.runup_offset + t) * dp.lpc + age) * 4 + series]; }, G);
}
// SEPAIHRD_OK, or the validator's refusal as the context's last error
int nb_plan(sepaihrd_ctx* ctx, const double* dispersion, NbPlan& plan) {
    char msg[256] = "";
    const int rc = validated(ctx, sepaihrd_particle_nb_validate(dispersion, msg, (int)sizeof(msg)), msg);
    if (rc != SEPAIHRD_OK) return rc;
    plan.d = sepaihrd_particle::Dispersion{dispersion[0], dispersion[1], dispersion[2]};
    plan.some = sepaihrd_particle::any_dispersed(plan.d);
    if (plan.some) {
        plan.G.resize((size_t)(ctx->dp.T - ctx->dp.runup_offset));
        nb_row_constants_of(ctx, plan.d, plan.G.data());
    }
    return SEPAIHRD_OK;
}

// The four forms of the particle-filter call, one body: the LDS kernel (sepaihrd_particle_loglik, _nb) or, with `wide`, the
// launches over particles in device memory (sepaihrd_particle_loglik_wide, _wide_nb; theta_chunk is theirs alone); dispersion
// NULL for the Poisson forms.  With no dispersed series no table is formed and the Poisson kernels run, launch for launch.
// Each form keeps its own validator, memory rule and timing slot.  A further form, sepaihrd_particle_filter_states (`states`
// given; wide): the wide launches with every output row a segment and the row summaries of DESIGN.md section 6n between them.
struct StatesOutputs {
    const double* probs;
    int n_probs;
    double *state_mean, *state_quantiles;
};
int particle_loglik_call(sepaihrd_ctx* ctx, const char* who, bool wide, int theta_chunk, const double* dispersion, const double* theta, int B, int J,
                         int steps_per_interval, uint64_t seed, double* loglik, double* increments, double* ess, double* final_state,
                         double* model_values, int32_t* status, int32_t* n_valid, const StatesOutputs* states = nullptr) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (states != nullptr && (!theta || !loglik || !states->state_mean))
        return refuse(ctx, who, "need theta, loglik and state_mean", SEPAIHRD_E_INVALID_ARG);
    if (!theta || !loglik) return refuse(ctx, who, "need theta and loglik", SEPAIHRD_E_INVALID_ARG);
    int rc = ensemble_preflight(ctx, who, true, nullptr, CHECK_PENDING);
    if (rc != SEPAIHRD_OK) return rc;
    const DevProblem& dp = ctx->dp;
    const int Tp = dp.T - dp.runup_offset;
    if (dp.n > 16 || dp.lpc > 16) return refuse(ctx, who, "built for at most 16 age classes", SEPAIHRD_E_UNSUPPORTED);
    char msg[256] = "";
    rc = validated(ctx,
                   states ? sepaihrd_particle_states_validate(B, J, steps_per_interval, theta_chunk, dp.T, Tp, dp.n, states->probs, states->n_probs, msg,
                                                              (int)sizeof(msg))
                   : wide ? sepaihrd_particle_wide_validate(B, J, steps_per_interval, theta_chunk, dp.T, Tp, dp.n, msg, (int)sizeof(msg))
                          : sepaihrd_particle_validate(B, J, steps_per_interval, dp.T, Tp, dp.n, msg, (int)sizeof(msg)),
                   msg);
    if (rc != SEPAIHRD_OK) return rc;
    if (states != nullptr && states->state_quantiles != nullptr && states->n_probs == 0)
        return refuse(ctx, who, "state_quantiles needs n_probs > 0", SEPAIHRD_E_INVALID_ARG);
    NbPlan nb;
    if (dispersion != nullptr) {
        rc = nb_plan(ctx, dispersion, nb);
        if (rc != SEPAIHRD_OK) return rc;
    }
    if (ctx->precision != SEPAIHRD_PRECISION_F64)
        return refuse(ctx, who, "the stochastic model is built for fp64 contexts (set precision F64)", SEPAIHRD_E_UNSUPPORTED);
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    // sizes
    const int W = sepaihrd_stochastic_values_width(dp.n, dp.nb, dp.nk);
    const size_t n_values = (size_t)B * W, n_rows = (size_t)B * Tp;
    const size_t n_final = final_state ? (size_t)B * J * NUM_COMP * dp.n : 0;
    const size_t chunk = states ? particle_states_chunk(dp.lpc, dp.n, J, B, theta_chunk) : wide ? particle_wide_chunk(dp.lpc, J, B, theta_chunk) : 0;
    const size_t scratch_bytes = wide ? particle_wide_scratch_bytes(dp.lpc, J, chunk) : 0;  // the particles: the LDS form keeps them on chip
    // the summaries: the row table of a chunk, the probabilities and the two outputs
    const size_t n_table = states ? particle_states_table_doubles(dp.n, J, chunk) : 0;
    const size_t n_mean = states ? (size_t)B * dp.T * NUM_COMP * (dp.n + 1) : 0;
    const size_t n_quant = states && states->state_quantiles ? n_mean * (size_t)states->n_probs : 0;
    const size_t n_probs = states ? (size_t)states->n_probs : 0;
    const size_t need_bytes = scratch_bytes +
                              sizeof(double) * ((size_t)B * ctx->P + n_values + (size_t)B + 2 * n_rows + n_final + nb.G.size() + n_table + n_mean + n_quant +
                                                n_probs) +
                              sizeof(int32_t) * ((size_t)B + 2);
    const std::string what =
        states ? "particle_filter_states: the particles and the row table of " + std::to_string(chunk) +
                     " parameter vectors at a time, the model values of B = " + std::to_string(B) + " and the outputs asked for need"
        : wide ? "particle_loglik_wide: the particles of " + std::to_string(chunk) + " parameter vectors at a time, the model values of B = " +
                     std::to_string(B) + " and the outputs asked for need"
               : "particle_loglik: the model values of B = " + std::to_string(B) + " parameter vectors and the outputs asked for need";
    rc = require_device_memory(ctx, need_bytes, what,
                               wide ? "lower theta_chunk or split the parameter vectors over several calls" : "split the parameter vectors over several calls");
    if (rc != SEPAIHRD_OK) return rc;
    // buffers and events of this call alone
    CallScratch sc(3);
    double *d_theta = nullptr, *d_values = nullptr, *d_ll = nullptr, *d_inc = nullptr, *d_ess = nullptr, *d_final = nullptr, *d_scratch = nullptr,
           *d_G = nullptr;
    int32_t *d_counts = nullptr, *d_status = nullptr;
    if (!sc.alloc(&d_theta, (size_t)B * ctx->P) || !sc.alloc(&d_values, n_values) || !sc.alloc(&d_ll, (size_t)B) ||
        !sc.alloc(&d_inc, increments ? n_rows : 0) || !sc.alloc(&d_ess, ess ? n_rows : 0) || !sc.alloc(&d_final, n_final) ||
        !sc.alloc(&d_counts, 2) || !sc.alloc(&d_status, (size_t)B) ||
        (wide && !sc.alloc(&d_scratch, (scratch_bytes + sizeof(double) - 1) / sizeof(double))) || !sc.alloc(&d_G, nb.G.size()))
        return refuse(ctx, who, "device allocation failed", SEPAIHRD_E_HIP);
    double *d_table = nullptr, *d_mean = nullptr, *d_quant = nullptr, *d_probs = nullptr;
    if (!sc.alloc(&d_table, n_table) || !sc.alloc(&d_mean, n_mean) || !sc.alloc(&d_quant, n_quant) || !sc.alloc(&d_probs, n_probs))
        return refuse(ctx, who, "device allocation failed", SEPAIHRD_E_HIP);
    // a pair of events around every row's summary of the first chunk, where the grid has few enough rows: the third entry of the
    // timing
    const size_t n_summaries = states ? (size_t)dp.T : 0;
    if (n_summaries > 0 && n_summaries <= 1024) sc.ev.resize(3 + 2 * n_summaries);
    for (Event& e : sc.ev) HIP_TRY(hipEventCreate(&e), ctx, return SEPAIHRD_E_HIP);
    std::vector<void*> summary_ev;
    for (size_t i = 3; i < sc.ev.size(); ++i) summary_ev.push_back(static_cast<hipEvent_t>(sc.ev[i]));
    HIP_TRY(hipMemcpy(d_theta, theta, (size_t)B * ctx->P * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    if (n_probs) HIP_TRY(hipMemcpy(d_probs, states->probs, n_probs * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    if (nb.some) HIP_TRY(hipMemcpy(d_G, nb.G.data(), nb.G.size() * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    // launches
    StochEpiArgs da{};
    da.S = B; da.R = J; da.W = W;
    da.theta = d_theta; da.values = d_values; da.status = d_status; da.counts = d_counts;
    (void)hipEventRecord(sc.ev[0], nullptr);
    if (launch_stoch_epi_decode(dp, da, nullptr) != 0) return refuse(ctx, who, "decode kernel launch failed", SEPAIHRD_E_HIP);
    (void)hipEventRecord(sc.ev[1], nullptr);
    ParticleWideArgs a{};
    a.B = B; a.J = J; a.m = steps_per_interval; a.W = W;
    a.seed = seed;
    a.values = d_values; a.status = d_status; a.loglik = d_ll;
    a.increments = increments ? d_inc : nullptr; a.ess = ess ? d_ess : nullptr; a.final_state = final_state ? d_final : nullptr;
    if (nb.some) {
        a.k_H = nb.d.k_H; a.k_ICU = nb.d.k_ICU; a.k_D = nb.d.k_D;
        a.row_const = d_G;
    }
    a.chunk = chunk; a.scratch = d_scratch; a.host_grid = ctx->host_grid.data();  // read by the wide launch alone
    ParticleStatesArgs sa{};
    if (states != nullptr) {
        sa.n_probs = states->n_probs; sa.probs = d_probs; sa.table = d_table;
        sa.state_mean = d_mean; sa.state_quantiles = states->state_quantiles ? d_quant : nullptr;
        sa.ev = summary_ev.empty() ? nullptr : summary_ev.data(); sa.n_ev = summary_ev.size();
        a.states = &sa;
    }
    const int lrc = wide      ? launch_particle_filter_wide(dp, a, nullptr)
                    : nb.some ? launch_particle_filter_nb(dp, a, nullptr)
                              : launch_particle_filter(dp, a, nullptr);
    (void)hipEventRecord(sc.ev[2], nullptr);
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    if (lrc != 0) return refuse(ctx, who, wide ? "filter launch failed" : "filter kernel launch failed", SEPAIHRD_E_HIP);
    elapsed_ms(sc.ev, states ? ctx->particle_states_ms : wide ? ctx->particle_wide_ms : ctx->particle_ms, 2);
    if (states != nullptr) {  // the summaries' share of the first chunk's launches; NaN where the grid has too many rows for the events
        double summary = sa.used_ev == 2 * n_summaries && n_summaries > 0 ? 0.0 : std::numeric_limits<double>::quiet_NaN();
        for (size_t i = 0; i + 1 < sa.used_ev; i += 2) {
            float t = 0.0f;
            (void)hipEventElapsedTime(&t, static_cast<hipEvent_t>(summary_ev[i]), static_cast<hipEvent_t>(summary_ev[i + 1]));
            summary += t;
        }
        ctx->particle_states_ms[2] = summary;
    }
    // fetches
    ResultFetch res;
    if (states != nullptr) {
        res.fetch(states->state_mean, d_mean, n_mean * sizeof(double));
        res.fetch(states->state_quantiles, d_quant, n_quant * sizeof(double));
    }
    res.fetch(loglik, d_ll, (size_t)B * sizeof(double));
    res.fetch(increments, d_inc, n_rows * sizeof(double));
    res.fetch(ess, d_ess, n_rows * sizeof(double));
    res.fetch(final_state, d_final, n_final * sizeof(double));
    res.fetch(model_values, d_values, n_values * sizeof(double));
    res.fetch(status, d_status, (size_t)B * sizeof(int32_t));
    res.fetch(n_valid, d_counts, sizeof(int32_t));
    if (!res.ok()) return refuse(ctx, who, "copy of the results failed", SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

}  // namespace

extern "C" {

int sepaihrd_particle_loglik(sepaihrd_ctx* ctx, const double* theta, int B, int J, int steps_per_interval, uint64_t seed, double* loglik,
                             double* increments, double* ess, double* final_state, double* model_values, int32_t* status, int32_t* n_valid) {
    return particle_loglik_call(ctx, "particle_loglik", false, 0, nullptr, theta, B, J, steps_per_interval, seed, loglik, increments, ess, final_state,
                                model_values, status, n_valid);
}

int sepaihrd_particle_loglik_nb(sepaihrd_ctx* ctx, const double* theta, int B, int J, int steps_per_interval, uint64_t seed,
                                const double dispersion[3], double* loglik, double* increments, double* ess, double* final_state,
                                double* model_values, int32_t* status, int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (!dispersion) return refuse(ctx, "particle_loglik_nb", "need dispersion (three entries: k_H, k_ICU, k_D)", SEPAIHRD_E_INVALID_ARG);
    return particle_loglik_call(ctx, "particle_loglik_nb", false, 0, dispersion, theta, B, J, steps_per_interval, seed, loglik, increments, ess,
                                final_state, model_values, status, n_valid);
}

int sepaihrd_particle_nb_row_constants(const sepaihrd_ctx* ctx, const double dispersion[3], double* G) {
    if (!ctx || !G || sepaihrd_particle_nb_validate(dispersion, nullptr, 0) != SEPAIHRD_OK || ctx->host_grid.empty()) return SEPAIHRD_E_INVALID_ARG;
    nb_row_constants_of(ctx, sepaihrd_particle::Dispersion{dispersion[0], dispersion[1], dispersion[2]}, G);
    return SEPAIHRD_OK;
}

int sepaihrd_particle_timing(const sepaihrd_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SEPAIHRD_E_INVALID_ARG;
    for (int i = 0; i < 2; ++i) ms[i] = ctx->particle_ms[i];
    return SEPAIHRD_OK;
}

int sepaihrd_particle_loglik_wide(sepaihrd_ctx* ctx, const double* theta, int B, int J, int steps_per_interval, uint64_t seed, int theta_chunk,
                                  double* loglik, double* increments, double* ess, double* final_state, double* model_values, int32_t* status,
                                  int32_t* n_valid) {
    return particle_loglik_call(ctx, "particle_loglik_wide", true, theta_chunk, nullptr, theta, B, J, steps_per_interval, seed, loglik, increments, ess,
                                final_state, model_values, status, n_valid);
}

int sepaihrd_particle_loglik_wide_nb(sepaihrd_ctx* ctx, const double* theta, int B, int J, int steps_per_interval, uint64_t seed,
                                     const double dispersion[3], int theta_chunk, double* loglik, double* increments, double* ess,
                                     double* final_state, double* model_values, int32_t* status, int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (!dispersion) return refuse(ctx, "particle_loglik_wide_nb", "need dispersion (three entries: k_H, k_ICU, k_D)", SEPAIHRD_E_INVALID_ARG);
    return particle_loglik_call(ctx, "particle_loglik_wide_nb", true, theta_chunk, dispersion, theta, B, J, steps_per_interval, seed, loglik,
                                increments, ess, final_state, model_values, status, n_valid);
}

int sepaihrd_particle_wide_timing(const sepaihrd_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SEPAIHRD_E_INVALID_ARG;
    for (int i = 0; i < 2; ++i) ms[i] = ctx->particle_wide_ms[i];
    return SEPAIHRD_OK;
}

int sepaihrd_particle_filter_states(sepaihrd_ctx* ctx, const double* theta, int B, int J, int steps_per_interval, uint64_t seed, int theta_chunk,
                                    const double* dispersion, const double* probs, int n_probs, double* loglik, double* increments, double* ess,
                                    double* state_mean, double* state_quantiles, double* model_values, int32_t* status, int32_t* n_valid) {
    const StatesOutputs states{probs, n_probs, state_mean, state_quantiles};
    return particle_loglik_call(ctx, "particle_filter_states", true, theta_chunk, dispersion, theta, B, J, steps_per_interval, seed, loglik, increments,
                                ess, nullptr, model_values, status, n_valid, &states);
}

int sepaihrd_particle_states_timing(const sepaihrd_ctx* ctx, double* ms) {
    if (!ctx || !ms) return SEPAIHRD_E_INVALID_ARG;
    for (int i = 0; i < 3; ++i) ms[i] = ctx->particle_states_ms[i];
    return SEPAIHRD_OK;
}

int sepaihrd_scenario_ensemble(sepaihrd_ctx* ctx, const double* theta, int S, const double* kappa_mult, int K, int n_kappa,
                               const double* probs, int n_probs, double* ppc_quantiles, double* sero_quantiles,
                               double* rt_quantiles, double* metrics, double* metric_summary, double* diff_quantiles,
                               int32_t* status, int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    const char* const who = "scenario_ensemble";
    int rc = ensemble_preflight(ctx, who, S > 0 && K > 0 && theta && kappa_mult && probs, "need S > 0, K > 0, theta, kappa_mult and probs (1..1024)",
                                CHECK_PROBS, probs, n_probs);
    if (rc != SEPAIHRD_OK) return rc;
    const DevProblem& dp = ctx->dp;
    if (n_kappa != dp.nk) return refuse(ctx, who, "the multiplier table must have one column per kappa value", SEPAIHRD_E_INVALID_ARG);
    for (size_t i = 0; i < (size_t)K * n_kappa; ++i)
        if (!(std::isfinite(kappa_mult[i]) && kappa_mult[i] >= 0.0))
            return refuse(ctx, who, "kappa multipliers must be finite and >= 0", SEPAIHRD_E_INVALID_ARG);
    rc = ensemble_preflight(ctx, who, true, nullptr, CHECK_PENDING | CHECK_F64);
    if (rc != SEPAIHRD_OK) return rc;
    if (dp.n > 16) return refuse(ctx, who, "the metric table needs Rt trajectories, built for at most 16 age classes", SEPAIHRD_E_UNSUPPORTED);
    rc = ensemble_preflight(ctx, who, true, nullptr, CHECK_TP);
    if (rc != SEPAIHRD_OK) return rc;
    const int Tp = dp.T - dp.runup_offset;
    // scenario k's samples are chains k S_str .. k S_str + S - 1: S_str = S rounded up to whole waves' worth of chains, so that
    // every scenario's parked increments start on a wave boundary of the workspace (the ensemble passes then read it in place)
    const size_t cpw = (size_t)(WAVE / dp.lpc);
    const size_t S_str = ((size_t)S + cpw - 1) / cpw * cpw;
    const size_t B = (size_t)(K - 1) * S_str + (size_t)S;  // the last scenario needs no padding chains
    if (B > (size_t)std::numeric_limits<int32_t>::max() / 2)
        return refuse(ctx, who, "K x S chains exceed one launch (the workspace is sized by a 32-bit chain count)", SEPAIHRD_E_INVALID_ARG);
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    // sizes
    const SegmentPlan plan = plan_segments((size_t)S);  // a segment: the S samples of one cell of one scenario
    const int S_pad = (int)plan.pad;
    const size_t chains = (B + cpw - 1) / cpw * cpw;
    const bool want_sero = sero_quantiles != nullptr;
    const int W = 12 + 4 * dp.n;
    const size_t P = (size_t)ctx->P;
    const size_t n_ppc = (size_t)6 * n_probs * Tp * dp.n;  // per scenario
    const size_t n_sero = want_sero ? (size_t)n_probs * dp.T : 0;
    const size_t n_rt = (size_t)n_probs * dp.T;
    const size_t n_q = n_ppc + n_sero + n_rt;
    const size_t n_vals = ((size_t)6 * Tp * dp.n + (want_sero ? dp.T : 0) + dp.T) * S_pad;
    const size_t n_svals = (size_t)2 * K * W * S_pad;
    const size_t n_metrics = (size_t)K * S * W;
    const size_t n_summary = (size_t)K * W * (2 + n_probs), n_diff = (size_t)K * W * n_probs;
    const size_t n_scratch = sort_scratch_doubles(plan, std::max(n_vals, n_svals));
    // K x S within one launch: the device buffers below plus the likelihood workspace must fit the device's memory
    // (the trajectories dominate: K S T 11 n doubles)
    const size_t need_bytes =
        sizeof(double) * (chains * P + chains + n_vals + chains * dp.T * NUM_COMP * dp.n + (size_t)K * n_q + n_metrics + n_scratch +
                          (size_t)K * n_kappa + n_svals + n_summary + n_diff + (size_t)n_probs) +
        sizeof(double) * (workspace_cum_doubles(dp, chains) + workspace_rows_doubles(dp, chains)) + sizeof(int32_t) * (chains + 3 * (size_t)K);
    rc = require_device_memory(ctx, need_bytes, "scenario_ensemble: K x S = " + std::to_string((size_t)K * S) + " runs need",
                               "split the scenarios or the samples over several calls");
    if (rc != SEPAIHRD_OK) return rc;
    // buffers: they stay with the context, the ones sepaihrd_ensemble_quantiles uses in the same roles
    rc = ensure_workspace(ctx, chains);
    if (rc != SEPAIHRD_OK) return rc;
    double *d_theta = nullptr, *d_ll = nullptr, *d_mult = nullptr, *d_traj = nullptr, *d_vals = nullptr, *d_svals = nullptr,
           *d_probs = nullptr, *d_q = nullptr, *d_metrics = nullptr, *d_summary = nullptr, *d_scratch = nullptr;
    int32_t *d_nv = nullptr, *d_counts = nullptr;
    auto& slots = ctx->ens;
    if (!slots.get(SLOT_THETA, &d_theta, chains * P) || !slots.get(SLOT_LOGLIK, &d_ll, chains) || !slots.get(SLOT_VALS, &d_vals, n_vals) ||
        !slots.get(SLOT_TRAJ, &d_traj, chains * dp.T * NUM_COMP * dp.n) || !slots.get(SLOT_PROBS, &d_probs, (size_t)n_probs) ||
        !slots.get(SLOT_QUANTILES, &d_q, (size_t)K * n_q) || !slots.get(SLOT_N_VALID, &d_nv, (size_t)K) ||
        !slots.get(SLOT_METRICS, &d_metrics, n_metrics) || !slots.get(SLOT_SORT_SCRATCH, &d_scratch, n_scratch) ||
        !slots.get(SLOT_KAPPA_MULT, &d_mult, (size_t)K * n_kappa) || !slots.get(SLOT_SCEN_VALS, &d_svals, n_svals) ||
        !slots.get(SLOT_SCEN_SUMMARY, &d_summary, n_summary + n_diff) || !slots.get(SLOT_SCEN_COUNTS, &d_counts, (size_t)2 * K))
        return refuse(ctx, who, "device allocation failed", SEPAIHRD_E_HIP);
    // uploads.  Every scenario integrates the same samples; the padding chains repeat the scenario's first sample and are never read
    std::vector<double> h_theta(B * P);
    for (size_t c = 0; c < B; ++c) {
        const size_t s = c % S_str;
        std::memcpy(&h_theta[c * P], theta + (s < (size_t)S ? s : 0) * P, P * sizeof(double));
    }
    HIP_TRY(hipMemcpy(d_theta, h_theta.data(), B * P * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(d_mult, kappa_mult, (size_t)K * n_kappa * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(d_probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    // launches
    EvalOutputs out{d_ll, nullptr, nullptr, nullptr, nullptr, d_traj, ctx->ws_cum, ctx->ws_rows, ctx->ws_status, nullptr, 1};
    rc = fence_before(ctx, nullptr);
    if (rc != SEPAIHRD_OK) return rc;
    // the integrator scales kappa per scenario (scenario build of the kernels); the Rt and metric passes read ctx->dp, unscaled
    rc = launch_eval_for(ctx, "", d_theta, (int)B, out, d_mult, (int)S_str);
    if (rc != SEPAIHRD_OK) return rc;
    const double total_pop = total_population(ctx);
    // series, seroprevalence, Rt, metric table and their quantiles: once per scenario, on the scenario's block of chains
    for (int k = 0; k < K && rc == 0; ++k) {
        const size_t c0 = (size_t)k * S_str;
        EnsembleArgs a{};
        a.S = S; a.S_pad = S_pad; a.lpc = dp.lpc; a.n = dp.n; a.T = dp.T; a.Tp = Tp; a.runup_offset = dp.runup_offset;
        a.n_probs = n_probs;
        a.cum_stride = chains * dp.lpc;
        a.cum = ctx->ws_cum + cum_index(dp.T, c0 * dp.lpc, 0, 0);  // c0 lpc is a multiple of WAVE
        a.wstatus = ctx->ws_status + c0;
        a.traj = d_traj + c0 * dp.T * NUM_COMP * dp.n;
        a.total_pop = total_pop;
        a.vals = d_vals; a.probs = d_probs;
        a.q_out = d_q + (size_t)k * n_q;
        a.sero_out = want_sero ? a.q_out + n_ppc : nullptr;
        a.n_valid = d_nv + k;
        a.rt_out = a.q_out + n_ppc + n_sero;
        a.rt_segment0 = 6 * Tp * dp.n + (want_sero ? dp.T : 0);
        a.pb = &ctx->dp;
        a.theta = d_theta + c0 * P;
        a.metrics_out = d_metrics + (size_t)k * S * W;
        a.sort_scratch = plan.in_lds ? nullptr : d_scratch;
        a.sort_scratch_doubles = n_scratch;
        rc = launch_ensemble_summaries(a, nullptr);
    }
    if (rc == 0) {
        ScenarioArgs sa{};
        sa.K = K; sa.S = S; sa.S_pad = S_pad; sa.W = W; sa.n_probs = n_probs; sa.probs = d_probs;
        sa.metrics = d_metrics; sa.wstatus = ctx->ws_status; sa.status_stride = S_str;
        sa.vals = d_svals; sa.counts = d_counts;
        sa.summary_out = d_summary; sa.diff_out = d_summary + n_summary;
        sa.sort_scratch = plan.in_lds ? nullptr : d_scratch;
        sa.sort_scratch_doubles = n_scratch;
        rc = launch_scenario_summaries(sa, nullptr);
    }
    if (rc != 0) {
        ctx->last_error = "scenario summary launch failed";
        return SEPAIHRD_E_HIP;
    }
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    // fetches
    ResultFetch res;
    for (int k = 0; k < K; ++k) {
        const double* q = d_q + (size_t)k * n_q;
        res.fetch(ppc_quantiles ? ppc_quantiles + (size_t)k * n_ppc : nullptr, q, n_ppc * sizeof(double));
        res.fetch(want_sero ? sero_quantiles + (size_t)k * n_sero : nullptr, q + n_ppc, n_sero * sizeof(double));
        res.fetch(rt_quantiles ? rt_quantiles + (size_t)k * n_rt : nullptr, q + n_ppc + n_sero, n_rt * sizeof(double));
        res.fetch(status ? status + (size_t)k * S : nullptr, ctx->ws_status + (size_t)k * S_str, (size_t)S * sizeof(int32_t));
    }
    res.fetch(metrics, d_metrics, n_metrics * sizeof(double));
    res.fetch(metric_summary, d_summary, n_summary * sizeof(double));
    res.fetch(diff_quantiles, d_summary + n_summary, n_diff * sizeof(double));
    res.fetch(n_valid, d_nv, (size_t)K * sizeof(int32_t));
    if (!res.ok()) return refuse(ctx, who, "copy of the results failed", SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_apply_constraints(const sepaihrd_ctx* ctx, int mode, const double* in, int B, double* out) {
    if (!ctx || !in || !out || B < 0) return SEPAIHRD_E_INVALID_ARG;
    const int P = ctx->P;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < P; ++p)
            out[(size_t)b * P + p] = constrain(in[(size_t)b * P + p], ctx->lower[p], ctx->upper[p], ctx->has_bounds[p],
                                               mode == SEPAIHRD_CONSTRAINT_CLAMP ? 0 : 1);
    return SEPAIHRD_OK;
}

int sepaihrd_get_kernel_info_for_batch(sepaihrd_ctx* ctx, int32_t batch_chains, sepaihrd_kernel_info* info) {
    if (!ctx || !info) return SEPAIHRD_E_INVALID_ARG;
    std::memset(info, 0, sizeof(*info));
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    LaunchInfo li{};
    // a dispersed context: the pass that takes the Poisson pass's place behind whichever integrator form parks the increments
    const int rc = nb_any_dispersed(ctx->disp) && ctx->precision != SEPAIHRD_PRECISION_F32 ? kernel_info_nb_pass(ctx->dp, &li)
                   : ctx->precision == SEPAIHRD_PRECISION_F32 ? kernel_info_f32(ctx->dp, ctx->solver, &li)
                   : ctx->arith == SEPAIHRD_ARITH_FMA       ? kernel_info_fma(ctx->dp, ctx->solver, batch_chains, &li)
                                                            : kernel_info_strict(ctx->dp, ctx->solver, batch_chains, &li);
    if (rc != 0) { ctx->last_error = "kernel_info failed"; return SEPAIHRD_E_HIP; }
    info->lanes_per_chain = li.lanes_per_chain;
    info->chains_per_wave = WAVE / li.lanes_per_chain;
    info->block_threads = WAVE;
    info->vgprs = li.vgprs; info->sgprs = li.sgprs; info->scratch_bytes = li.scratch;
    info->lds_bytes = li.lds_static + li.lds_dynamic;
    info->max_blocks_per_cu = li.max_blocks_per_cu;
    info->likelihood_form = li.likelihood_form;
    info->phase_pass_applied = ctx->precision == SEPAIHRD_PRECISION_F32 ? 0  // the fp32-state kernel does not go through the pass
                               : ctx->arith == SEPAIHRD_ARITH_FMA       ? phase_pass_applied_fma()
                                                                        : phase_pass_applied_strict();
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device), ctx, return SEPAIHRD_E_HIP);
    info->num_cus = prop.multiProcessorCount;
    std::snprintf(info->kernel_name, sizeof(info->kernel_name), "%s lpc=%d solver=%d", li.name, li.lanes_per_chain,
                  ctx->solver);
    std::snprintf(info->device_name, sizeof(info->device_name), "%s (%s)", prop.name, prop.gcnArchName);
    return SEPAIHRD_OK;
}

int sepaihrd_get_kernel_info(sepaihrd_ctx* ctx, sepaihrd_kernel_info* info) {
    return sepaihrd_get_kernel_info_for_batch(ctx, 0, info);
}

// The device's log / exp (csrc/sepaihrd_rng.inc) restate ONE libm build.  Before a sampler lets the device draw, they are
// evaluated on fixed arguments and compared, bit for bit, with the std::log / std::exp of THIS process.
int sepaihrd_device_libm_check(sepaihrd_ctx* ctx, int32_t* n_log_diff, int32_t* n_exp_diff) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    return device_libm_check(ctx->device, ctx->last_error, ctx->libm_log_diff, ctx->libm_exp_diff, n_log_diff, n_exp_diff);
}

int sepaihrd_device_log_values(sepaihrd_ctx* ctx, const double* x, int32_t n, double* out) {
    if (!ctx || n < 0 || (n > 0 && (!x || !out))) return SEPAIHRD_E_INVALID_ARG;
    if (n == 0) return SEPAIHRD_OK;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    DeviceBuf buf;
    double* d = nullptr;
    ALLOC_TRY(buf.get(&d, 2 * (size_t)n), ctx, return SEPAIHRD_E_HIP);
    const bool ok = hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                    poisson_log_values(d, n, d + n, nullptr) == 0 &&
                    hipMemcpy(out, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) { ctx->last_error = "device_log_values: launch or copy failed"; return SEPAIHRD_E_HIP; }
    return SEPAIHRD_OK;
}

int sepaihrd_chain_diagnostics(sepaihrd_ctx* ctx, const double* samples, const double* values, int C, int N, int P, double* out,
                               int32_t* max_lag) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (!samples || !out) { ctx->last_error = "chain_diagnostics: samples and out are required"; return SEPAIHRD_E_INVALID_ARG; }
    int rc = diag_check_shape(ctx, "chain_diagnostics", C, N, P);
    if (rc != SEPAIHRD_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    if (!ctx->own_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking), ctx, return SEPAIHRD_E_HIP);
    const size_t CN = (size_t)C * N;
    DeviceBuf buf;
    double* d = nullptr;
    ALLOC_TRY(buf.get(&d, CN * ((size_t)P + (values ? 1 : 0))), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpyAsync(d, samples, CN * P * sizeof(double), hipMemcpyHostToDevice, ctx->own_stream), ctx, return SEPAIHRD_E_HIP);
    if (values)
        HIP_TRY(hipMemcpyAsync(d + CN * P, values, CN * sizeof(double), hipMemcpyHostToDevice, ctx->own_stream), ctx, return SEPAIHRD_E_HIP);
    DiagInput in{};
    in.samples = d;
    in.chain_stride = (size_t)N * P;
    in.sample_stride = (size_t)P;
    in.P = P;
    in.values = values ? d + CN * P : nullptr;
    in.value_chain_stride = (size_t)N;
    in.C = C;
    in.N = N;
    return diag_run(ctx, "chain_diagnostics", in, out, max_lag, ctx->own_stream);
}

// ------------------------------------------------------------------ summary records across devices
// The one exchange of the path: after sampling, every device gets the fixed-width per-chain records of ALL chains so that
// it can form the ensemble quantiles the reference computes serially (ResultAggregator.cpp:35-172).  One process drives
// several devices here (one context / host thread per device, as optimizeChainGroupsOnDevice runs them), so the
// collective is RCCL's single-process form: ncclCommInitAll over the contexts' devices and one ncclAllGather per device
// inside a group call -- xGMI is point to point, each device's block goes to its peers directly.  RCCL is loaded at first
// use (dlopen of librccl.so.1: the library has no link-time dependency on it, and a process that already carries a copy
// -- PyTorch's -- shares it); without it, or when two contexts share a device (RCCL wants one rank per device), the
// records are staged through the host.
double* sepaihrd_records_buffer(sepaihrd_ctx* ctx, int which, size_t doubles) {
    if (!ctx || which < 0 || which > 1) return nullptr;
    DeviceBuf& buf = ctx->rec_buf[which];
    if (doubles * sizeof(double) > buf.cap) {
        if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
        if (!buf.reserve(doubles * sizeof(double))) ctx->last_error = "records_buffer: device allocation failed";
    }
    return buf.as<double>();
}

int sepaihrd_read_records(sepaihrd_ctx* ctx, int which, double* out, size_t doubles) {
    if (!ctx || which < 0 || which > 1 || !out || doubles * sizeof(double) > ctx->rec_buf[which].cap) return SEPAIHRD_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(out, ctx->rec_buf[which].p, doubles * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_write_records(sepaihrd_ctx* ctx, int which, const double* in, size_t doubles) {
    if (!ctx || which < 0 || which > 1 || !in) return SEPAIHRD_E_INVALID_ARG;
    if (!sepaihrd_records_buffer(ctx, which, doubles)) return SEPAIHRD_E_HIP;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(ctx->rec_buf[which].p, in, doubles * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_allgather_records(sepaihrd_ctx* const* ctxs, int n, const int32_t* rows, int width, int backend, int* backend_used) {
    if (!ctxs || n <= 0 || !rows || width <= 0 || backend < SEPAIHRD_GATHER_AUTO || backend > SEPAIHRD_GATHER_HOST) return SEPAIHRD_E_INVALID_ARG;
    for (int k = 0; k < n; ++k)
        if (!ctxs[k] || rows[k] < 0) return SEPAIHRD_E_INVALID_ARG;
    sepaihrd_ctx* c0 = ctxs[0];
    size_t total = 0;
    int max_rows = 0;
    for (int k = 0; k < n; ++k) { total += (size_t)rows[k]; max_rows = std::max(max_rows, (int)rows[k]); }
    for (int k = 0; k < n; ++k)
        if ((size_t)rows[k] * width * sizeof(double) > ctxs[k]->rec_buf[0].cap) { c0->last_error = "allgather_records: a context's local table (records_buffer 0) is smaller than rows * width"; return SEPAIHRD_E_INVALID_ARG; }
    bool distinct = true;
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) distinct = distinct && ctxs[a]->device != ctxs[b]->device;
    const bool can_rccl = distinct && rccl_api().ok;
    if (backend == SEPAIHRD_GATHER_RCCL && !can_rccl) {
        c0->last_error = !distinct ? "allgather_records: RCCL wants one rank per device, two contexts share one" : "allgather_records: librccl could not be loaded";
        return SEPAIHRD_E_UNSUPPORTED;
    }
    const bool use_rccl = backend == SEPAIHRD_GATHER_RCCL || (backend == SEPAIHRD_GATHER_AUTO && can_rccl);
    if (backend_used) *backend_used = use_rccl ? SEPAIHRD_GATHER_RCCL : SEPAIHRD_GATHER_HOST;
    for (int k = 0; k < n; ++k)
        if (!sepaihrd_records_buffer(ctxs[k], 1, total * width)) { c0->last_error = "allgather_records: no room for the gathered table"; return SEPAIHRD_E_HIP; }

    if (!use_rccl) {  // host staging: every local table down, the whole table up
        std::vector<double> table(total * width);
        size_t off = 0;
        for (int k = 0; k < n; ++k) {
            HIP_TRY(hipSetDevice(ctxs[k]->device), c0, return SEPAIHRD_E_HIP);
            HIP_TRY(hipMemcpy(table.data() + off, ctxs[k]->rec_buf[0].p, (size_t)rows[k] * width * sizeof(double), hipMemcpyDeviceToHost), c0, return SEPAIHRD_E_HIP);
            off += (size_t)rows[k] * width;
        }
        for (int k = 0; k < n; ++k) {
            HIP_TRY(hipSetDevice(ctxs[k]->device), c0, return SEPAIHRD_E_HIP);
            HIP_TRY(hipMemcpy(ctxs[k]->rec_buf[1].p, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice), c0, return SEPAIHRD_E_HIP);
        }
        return SEPAIHRD_OK;
    }

    // RCCL: equal counts per rank, so every rank sends max_rows rows (its table padded) and the blocks are compacted after
    const RcclApi& rc = rccl_api();
    const size_t block = (size_t)max_rows * width;
    std::vector<int> devs(n);
    for (int k = 0; k < n; ++k) devs[k] = ctxs[k]->device;
    std::vector<void*> comms(n, nullptr);
    std::vector<double*> send(n, nullptr), recv(n, nullptr);
    std::vector<hipStream_t> streams(n, nullptr);
    int rc_code = 0;
    auto fail = [&](const char* what) {
        c0->last_error = std::string("allgather_records: ") + what + (rc_code && rc.GetErrorString ? std::string(": ") + rc.GetErrorString(rc_code) : std::string());
        for (int k = 0; k < n; ++k) {
            (void)hipSetDevice(devs[k]);
            if (send[k]) (void)hipFree(send[k]);
            if (recv[k]) (void)hipFree(recv[k]);
            if (streams[k]) (void)hipStreamDestroy(streams[k]);
            if (comms[k]) (void)rc.CommDestroy(comms[k]);
        }
        return SEPAIHRD_E_HIP;
    };
    for (int k = 0; k < n; ++k) {
        if (hipSetDevice(devs[k]) != hipSuccess || hipStreamCreateWithFlags(&streams[k], hipStreamNonBlocking) != hipSuccess ||
            hipMalloc((void**)&send[k], block * sizeof(double)) != hipSuccess || hipMalloc((void**)&recv[k], block * n * sizeof(double)) != hipSuccess ||
            hipMemsetAsync(send[k], 0, block * sizeof(double), streams[k]) != hipSuccess ||
            hipMemcpyAsync(send[k], ctxs[k]->rec_buf[0].p, (size_t)rows[k] * width * sizeof(double), hipMemcpyDeviceToDevice, streams[k]) != hipSuccess)
            return fail("staging buffers");
    }
    if ((rc_code = rc.CommInitAll(comms.data(), n, devs.data())) != 0) return fail("ncclCommInitAll");
    if ((rc_code = rc.GroupStart()) != 0) return fail("ncclGroupStart");
    for (int k = 0; k < n; ++k) {
        (void)hipSetDevice(devs[k]);
        if ((rc_code = rc.AllGather(send[k], recv[k], block, NCCL_DOUBLE, comms[k], streams[k])) != 0) { (void)rc.GroupEnd(); return fail("ncclAllGather"); }
    }
    if ((rc_code = rc.GroupEnd()) != 0) return fail("ncclGroupEnd");
    rc_code = 0;
    for (int k = 0; k < n; ++k) {  // compact: rank r's first rows[r] rows, in rank order
        (void)hipSetDevice(devs[k]);
        size_t off = 0;
        for (int r = 0; r < n; ++r) {
            if (rows[r] > 0 && hipMemcpyAsync(ctxs[k]->rec_buf[1].as<double>() + off, recv[k] + (size_t)r * block, (size_t)rows[r] * width * sizeof(double),
                                              hipMemcpyDeviceToDevice, streams[k]) != hipSuccess)
                return fail("compaction");
            off += (size_t)rows[r] * width;
        }
    }
    for (int k = 0; k < n; ++k) {
        (void)hipSetDevice(devs[k]);
        if (hipStreamSynchronize(streams[k]) != hipSuccess) return fail("stream synchronisation");
    }
    for (int k = 0; k < n; ++k) {
        (void)hipSetDevice(devs[k]);
        (void)hipFree(send[k]); (void)hipFree(recv[k]); (void)hipStreamDestroy(streams[k]); (void)rc.CommDestroy(comms[k]);
    }
    return SEPAIHRD_OK;
}

}  // extern "C"
