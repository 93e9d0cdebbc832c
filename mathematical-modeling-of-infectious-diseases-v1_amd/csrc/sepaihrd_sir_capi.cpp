// csrc/sepaihrd_sir_capi.cpp -- the age-structured SIR block of the C ABI (include/sepaihrd_hip.h, sepaihrd_sir_*).
// Host side only: validates the problem, pads the per-age tables to the lanes of a chain, uploads them once and launches
// the kernels of csrc/sepaihrd_sir.hip.  There is no CPU evaluation path.
#include "sepaihrd_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sepaihrd_device.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_mh_backend.h"
#include "sepaihrd_segments.h"
#include "sepaihrd_sir_device.h"

using namespace sepaihrd;

// the roles of the buffers sepaihrd_sir_scenario_ensemble keeps with its context
enum EnsSlot {
    SLOT_THETA, SLOT_VALS, SLOT_PROBS, SLOT_QUANTILES, SLOT_METRICS, SLOT_SCEN_VALS, SLOT_SCEN_SUMMARY, SLOT_SORT_SCRATCH, SLOT_INTS,
    SLOT_COUNTS, SLOT_N_EVENTS, SLOT_EVENTS, SLOT_COUNT
};

struct sepaihrd_sir_ctx {
    int device = 0, solver = 0, arith = 0;
    int n = 0, T = 0, P = 0;
    SirDevProblem dp{};
    // the owners below release in reverse order of declaration: events, then buffers (the context has no stream of its own)
    DeviceAllocs allocs;  // the problem's tables
    std::vector<int32_t> field;  // host copy for sepaihrd_sir_apply_constraints
    std::string last_error;
    // staging of the host-pointer entry point (grow-only) and the views ensure_staging hands out
    DeviceBuf theta_buf, loglik_buf, ints_buf, traj_buf;
    double* d_theta = nullptr;
    double* d_loglik = nullptr;
    int32_t* d_ints = nullptr;  // [3][B] status, accepted, rejected of the batch at hand
    double* d_traj = nullptr;
    // what a device-resident sampler on this context reads (sepaihrd_sir_mh_create, csrc/sepaihrd_mh_backend.h):
    // SIRParameterManager::applyConstraints as the clamp mode of the propose kernels' constrain() (the table of
    // sepaihrd_sir_constraint_bounds, constraint_mode 0; uploaded by the first sampler) -- and the libm self-check's result
    DevProblem mh_dp{};
    bool mh_dp_ready = false;
    int libm_log_diff = -1, libm_exp_diff = -1;
    int no_pending = 0;  // this context has no begin / end evaluation a sampler could collide with
    // scratch of sepaihrd_sir_scenario_ensemble by role (grow-only, reused across calls), its phase events, the device time
    // of the last call and the number of calls that reached the device
    GrowSlots<SLOT_COUNT> slots;
    Event ens_ev[4];
    double ens_ms[3] = {0.0, 0.0, 0.0};
    int64_t ens_calls = 0;
};
static_assert(sizeof(sepaihrd_sir_event) == sizeof(SirEvent) && SEPAIHRD_SIR_MAX_EVENTS == SIR_MAX_EVENTS &&
                  SEPAIHRD_SIR_EV_CONTACT == SIR_EV_CONTACT && SEPAIHRD_SIR_EV_TRANSMISSION == SIR_EV_TRANSMISSION,
              "the kernels read the C ABI's event table in place");

namespace {

int ensure_staging(sepaihrd_sir_ctx* c, size_t B, size_t traj_elems) {
    ALLOC_TRY(c->theta_buf.get(&c->d_theta, B * c->P), c, return SEPAIHRD_E_HIP);
    ALLOC_TRY(c->loglik_buf.get(&c->d_loglik, B), c, return SEPAIHRD_E_HIP);
    ALLOC_TRY(c->ints_buf.get(&c->d_ints, 3 * B), c, return SEPAIHRD_E_HIP);
    if (traj_elems) ALLOC_TRY(c->traj_buf.get(&c->d_traj, traj_elems), c, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

}  // namespace

extern "C" {

sepaihrd_sir_ctx* sepaihrd_sir_create(const sepaihrd_sir_problem* pb, int device, char* err, int errlen) {
    if (!pb) { set_err(err, errlen, "problem is NULL"); return nullptr; }
    if (pb->abi_version != SEPAIHRD_ABI_VERSION) { set_err(err, errlen, "ABI version mismatch"); return nullptr; }
    const int n = pb->n_age, T = pb->n_times, P = pb->n_params;
    if (n < 1 || n > SEPAIHRD_MAX_AGE_CLASSES) { set_err(err, errlen, "n_age out of range [1,64]"); return nullptr; }
    if (T < 1) { set_err(err, errlen, "n_times must be >= 1"); return nullptr; }
    if (P < 1) { set_err(err, errlen, "n_params must be >= 1"); return nullptr; }
    if (!pb->times || !pb->N || !pb->C || !pb->gamma || !pb->initial_state || !pb->obs || !pb->param_field || !pb->param_index) {
        set_err(err, errlen, "a required array pointer is NULL"); return nullptr;
    }
    if (pb->solver != SEPAIHRD_SOLVER_DOPRI5 && pb->solver != SEPAIHRD_SOLVER_CASH_KARP54 && pb->solver != SEPAIHRD_SOLVER_FEHLBERG78) {
        set_err(err, errlen, "unknown solver"); return nullptr;
    }
    if (pb->arith != SEPAIHRD_ARITH_STRICT && pb->arith != SEPAIHRD_ARITH_FMA) { set_err(err, errlen, "unknown arithmetic mode"); return nullptr; }
    // Simulator::run grid rules (Simulator.cpp:78-88) and its ctor checks
    for (int i = 1; i < T; ++i)
        if (!(pb->times[i] > pb->times[i - 1])) { set_err(err, errlen, "time points must be strictly increasing"); return nullptr; }
    if (pb->abs_err < 0 || pb->rel_err < 0) { set_err(err, errlen, "negative error tolerance"); return nullptr; }
    if (!(pb->dt_hint > 0)) { set_err(err, errlen, "dt_hint must be positive"); return nullptr; }
    // AgeSIRModel::validate_parameters (AgeSIRModel.cpp:66-77)
    for (int i = 0; i < n; ++i) {
        if (pb->N[i] < 0) { set_err(err, errlen, "Population sizes (N) cannot be negative."); return nullptr; }
        if (pb->gamma[i] < 0) { set_err(err, errlen, "Recovery rates (gamma) cannot be negative."); return nullptr; }
    }
    if (pb->q < 0) { set_err(err, errlen, "Transmissibility (q) cannot be negative."); return nullptr; }
    if (pb->scale_C_total < 0) { set_err(err, errlen, "Contact scale factor (scale_C_total) cannot be negative."); return nullptr; }
    for (int i = 0; i < n * n; ++i)
        if (pb->C[i] < 0) { set_err(err, errlen, "Baseline contact matrix entries cannot be negative."); return nullptr; }
    for (int p = 0; p < P; ++p) {
        const int f = pb->param_field[p];
        if (f != SEPAIHRD_SIR_F_Q && f != SEPAIHRD_SIR_F_SCALE_C_TOTAL && f != SEPAIHRD_SIR_F_GAMMA) {
            set_err(err, errlen, "param " + std::to_string(p) + ": unknown field code"); return nullptr;
        }
        if (f == SEPAIHRD_SIR_F_GAMMA && (pb->param_index[p] < 0 || pb->param_index[p] >= n)) {
            set_err(err, errlen, "param " + std::to_string(p) + ": age index out of range"); return nullptr;
        }
    }

    if (select_device(device, err, errlen) != SEPAIHRD_OK) return nullptr;

    auto* ctx = new sepaihrd_sir_ctx();
    ctx->device = device; ctx->solver = pb->solver; ctx->arith = pb->arith;
    ctx->n = n; ctx->T = T; ctx->P = P;
    ctx->field.assign(pb->param_field, pb->param_field + P);

    const int lpc = lanes_per_chain(n);
    std::vector<double> Npad(lpc, 0.0), gpad(lpc, 0.0), Cpad((size_t)lpc * lpc, 0.0), init((size_t)SIR_COMP * lpc, 0.0),
        obs((size_t)T * lpc, 0.0);
    for (int i = 0; i < n; ++i) { Npad[i] = pb->N[i]; gpad[i] = pb->gamma[i]; }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Cpad[(size_t)i * lpc + j] = pb->C[(size_t)i * n + j];
    for (int c = 0; c < SIR_COMP; ++c)
        for (int i = 0; i < n; ++i) init[(size_t)c * lpc + i] = pb->initial_state[(size_t)c * n + i];
    int obs_not_finite = 0;
    for (int k = 0; k < T; ++k)
        for (int i = 0; i < n; ++i) {
            const double o = pb->obs[(size_t)k * n + i];
            const double y = (o < 0.0) ? 0.0 : o;  // cwiseMax(0.0); +inf and NaN stay as they are
            if (!std::isfinite(y)) obs_not_finite = 1;
            obs[(size_t)k * lpc + i] = y;
        }
    double max_gap = 0.0;
    for (int i = 1; i < T; ++i) max_gap = std::max(max_gap, pb->times[i] - pb->times[i - 1]);

    SirDevProblem& d = ctx->dp;
    d.n = n; d.lpc = lpc; d.T = T; d.P = P;
    d.max_attempts = pb->max_attempts > 0 ? pb->max_attempts : 1000000;
    d.obs_not_finite = obs_not_finite;
    d.abs_tol = pb->abs_err; d.rel_tol = pb->rel_err; d.dt_hint = pb->dt_hint; d.max_gap = max_gap;
    d.q = pb->q; d.scale = pb->scale_C_total;
    bool ok = true;
    d.times = upload(ctx->allocs, std::vector<double>(pb->times, pb->times + T), ok);
    d.N = upload(ctx->allocs, Npad, ok);
    d.C = upload(ctx->allocs, Cpad, ok);
    d.gamma = upload(ctx->allocs, gpad, ok);
    d.init_state = upload(ctx->allocs, init, ok);
    d.obs = upload(ctx->allocs, obs, ok);
    d.param_field = upload(ctx->allocs, ctx->field, ok);
    d.param_index = upload(ctx->allocs, std::vector<int32_t>(pb->param_index, pb->param_index + P), ok);
    if (!ok) {
        set_err(err, errlen, "device allocation / upload failed");
        sepaihrd_sir_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void sepaihrd_sir_destroy(sepaihrd_sir_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    delete ctx;
}

const char* sepaihrd_sir_last_error(const sepaihrd_sir_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "ctx is NULL"; }

int sepaihrd_sir_set_arith(sepaihrd_sir_ctx* ctx, int arith) {
    if (!ctx || (arith != SEPAIHRD_ARITH_STRICT && arith != SEPAIHRD_ARITH_FMA)) return SEPAIHRD_E_INVALID_ARG;
    ctx->arith = arith;
    return SEPAIHRD_OK;
}

int sepaihrd_sir_reserve(sepaihrd_sir_ctx* ctx, int max_B) {
    if (!ctx || max_B < 0) return SEPAIHRD_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    return ensure_staging(ctx, (size_t)max_B, 0);
}

int sepaihrd_sir_eval_batch_device(sepaihrd_sir_ctx* ctx, const double* d_theta, int B, double* d_loglik, int32_t* d_status,
                                   int32_t* d_n_accept, int32_t* d_n_reject, double* d_traj, void* stream) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (B < 0 || (B > 0 && (!d_theta || !d_loglik))) {
        ctx->last_error = "sir_eval_batch_device: NULL theta/loglik or negative B";
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (B == 0) return SEPAIHRD_OK;
    const SirOutputs out{d_loglik, d_status, d_n_accept, d_n_reject, d_traj};
    const int rc = ctx->arith == SEPAIHRD_ARITH_FMA ? launch_sir_eval_fma(ctx->dp, ctx->solver, d_theta, B, out, stream)
                                                    : launch_sir_eval_strict(ctx->dp, ctx->solver, d_theta, B, out, stream);
    if (rc != 0) {
        ctx->last_error = rc == -4 ? "unsupported lanes-per-chain or solver" : "kernel launch failed";
        return rc == -4 ? SEPAIHRD_E_UNSUPPORTED : SEPAIHRD_E_HIP;
    }
    return SEPAIHRD_OK;
}

int sepaihrd_sir_eval_batch(sepaihrd_sir_ctx* ctx, const double* theta, int B, double* loglik, int32_t* status, int32_t* n_accept,
                            int32_t* n_reject, double* traj) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (B < 0 || (B > 0 && (!theta || !loglik))) {
        ctx->last_error = "sir_eval_batch: NULL theta/loglik or negative B";
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (B == 0) return SEPAIHRD_OK;
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    const size_t nB = (size_t)B;
    const size_t traj_elems = traj ? nB * ctx->T * SIR_COMP * ctx->n : 0;
    {
        const int rc = ensure_staging(ctx, nB, traj_elems);
        if (rc != SEPAIHRD_OK) return rc;
    }
    int32_t* d_status = ctx->d_ints;
    int32_t* d_nacc = ctx->d_ints + nB;
    int32_t* d_nrej = ctx->d_ints + 2 * nB;
    HIP_TRY(hipMemcpy(ctx->d_theta, theta, nB * ctx->P * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    const int rc = sepaihrd_sir_eval_batch_device(ctx, ctx->d_theta, B, ctx->d_loglik, d_status, d_nacc, d_nrej,
                                                  traj ? ctx->d_traj : nullptr, nullptr);
    if (rc != SEPAIHRD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(loglik, ctx->d_loglik, nB * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (status) HIP_TRY(hipMemcpy(status, d_status, nB * sizeof(int32_t), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (n_accept) HIP_TRY(hipMemcpy(n_accept, d_nacc, nB * sizeof(int32_t), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (n_reject) HIP_TRY(hipMemcpy(n_reject, d_nrej, nB * sizeof(int32_t), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (traj) HIP_TRY(hipMemcpy(traj, ctx->d_traj, traj_elems * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

// SIRParameterManager::applyConstraints (SIRParameterManager.cpp:137-156)
int sepaihrd_sir_apply_constraints(const sepaihrd_sir_ctx* ctx, const double* in, int B, double* out) {
    if (!ctx || !in || !out || B < 0) return SEPAIHRD_E_INVALID_ARG;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < ctx->P; ++p) {
            const double v = in[(size_t)b * ctx->P + p];
            out[(size_t)b * ctx->P + p] = ctx->field[p] == SEPAIHRD_SIR_F_Q ? std::max(1e-12, v) : std::max(0.0, v);
        }
    return SEPAIHRD_OK;
}

// The constraint table of a sampler's proposals, for constrain() of the propose kernels in clamp mode.  q: bounded, lower =
// 1e-12, upper = +inf -- m = (v < lo) ? lo : v, then (hi < m) ? hi : m = m, the value std::max(1e-12, v) returns for every
// finite v.  scale_C_total and gamma_i: NOT marked bounded, because the kernels' unbounded clamp is (0 < v) ? v : 0 --
// std::max(0.0, v) as libstdc++ writes it, the sign of a zero included (the bounded form would keep a -0.0 that std::max
// turns into +0.0).  Their lower / upper entries (0, +inf) say what the rule amounts to.
int sepaihrd_sir_constraint_bounds(const int32_t* param_field, int n_params, double* lower, double* upper, int32_t* has_bounds) {
    if (!param_field || n_params < 0 || !lower || !upper) return SEPAIHRD_E_INVALID_ARG;
    for (int p = 0; p < n_params; ++p) {
        lower[p] = param_field[p] == SEPAIHRD_SIR_F_Q ? 1e-12 : 0.0;
        upper[p] = std::numeric_limits<double>::infinity();
        if (has_bounds) has_bounds[p] = param_field[p] == SEPAIHRD_SIR_F_Q ? 1 : 0;
    }
    return SEPAIHRD_OK;
}

int sepaihrd_sir_validate_events(const sepaihrd_sir_event* events, const int32_t* n_events, int K, int n_times, char* err, int errlen) {
    if (K <= 0 || n_times < 1 || !n_events) { set_err(err, errlen, "validate_events: need K > 0, n_times >= 1 and n_events"); return SEPAIHRD_E_INVALID_ARG; }
    for (int k = 0; k < K; ++k) {
        const std::string sc = "scenario " + std::to_string(k);
        if (n_events[k] < 0 || n_events[k] > SEPAIHRD_SIR_MAX_EVENTS) {
            set_err(err, errlen, sc + ": " + std::to_string(n_events[k]) + " events (at most " + std::to_string(SEPAIHRD_SIR_MAX_EVENTS) + ")");
            return SEPAIHRD_E_INVALID_ARG;
        }
        if (n_events[k] > 0 && !events) { set_err(err, errlen, sc + ": events is NULL"); return SEPAIHRD_E_INVALID_ARG; }
        for (int e = 0; e < n_events[k]; ++e) {
            const sepaihrd_sir_event& ev = events[(size_t)k * SEPAIHRD_SIR_MAX_EVENTS + e];
            const std::string who = sc + " event " + std::to_string(e) + ": ";
            if (ev.time_index < 0 || ev.time_index >= n_times) {
                set_err(err, errlen, who + "time_index " + std::to_string(ev.time_index) + " outside [0, " + std::to_string(n_times) + ")");
                return SEPAIHRD_E_INVALID_ARG;
            }
            if (e > 0 && ev.time_index < events[(size_t)k * SEPAIHRD_SIR_MAX_EVENTS + e - 1].time_index) {
                set_err(err, errlen, who + "events are not sorted by time_index");
                return SEPAIHRD_E_INVALID_ARG;
            }
            if (ev.kind != SEPAIHRD_SIR_EV_CONTACT && ev.kind != SEPAIHRD_SIR_EV_TRANSMISSION) {
                set_err(err, errlen, who + "unknown kind " + std::to_string(ev.kind));
                return SEPAIHRD_E_INVALID_ARG;
            }
            if (!std::isfinite(ev.value)) { set_err(err, errlen, who + "value is not finite"); return SEPAIHRD_E_INVALID_ARG; }
            if (ev.kind == SEPAIHRD_SIR_EV_CONTACT && ev.value < 0.0) {
                set_err(err, errlen, who + "contact scale factor must be >= 0");
                return SEPAIHRD_E_INVALID_ARG;
            }
            if (ev.kind == SEPAIHRD_SIR_EV_TRANSMISSION && (ev.value < 0.0 || ev.value > 1.0)) {
                set_err(err, errlen, who + "transmission reduction must lie in [0, 1]");
                return SEPAIHRD_E_INVALID_ARG;
            }
        }
    }
    return SEPAIHRD_OK;
}

int sepaihrd_sir_scenario_ensemble(sepaihrd_sir_ctx* ctx, const double* theta, int S, const sepaihrd_sir_event* events,
                                   const int32_t* n_events, int K, const double* probs, int n_probs, double* quantiles, double* metrics,
                                   double* metric_summary, double* diff_quantiles, int32_t* status, int32_t* n_accept, int32_t* n_reject,
                                   int32_t* n_valid) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    auto refuse = [&](const std::string& msg, int rc) { ctx->last_error = "sir_scenario_ensemble: " + msg; return rc; };
    if (S <= 0 || K <= 0 || !theta || !n_events || !probs || n_probs <= 0 || n_probs > 1024)
        return refuse("need S > 0, K > 0, theta, n_events and probs (1..1024)", SEPAIHRD_E_INVALID_ARG);
    if (!probabilities_valid(probs, n_probs)) return refuse("probabilities must lie in [0, 1]", SEPAIHRD_E_INVALID_ARG);
    {
        char msg[256] = "";
        if (sepaihrd_sir_validate_events(events, n_events, K, ctx->T, msg, (int)sizeof(msg)) != SEPAIHRD_OK)
            return refuse(msg, SEPAIHRD_E_INVALID_ARG);
    }
    const SirDevProblem& dp = ctx->dp;
    const size_t B = (size_t)K * (size_t)S;
    if (B > (size_t)std::numeric_limits<int32_t>::max() / 2)
        return refuse("K x S chains exceed one launch (a 32-bit chain count)", SEPAIHRD_E_INVALID_ARG);
    // sizes
    const SegmentPlan plan = plan_segments((size_t)S);  // a segment: the S samples of one (scenario, series, time, column)
    const int S_pad = (int)plan.pad;
    const int n = dp.n, T = dp.T, W = SIR_ENS_SCALARS + 2 * n;
    const size_t P = (size_t)ctx->P;
    const size_t n_rows = (size_t)SIR_ENS_SERIES * T * (n + 1);  // sortable segments per scenario
    const size_t n_vals = (size_t)K * n_rows * S_pad;
    const size_t n_q = (size_t)K * SIR_ENS_SERIES * n_probs * T * (n + 1);
    const size_t n_metrics = B * W, n_svals = (size_t)2 * K * W * S_pad;
    const size_t n_summary = (size_t)K * W * (2 + n_probs), n_diff = (size_t)K * W * n_probs;
    const size_t n_scratch = sort_scratch_doubles(plan, std::max(n_rows * S_pad, n_svals));
    const size_t n_evbytes = (size_t)K * SEPAIHRD_SIR_MAX_EVENTS * sizeof(sepaihrd_sir_event);
    HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP);
    // K x S within one launch: the buffers below must fit the device's memory (the stored series dominate: K 3 T (n + 1)
    // S_pad doubles); larger requests are refused before anything is allocated
    const size_t need_bytes = sizeof(double) * (B * P + n_vals + n_q + n_metrics + (size_t)S + n_svals + n_summary + n_diff + n_scratch + (size_t)n_probs) +
                              sizeof(int32_t) * (3 * B + 4 * (size_t)K) + n_evbytes;
    {
        const int rc = require_device_memory(ctx, need_bytes, "sir_scenario_ensemble: K x S = " + std::to_string(B) + " runs need",
                                             "split the scenarios or the samples over several calls");
        if (rc != SEPAIHRD_OK) return rc;
    }
    // buffers
    auto& slots = ctx->slots;
    double *d_theta = nullptr, *d_vals = nullptr, *d_probs = nullptr, *d_q = nullptr, *d_metrics = nullptr, *d_svals = nullptr,
           *d_summary = nullptr, *d_scratch = nullptr;
    int32_t *d_ints = nullptr, *d_counts = nullptr, *d_nev = nullptr;
    SirEvent* d_events = nullptr;
    if (!slots.get(SLOT_THETA, &d_theta, B * P) || !slots.get(SLOT_VALS, &d_vals, n_vals) ||
        !slots.get(SLOT_PROBS, &d_probs, (size_t)n_probs) || !slots.get(SLOT_QUANTILES, &d_q, n_q) ||
        !slots.get(SLOT_METRICS, &d_metrics, n_metrics + (size_t)S) || !slots.get(SLOT_SCEN_VALS, &d_svals, n_svals) ||
        !slots.get(SLOT_SCEN_SUMMARY, &d_summary, n_summary + n_diff) || !slots.get(SLOT_SORT_SCRATCH, &d_scratch, n_scratch) ||
        !slots.get(SLOT_INTS, &d_ints, 3 * B) || !slots.get(SLOT_COUNTS, &d_counts, (size_t)3 * K) ||
        !slots.get(SLOT_N_EVENTS, &d_nev, (size_t)K) || !slots.get(SLOT_EVENTS, &d_events, (size_t)K * SEPAIHRD_SIR_MAX_EVENTS))
        return refuse("device allocation failed", SEPAIHRD_E_HIP);
    for (Event& e : ctx->ens_ev)
        if (!e) HIP_TRY(hipEventCreate(&e), ctx, return SEPAIHRD_E_HIP);
    // uploads.  Every scenario integrates the same samples: theta replicated K times, chain c = scenario c / S, sample c % S
    HIP_TRY(hipMemcpy(d_theta, theta, (size_t)S * P * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    for (int k = 1; k < K; ++k)
        HIP_TRY(hipMemcpy(d_theta + (size_t)k * S * P, d_theta, (size_t)S * P * sizeof(double), hipMemcpyDeviceToDevice), ctx,
                    return SEPAIHRD_E_HIP);
    {
        std::vector<sepaihrd_sir_event> tab((size_t)K * SEPAIHRD_SIR_MAX_EVENTS, sepaihrd_sir_event{0, 0, 0.0});
        for (int k = 0; k < K; ++k)
            for (int e = 0; e < n_events[k]; ++e) tab[(size_t)k * SEPAIHRD_SIR_MAX_EVENTS + e] = events[(size_t)k * SEPAIHRD_SIR_MAX_EVENTS + e];
        HIP_TRY(hipMemcpy(d_events, tab.data(), n_evbytes, hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    }
    HIP_TRY(hipMemcpy(d_nev, n_events, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(d_probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    // launches
    ++ctx->ens_calls;
    int32_t* d_status = d_ints;
    int32_t* d_nacc = d_ints + B;
    int32_t* d_nrej = d_ints + 2 * B;
    HIP_TRY(hipEventRecord(ctx->ens_ev[0], nullptr), ctx, return SEPAIHRD_E_HIP);
    const SirOutputs out{nullptr, d_status, d_nacc, d_nrej, nullptr};
    const SirEnsArgs ens{S, S_pad, d_events, d_nev, d_vals};
    int rc = ctx->arith == SEPAIHRD_ARITH_FMA ? launch_sir_ens_fma(dp, ctx->solver, d_theta, (int)B, out, ens, nullptr)
                                              : launch_sir_ens_strict(dp, ctx->solver, d_theta, (int)B, out, ens, nullptr);
    if (rc != 0) {
        ctx->last_error = rc == -4 ? "unsupported lanes-per-chain or solver" : "kernel launch failed";
        return rc == -4 ? SEPAIHRD_E_UNSUPPORTED : SEPAIHRD_E_HIP;
    }
    HIP_TRY(hipEventRecord(ctx->ens_ev[1], nullptr), ctx, return SEPAIHRD_E_HIP);
    SirEnsSummaryArgs a{};
    a.K = K; a.S = S; a.S_pad = S_pad; a.n = n; a.lpc = dp.lpc; a.T = T; a.P = ctx->P; a.n_probs = n_probs;
    a.pb = &ctx->dp; a.theta = d_theta; a.status = d_status; a.vals = d_vals; a.probs = d_probs;
    a.q_out = quantiles ? d_q : nullptr;
    a.n_valid = d_counts + 2 * K;
    const bool want_summaries = metric_summary != nullptr || diff_quantiles != nullptr;
    a.metrics = (metrics != nullptr || want_summaries) ? d_metrics : nullptr;
    a.r0 = d_metrics + n_metrics;
    a.svals = d_svals; a.counts = d_counts;
    a.summary_out = want_summaries ? d_summary : nullptr;
    a.diff_out = want_summaries ? d_summary + n_summary : nullptr;
    a.sort_scratch = plan.in_lds ? nullptr : d_scratch;
    a.sort_scratch_doubles = n_scratch;
    a.ev_after_metrics = ctx->ens_ev[2];
    rc = launch_sir_ensemble_summaries(a, nullptr);
    if (rc != 0) return refuse("summary launch failed", SEPAIHRD_E_HIP);
    HIP_TRY(hipEventRecord(ctx->ens_ev[3], nullptr), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipDeviceSynchronize(), ctx, return SEPAIHRD_E_HIP);
    for (int i = 0; i < 3; ++i) {
        float ms = 0.0f;
        ctx->ens_ms[i] = hipEventElapsedTime(&ms, ctx->ens_ev[i], ctx->ens_ev[i + 1]) == hipSuccess ? (double)ms : -1.0;
    }
    // fetches
    ResultFetch res;
    res.fetch(quantiles, d_q, n_q * sizeof(double));
    res.fetch(metrics, d_metrics, n_metrics * sizeof(double));
    res.fetch(metric_summary, d_summary, n_summary * sizeof(double));
    res.fetch(diff_quantiles, d_summary + n_summary, n_diff * sizeof(double));
    res.fetch(status, d_status, B * sizeof(int32_t));
    res.fetch(n_accept, d_nacc, B * sizeof(int32_t));
    res.fetch(n_reject, d_nrej, B * sizeof(int32_t));
    res.fetch(n_valid, d_counts + 2 * K, (size_t)K * sizeof(int32_t));
    if (!res.ok()) return refuse("copy of the results failed", SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_sir_ensemble_quantiles(sepaihrd_sir_ctx* ctx, const double* theta, int S, const double* probs, int n_probs, double* quantiles,
                                    double* metrics, double* metric_summary, int32_t* status, int32_t* n_valid) {
    const int32_t none = 0;
    return sepaihrd_sir_scenario_ensemble(ctx, theta, S, nullptr, &none, 1, probs, n_probs, quantiles, metrics, metric_summary, nullptr, status,
                                          nullptr, nullptr, n_valid);
}

int sepaihrd_sir_ensemble_timing(const sepaihrd_sir_ctx* ctx, int64_t* calls, double* ms) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    if (calls) *calls = ctx->ens_calls;
    if (ms)
        for (int i = 0; i < 3; ++i) ms[i] = ctx->ens_ms[i];
    return SEPAIHRD_OK;
}

sepaihrd_mh* sepaihrd_sir_mh_create(sepaihrd_sir_ctx* ctx, const sepaihrd_mh_config* config, const double* x0, const double* cov0) {
    if (!ctx) return nullptr;
    if (!ctx->mh_dp_ready) {
        if (hipSetDevice(ctx->device) != hipSuccess) { ctx->last_error = "hipSetDevice failed"; return nullptr; }
        std::vector<double> lower((size_t)ctx->P), upper((size_t)ctx->P);
        std::vector<int32_t> bounded((size_t)ctx->P);
        (void)sepaihrd_sir_constraint_bounds(ctx->field.data(), ctx->P, lower.data(), upper.data(), bounded.data());
        bool ok = true;
        DevProblem& d = ctx->mh_dp;
        d.n = ctx->n; d.lpc = ctx->dp.lpc; d.T = ctx->T; d.P = ctx->P;
        d.constraint_mode = 0;  // clamp: this manager has no reflect mode
        d.lower = upload(ctx->allocs, lower, ok);
        d.upper = upload(ctx->allocs, upper, ok);
        d.has_bounds = upload(ctx->allocs, bounded, ok);
        if (!ok) { ctx->last_error = "sir_mh_create: upload of the constraint table failed"; return nullptr; }
        ctx->mh_dp_ready = true;
    }
    return mh_create_on(MhBackend{ctx->device, ctx->P, ctx->last_error, ctx->mh_dp, ctx->libm_log_diff, ctx->libm_exp_diff, ctx->no_pending, nullptr, ctx},
                        config, x0, cov0);
}

int sepaihrd_sir_device_libm_check(sepaihrd_sir_ctx* ctx, int32_t* n_log_diff, int32_t* n_exp_diff) {
    if (!ctx) return SEPAIHRD_E_INVALID_ARG;
    return device_libm_check(ctx->device, ctx->last_error, ctx->libm_log_diff, ctx->libm_exp_diff, n_log_diff, n_exp_diff);
}

}  // extern "C"
