// csrc/sepaihrd_mh_capi.cpp -- the host driver of the device-resident Adaptive-Metropolis sampler: sepaihrd_mh, the
// sepaihrd_mh_* entry points of include/sepaihrd_hip.h and the libm self-check a sampler asks of its context.  A sampler sees
// its context (SEPAIHRD or SIR) through MhBackend (csrc/sepaihrd_mh_backend.h); the layout of every slab it carves is stated
// in csrc/sepaihrd_mh_layout.h; the kernels are csrc/sepaihrd_sampler.hip's.
#include "sepaihrd_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sepaihrd_device.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_mh_backend.h"
#include "sepaihrd_mh_layout.h"

using namespace sepaihrd;
namespace lay = sepaihrd::mh_layout;

struct sepaihrd_mh {
    explicit sepaihrd_mh(const MhBackend& b) : be(b) {}
    // the context this sampler evaluates on, as far as a sampler needs it (csrc/sepaihrd_mh_backend.h)
    MhBackend be;
    MhBackend* const ctx = &be;
    int form_asked = SEPAIHRD_MH_FORM_AUTO;  // sepaihrd_mh_set_kernel_form
    bool packed = false;                     // ... resolved: the per-iteration kernels run in the packed form
    SamplerState st{};
    int rows = 0;  // history rows written so far
    // Owners release in reverse order of declaration: the three streams, declared last, are drained and destroyed before the
    // events, and those before the buffers.  st's pointers, and the d_ / h_ pointers and views below, are views of these two:
    DeviceAllocs allocs;  // what the sampler allocates once (sepaihrd_mh_create, sepaihrd_mh_keep_scale_on_device)
    PinnedAllocs pinned;
    double *d_z = nullptr, *d_scale = nullptr;
    lay::Fetch d_fetch{}, h_fetch{};  // the evaluation's values and statuses, and their pinned mirror: one copy per fetch
    uint8_t* d_accept = nullptr;
    uint8_t* d_draw_todo = nullptr;  // [C] chains the windowed draw of the packed form left to the block-per-chain kernel
    // sepaihrd_mh_stage_normals / sepaihrd_mh_step: a second normals buffer filled by a copy stream while the
    // evaluation runs, and ONE packed upload per iteration (accept flags, scales, re-drawn rows) from pinned memory
    double* d_z_stage = nullptr;
    double* d_lz[2] = {nullptr, nullptr};  // [C][P] each: L z of both continuations, formed beside the evaluation (sampler_lz)
    bool lz_ready = false;                 // d_lz holds the products of the normals staged for the coming test
    Event ev_staged;
    bool staged = false;
    double* h_stage[2] = {nullptr, nullptr};  // pinned [C][P] each: the caller fills one while the other's copy may still run
    int stage_turn = 0;
    lay::Pack d_pack{}, h_pack{};
    // accept test on the device (sepaihrd_mh_step_tested): current and best values per chain, the test's inputs (the pinned
    // mirror is filled by the caller while the evaluation runs), its outcome with its pinned mirror, the scale it selected
    double *d_lp = nullptr, *d_best_lp = nullptr;
    lay::TestInputs d_test{}, h_test{};
    double* d_scale_sel = nullptr;
    lay::TestOutcome d_out{}, h_out{};
    Event ev_test_up, ev_tested, ev_fetched, ev_proposed;
    hipEvent_t ev_last_proposed = nullptr;  // whichever of the two marks the end of the last proposal
    bool values_set = false, test_pending = false, proposed_once = false;
    // rank-one covariance updates not yet applied (see mh_rank1_catchup_cov_kernel): the state each one reads and its
    // gamma, in the order they were asked for.  Uploaded from a page-locked buffer; both are laid out for r1_cap entries.
    std::vector<int32_t> pending_row;
    std::vector<double> pending_gamma;
    DeviceBuf r1_dev;
    PinnedBuf r1_host;
    lay::Rank1 d_r1{}, h_r1{};
    size_t r1_cap = 0;
    Event ev_r1;  // the last upload out of h_r1 has been copied
    bool r1_in_flight = false;
    // states [mom_rows, rows) have not entered the running sums yet (see mh_moments_catchup_kernel)
    int mom_rows = 0;
    bool device_rng = false;  // the chains' mt19937 streams live on the device (sepaihrd_mh_seed_streams)
    // a self-contained sampler lets its caller queue iterations ahead: at most ~128 of them (an event every 32 steps, four kept)
    Event ev_ahead[4];
    bool ev_ahead_used[4] = {false, false, false, false};
    long auto_steps = 0;
    int covariance_mode = SEPAIHRD_MH_COV_RUNNING;
    int iterations = 0;
    double* d_summary = nullptr;
    // sepaihrd_mh_snapshot_begin / _end: a gather on the sampler's stream, the copy home on a stream of its own
    Event ev_snap_gathered, ev_snap_done;
    DeviceBuf snap_dev, snap_chains_dev;
    PinnedBuf snap_host;
    double* d_snap = nullptr;   // views of the three, which grow with what is asked for; snap_dev and snap_host share snap_cap
    double* h_snap = nullptr;
    int32_t* d_snap_chains = nullptr;
    size_t snap_cap = 0, snap_chain_cap = 0;
    int snap_n = 0, snap_count = 0;
    bool snap_pending = false;
    std::vector<int32_t> snap_chain_list;  // what d_snap_chains holds
    Stream snap_stream;
    Stream copy_stream;
    Stream stream;  // own non-blocking stream: several samplers (one per host thread) overlap
};

namespace {

// How an entry point opens.  MH_ARGS: a null handle, or arguments that fail `args_ok`, are SEPAIHRD_E_INVALID_ARG without a text;
// from here on `ctx` is the sampler's context.  MH_ON_DEVICE: the context's device is the current one, or SEPAIHRD_E_HIP.
// MH_ENTER: both, where nothing else is checked in between.  MH_REFUSE: a refusal with its text.  MH_LAUNCH_TRY: a launch (or a
// chain of them) that did not go out.
#define MH_ARGS(mh, args_ok) if (!(mh) || !(args_ok)) return SEPAIHRD_E_INVALID_ARG; MhBackend* const ctx = (mh)->ctx
#define MH_ON_DEVICE() HIP_TRY(hipSetDevice(ctx->device), ctx, return SEPAIHRD_E_HIP)
#define MH_ENTER(mh, args_ok) MH_ARGS(mh, args_ok); MH_ON_DEVICE()
#define MH_REFUSE(text) do { ctx->last_error = text; return SEPAIHRD_E_INVALID_ARG; } while (0)
#define MH_LAUNCH_TRY(expr, what) do { if ((expr) != 0) { ctx->last_error = what; return SEPAIHRD_E_HIP; } } while (0)

// queue the rank-one update that precedes the next proposal: it reads the newest state (row rows - 1) with this gamma
void mh_queue_rank1(sepaihrd_mh* mh, double gamma) {
    mh->pending_row.push_back(mh->rows - 1);
    mh->pending_gamma.push_back(gamma);
}
// apply the queued updates in order (someone is about to read the covariance, or the ring is about to overwrite a
// state they read)
int mh_flush_rank1(sepaihrd_mh* mh) {
    const size_t n = mh->pending_gamma.size();
    if (n == 0) return 0;
    for (size_t k = 0; k < n; ++k)  // every state still in the ring (mh_before_commit keeps it so)
        if (mh->pending_row[k] < 0 || mh->pending_row[k] >= mh->rows || mh->pending_row[k] < mh->rows - mh->st.window) return -1;
    if (mh->r1_in_flight) {  // the page-locked buffer is still the source of the previous upload
        if (hipEventSynchronize(mh->ev_r1) != hipSuccess) return -3;
        mh->r1_in_flight = false;
    }
    if (n > mh->r1_cap) {
        const size_t cap = std::max<size_t>(2 * n, 256);
        mh->r1_cap = 0;
        if (!mh->r1_dev.reserve(lay::rank1_bytes(cap)) || !mh->r1_host.reserve(lay::rank1_bytes(cap))) return -3;
        mh->r1_cap = cap;
        mh->d_r1 = lay::rank1_view(mh->r1_dev.p, cap);
        mh->h_r1 = lay::rank1_view(mh->r1_host.p, cap);
    }
    std::memcpy(mh->h_r1.gammas, mh->pending_gamma.data(), n * sizeof(double));
    std::memcpy(mh->h_r1.rows, mh->pending_row.data(), n * sizeof(int32_t));
    if (hipMemcpyAsync(mh->d_r1.gammas, mh->h_r1.gammas, lay::rank1_sent_bytes(mh->r1_cap, n), hipMemcpyHostToDevice, mh->stream) != hipSuccess) return -3;
    if (hipEventRecord(mh->ev_r1, mh->stream) != hipSuccess) return -3;
    mh->r1_in_flight = true;
    const int rc = sampler_rank1_catchup(mh->st, mh->d_r1.rows, mh->d_r1.gammas, (int)n, mh->stream);
    mh->pending_gamma.clear();
    mh->pending_row.clear();
    return rc;
}
// the states committed since the last catch-up enter the running sums; emit_len > 0: and the refresh of
// recomputeFullCovariance for a history of emit_len states follows in the same launch
int mh_flush_moments(sepaihrd_mh* mh, int emit_len) {
    if (mh->covariance_mode != SEPAIHRD_MH_COV_RUNNING) return 0;
    const int n = mh->rows - mh->mom_rows;
    if (n <= 0 && emit_len <= 0) return 0;
    const int rc = sampler_moments_catchup(mh->st, mh->mom_rows, n, emit_len, mh->stream);
    mh->mom_rows = mh->rows;
    return rc;
}
// Before state `rows` is written into its ring slot: whatever is queued on the state that slot still holds runs first.
int mh_before_commit(sepaihrd_mh* mh) {
    const int oldest_kept = mh->rows + 1 - mh->st.window;  // after the commit the ring holds states oldest_kept .. rows
    int rc = 0;
    if (mh->covariance_mode == SEPAIHRD_MH_COV_RUNNING && mh->mom_rows < oldest_kept) rc = mh_flush_moments(mh, 0);
    if (rc == 0 && !mh->pending_row.empty() && mh->pending_row.front() < oldest_kept) rc = mh_flush_rank1(mh);
    return rc;
}
// the adaptation step before a proposal: 0 none, 1 rank-one update, 2 + Cholesky refresh of cov + eps I, 3 + full
// recompute first (which overwrites covariance and mean: queued rank-one updates are dropped unapplied)
int mh_adapt_step(sepaihrd_mh* mh, double gamma, int adapt) {
    int rc = 0;
    if (adapt >= 1) mh_queue_rank1(mh, gamma);
    if (adapt == 2) {
        rc = mh_flush_rank1(mh);
        if (rc == 0) rc = sampler_cholesky(mh->st, mh->st.reg_eps, 0, mh->stream);  // :295-300
    } else if (adapt == 3) {
        mh->pending_gamma.clear();
        mh->pending_row.clear();
        if (mh->covariance_mode == SEPAIHRD_MH_COV_RUNNING) rc = mh_flush_moments(mh, mh->rows);
        else rc = sampler_full_covariance(mh->st, mh->rows, mh->stream);
        if (rc == 0) rc = sampler_cholesky_refresh(mh->st, mh->stream);  // :190-197 and :295-300, each kept on success
    }
    return rc;
}

// log-likelihoods (and statuses) of the last evaluation: one copy into the page-locked mirror, the wait, two memcpy
int mh_fetch_values(sepaihrd_mh* mh, double* loglik, int32_t* status) {
    MhBackend* ctx = mh->ctx;
    const size_t C = (size_t)mh->st.C;
    HIP_TRY(hipMemcpyAsync(mh->h_fetch.loglik, mh->d_fetch.loglik, lay::fetch_bytes(C, status != nullptr), hipMemcpyDeviceToHost, mh->stream), ctx,
            return SEPAIHRD_E_HIP);
    HIP_TRY(hipStreamSynchronize(mh->stream), ctx, return SEPAIHRD_E_HIP);
    std::memcpy(loglik, mh->h_fetch.loglik, C * sizeof(double));
    if (status) std::memcpy(status, mh->h_fetch.status, C * sizeof(int32_t));
    return SEPAIHRD_OK;
}

// the objective of every chain at d_theta, queued on the sampler's stream: values and statuses land in d_fetch
int mh_eval_device(sepaihrd_mh* mh, const double* d_theta) {
    MhBackend* ctx = mh->ctx;
    if (ctx->sep)
        return sepaihrd_eval_batch_device(ctx->sep, d_theta, mh->st.C, mh->d_fetch.loglik, mh->d_fetch.status, nullptr, nullptr, nullptr, nullptr, mh->stream);
    return sepaihrd_sir_eval_batch_device(ctx->sir, d_theta, mh->st.C, mh->d_fetch.loglik, mh->d_fetch.status, nullptr, nullptr, nullptr, mh->stream);
}
int mh_eval(sepaihrd_mh* mh, const double* d_theta, double* loglik, int32_t* status) {
    const int rc = mh_eval_device(mh, d_theta);
    if (rc != SEPAIHRD_OK) return rc;
    return mh_fetch_values(mh, loglik, status);
}
// a proposal has been queued from the staged normals: the next staging goes to the other buffer, and the evaluation follows
int mh_proposal_queued(sepaihrd_mh* mh) {
    std::swap(mh->d_z, mh->d_z_stage);
    mh->staged = false;
    return mh_eval_device(mh, mh->st.prop);
}

// What a reader does before it copies: the sampler's device, `flush` (queued work that what is read depends on; flush_error
// when it fails), the sampler's stream drained.  Then `bytes` from `src`, where the reader has one plain copy (dst non-null).
int mh_read(sepaihrd_mh* mh, void* dst = nullptr, const void* src = nullptr, size_t bytes = 0, int (*flush)(sepaihrd_mh*) = nullptr,
            const char* flush_error = "") {
    MhBackend* ctx = mh->ctx;
    MH_ON_DEVICE();
    if (flush) MH_LAUNCH_TRY(flush(mh), flush_error);
    HIP_TRY(hipStreamSynchronize(mh->stream), ctx, return SEPAIHRD_E_HIP);
    if (dst) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

// The form of the per-iteration kernels.  AUTO on a SEPAIHRD-backed sampler is block-per-chain whatever P is.  On a
// SIR-backed sampler it is the packed form where that measured faster by more than the alternating runs' own spread
// (tools/bench_sir_mh.py): P = 5 (groups of 8 lanes) and P = 18 (groups of 32), at 4096 and at
// 65 536 chains -- 1.2 % to 33 % per iteration against spreads of 0.02 - 0.9 %.  Both chain counts won, so the rule does not
// look at C; it covers the group widths up to the widest one measured.  A group of 64 lanes (P > 32: one chain per
// wavefront, the mapping the block-per-chain kernels already have) was not measured and stays block-per-chain.
bool mh_auto_packed(const MhBackend* ctx, int P, int C) {
    (void)C;
    return ctx->sir != nullptr && mh_packed_group(P) <= 32;
}
void mh_resolve_form(sepaihrd_mh* mh) {
    mh->packed = mh->form_asked == SEPAIHRD_MH_FORM_PACKED ||
                 (mh->form_asked == SEPAIHRD_MH_FORM_AUTO && mh_auto_packed(mh->ctx, mh->st.P, mh->st.C));
}
// the launches that have two forms
int mh_launch_propose(sepaihrd_mh* mh, const double* d_z, const double* d_scale, hipStream_t st) {
    return mh->packed ? sampler_propose_packed(mh->st, mh_bounds_of(mh->ctx->dp), d_z, d_scale, st)
                      : sampler_propose(mh->st, mh->ctx->dp, d_z, d_scale, st);
}
int mh_launch_propose_select(sepaihrd_mh* mh, const double* d_z_uniform, const double* d_z_plain, const uint8_t* d_flags,
                             const double* d_scale, hipStream_t st) {
    return mh->packed ? sampler_propose_select_packed(mh->st, mh_bounds_of(mh->ctx->dp), d_z_uniform, d_z_plain, d_flags, d_scale, st)
                      : sampler_propose_select(mh->st, mh->ctx->dp, d_z_uniform, d_z_plain, d_flags, d_scale, st);
}
int mh_launch_draw(sepaihrd_mh* mh, const uint8_t* d_flags, int first, double* d_log_u, double* d_z_uniform, double* d_z_plain,
                   int want_normals, hipStream_t st) {
    return mh->packed ? sampler_draw_packed(mh->st, d_flags, first, d_log_u, d_z_uniform, d_z_plain, want_normals, mh->d_draw_todo, st)
                      : sampler_draw(mh->st, d_flags, first, d_log_u, d_z_uniform, d_z_plain, want_normals, st);
}
int mh_launch_lz(sepaihrd_mh* mh, const double* d_z_uniform, const double* d_z_plain, double* d_lz_uniform, double* d_lz_plain, hipStream_t st) {
    return mh->packed ? sampler_lz_packed(mh->st, d_z_uniform, d_z_plain, d_lz_uniform, d_lz_plain, st)
                      : sampler_lz(mh->st, d_z_uniform, d_z_plain, d_lz_uniform, d_lz_plain, st);
}
int mh_launch_test_commit_propose(sepaihrd_mh* mh, const SamplerTestArgs& a, hipStream_t st) {
    return mh->packed ? sampler_test_commit_propose_packed(mh->st, mh_bounds_of(mh->ctx->dp), a, st)
                      : sampler_test_commit_propose(mh->st, mh->ctx->dp, a, st);
}

// seed_streams / keep_scale_on_device refuse when the device functions are not this host's libm
int mh_require_matching_libm(sepaihrd_mh* mh, const char* who) {
    MhBackend* ctx = mh->ctx;
    int32_t dl = 0, de = 0;
    const int rc = device_libm_check(ctx->device, ctx->last_error, ctx->libm_log_diff, ctx->libm_exp_diff, &dl, &de);
    if (rc != SEPAIHRD_OK) return rc;
    if (dl == 0 && de == 0) return SEPAIHRD_OK;
    char msg[384];
    std::snprintf(msg, sizeof(msg),
                  "%s: the device's log / exp (csrc/sepaihrd_rng.inc: glibc 2.35, x86-64, FMA variants) differ from this host's libm on %d "
                  "(log) and %d (exp) of %d self-check arguments: streams drawn on the device would not be the host's -- keep the draws "
                  "and the scale adaptation on the host (device_streams 0)", who, dl, de, sampler_libm_check_count());
    ctx->last_error = msg;
    return SEPAIHRD_E_UNSUPPORTED;
}

// ---- the parts of sepaihrd_mh_step_tested
bool mh_lz_ahead_wanted() {
    const char* e = std::getenv("SEPAIHRD_MH_LZ");
    return !(e && std::string(e) == "fused");
}
// Do the draws of the next test queue behind the evaluation on the main stream, instead of running beside it on the copy
// stream?  The draws of test i + 1 need nothing of evaluation i, so they run beside it -- as long as the evaluation leaves
// room.  A saturating batch (two 256-register waves on every SIMD) leaves none: the draw kernel's 65 536 small waves then
// take the slots of retiring integrator waves and hold up the next ones (round 4, 65 536 chains: the evaluation stretched
// from 2.9 to 3.6 ms around 0.1 ms of draws).  From that size on -- more than one round of two integrator waves per SIMD, the
// threshold of launch_one's -- the draws queue behind the evaluation (65 536 chains: 4.01 -> 3.43 ms per iteration; a batch of
// exactly one round, 32 768 chains, still gains from the overlap -- 1.95 against 2.00 -- as the draws fill the round's tail;
// a low-priority copy stream changed nothing).  SEPAIHRD_MH_DRAW=overlap|serial overrides (A/B runs).
bool mh_draws_behind_the_evaluation(const MhBackend* ctx, int C) {
    if (const char* e = std::getenv("SEPAIHRD_MH_DRAW")) {
        if (std::string(e) == "overlap") return false;
        if (std::string(e) == "serial") return true;
    }
    const long long chains_per_wave = WAVE / (ctx->dp.lpc > 0 ? ctx->dp.lpc : 1);
    return (C + chains_per_wave - 1) / chains_per_wave > 2 * 1024;
}

// A self-contained sampler's caller queues iterations ahead; every 32nd step leaves an event and waits for the one of ~128 steps ago.
int mh_throttle_look_ahead(sepaihrd_mh* mh) {
    MhBackend* ctx = mh->ctx;
    if ((mh->auto_steps++ % 32) != 0) return SEPAIHRD_OK;
    const int slot = (int)((mh->auto_steps / 32) % 4);
    MH_ON_DEVICE();
    if (!mh->ev_ahead[slot]) HIP_TRY(hipEventCreateWithFlags(&mh->ev_ahead[slot], hipEventDisableTiming), ctx, return SEPAIHRD_E_HIP);
    if (mh->ev_ahead_used[slot]) HIP_TRY(hipEventSynchronize(mh->ev_ahead[slot]), ctx, return SEPAIHRD_E_HIP);  // ~128 steps ago
    HIP_TRY(hipEventRecord(mh->ev_ahead[slot], mh->stream), ctx, return SEPAIHRD_E_HIP);
    mh->ev_ahead_used[slot] = true;
    return SEPAIHRD_OK;
}

// The test's inputs travel on the copy stream while the evaluation still runs -- drawn there by the device, or uploaded from
// the caller's page-locked mirror -- and the main stream waits for them (ev_test_up).
int mh_stage_test_inputs(sepaihrd_mh* mh, bool self_contained, int adapt, int last) {
    MhBackend* ctx = mh->ctx;
    hipStream_t st = mh->stream, cs = mh->copy_stream;
    const size_t C = (size_t)mh->st.C, P = (size_t)mh->st.P;
    const lay::TestInputs& in = mh->d_test;
    mh->lz_ready = false;
    // they may not overwrite what the previous proposal is reading
    if (mh->proposed_once) HIP_TRY(hipStreamWaitEvent(cs, mh->ev_last_proposed, 0), ctx, return SEPAIHRD_E_HIP);
    if (mh->device_rng) {
        // the caller supplies the two scale candidates only; log(u) and the normals of both continuations are drawn here,
        // from where the previous test left every chain's stream (its flags are final: the copy stream has just waited
        // for the kernel that wrote them)
        if (!self_contained)
            HIP_TRY(hipMemcpyAsync(in.scale_reject, mh->h_test.scale_reject, lay::test_scales_bytes(C), hipMemcpyHostToDevice, cs), ctx, return SEPAIHRD_E_HIP);
        const bool serial_draw = mh_draws_behind_the_evaluation(ctx, mh->st.C);
        MH_LAUNCH_TRY(mh_launch_draw(mh, mh->d_out.flags, 0, in.log_u, mh->d_z_stage, in.z_plain, last ? 0 : 1, serial_draw ? st : cs),
                      "mh_step_tested: draw launch failed");
        mh->staged = true;
        // ... and, when the draws run beside the evaluation and no covariance refresh separates this test from its proposal,
        // L z of both continuations too: the launch between two evaluations then reads no factor (SEPAIHRD_MH_LZ=fused: A/B)
        if (!serial_draw && !last && adapt <= 1 && mh->st.P <= 200 && mh_lz_ahead_wanted()) {
            MH_LAUNCH_TRY(mh_launch_lz(mh, mh->d_z_stage, in.z_plain, mh->d_lz[0], mh->d_lz[1], cs), "mh_step_tested: L z launch failed");
            mh->lz_ready = true;
        }
    } else
        HIP_TRY(hipMemcpyAsync(in.log_u, mh->h_test.log_u, lay::test_inputs_sent_bytes(C, P, !last), hipMemcpyHostToDevice, cs), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipEventRecord(mh->ev_test_up, cs), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipStreamWaitEvent(st, mh->ev_test_up, 0), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

// The outcome of the test just queued on the main stream goes home on the copy stream as soon as the test has run (ev_tested);
// the main stream does not wait for it.  It is for the caller's bookkeeping (sepaihrd_mh_fetch_test): a self-contained sampler
// keeps its own and reads it at the end.
int mh_send_outcome_home(sepaihrd_mh* mh, bool self_contained) {
    MhBackend* ctx = mh->ctx;
    hipStream_t st = mh->stream, cs = mh->copy_stream;
    HIP_TRY(hipEventRecord(mh->ev_tested, st), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipStreamWaitEvent(cs, mh->ev_tested, 0), ctx, return SEPAIHRD_E_HIP);
    if (self_contained) return SEPAIHRD_OK;
    HIP_TRY(hipMemcpyAsync(mh->h_out.values, mh->d_out.values, lay::test_outcome_bytes((size_t)mh->st.C), hipMemcpyDeviceToHost, cs), ctx,
            return SEPAIHRD_E_HIP);
    HIP_TRY(hipEventRecord(mh->ev_fetched, cs), ctx, return SEPAIHRD_E_HIP);
    mh->test_pending = true;
    return SEPAIHRD_OK;
}

// No covariance refresh between commit and proposal: test, commit and proposal in one launch (the staged normals landed
// before the test's inputs: same copy stream, staged first -- ev_test_up covers them).
int mh_step_fused(sepaihrd_mh* mh, const SamplerTestArgs& a, bool self_contained, double gamma, int adapt) {
    MhBackend* ctx = mh->ctx;
    MH_LAUNCH_TRY(mh_launch_test_commit_propose(mh, a, mh->stream), "mh_step_tested: launch failed");
    if (mh_send_outcome_home(mh, self_contained) != SEPAIHRD_OK) return SEPAIHRD_E_HIP;
    mh->ev_last_proposed = mh->ev_tested;  // one marker: tested AND proposed
    mh->proposed_once = true;
    mh->rows++;
    if (adapt == 1) mh_queue_rank1(mh, gamma);  // as mh_adapt_step: the queued update names history row rows - 1
    return mh_proposal_queued(mh);
}

// Test, commit, the adaptation step and the proposal as launches of their own; the last test of a run has no proposal.
int mh_step_split(sepaihrd_mh* mh, const SamplerTestArgs& a, bool self_contained, double gamma, int adapt, int last) {
    MhBackend* ctx = mh->ctx;
    hipStream_t st = mh->stream;
    MH_LAUNCH_TRY(sampler_accept_test(mh->st, a, st), "mh_step_tested: launch failed");
    if (mh_send_outcome_home(mh, self_contained) != SEPAIHRD_OK) return SEPAIHRD_E_HIP;
    MH_LAUNCH_TRY(sampler_commit_counted(mh->st, a.flags, mh->rows, 1, st), "mh_step_tested: launch failed");
    mh->rows++;
    if (last) return SEPAIHRD_OK;
    MH_LAUNCH_TRY(mh_adapt_step(mh, gamma, adapt), "mh_step_tested: launch failed");
    HIP_TRY(hipStreamWaitEvent(st, mh->ev_staged, 0), ctx, return SEPAIHRD_E_HIP);  // the staged normals have landed
    MH_LAUNCH_TRY(mh_launch_propose_select(mh, a.z_uniform, a.z_plain, a.flags, a.scale_sel, st), "mh_step_tested: launch failed");
    HIP_TRY(hipEventRecord(mh->ev_proposed, st), ctx, return SEPAIHRD_E_HIP);
    mh->ev_last_proposed = mh->ev_proposed;
    mh->proposed_once = true;
    return mh_proposal_queued(mh);
}

}  // namespace

// sepaihrd_mh_create / sepaihrd_sir_mh_create: the sampler's state on the device of the context `be` names
sepaihrd_mh* sepaihrd::mh_create_on(const MhBackend& be, const sepaihrd_mh_config* cfg, const double* x0, const double* cov0) {
    const MhBackend* const ctx = &be;
    const int P = ctx->P;
    if (!cfg || cfg->chains <= 0 || cfg->iterations <= 0 || !x0 || !cov0 || P > 200 ||
        (cfg->covariance_mode != SEPAIHRD_MH_COV_RUNNING && cfg->covariance_mode != SEPAIHRD_MH_COV_TWO_PASS)) {
        ctx->last_error = "mh_create: need chains > 0, iterations > 0, a known covariance_mode, x0, cov0 and at most 200 parameters";
        return nullptr;
    }
    const int C = cfg->chains;
    // ring of the newest states: every state of the run for the two-pass refresh, else the window asked for
    // (at least 2: the newest state and the one a queued update may still read), never more than the run has
    int window = cfg->covariance_mode == SEPAIHRD_MH_COV_TWO_PASS ? cfg->iterations
                                                                   : std::min(cfg->iterations, std::max(cfg->adaptation_window > 0 ? cfg->adaptation_window : 128, 2));
    const int thinning = cfg->thinning > 0 ? cfg->thinning : 0;
    const int n_store = thinning > 0 ? (cfg->iterations - 1) / thinning + 1 : 0;
    if (hipSetDevice(ctx->device) != hipSuccess) { ctx->last_error = "hipSetDevice failed"; return nullptr; }
    const size_t nC = (size_t)C, nP = (size_t)P, CP = nC * nP, CPP = CP * nP;
    {
        // say what the state costs before allocating instead of failing somewhere inside
        const double need = (double)CP * ((double)window + (double)n_store) * 8.0 + 3.0 * (double)CPP * 8.0 + 10.0 * (double)CP * 8.0;  // ... + the C*P arrays (state, proposal, means, sums, normals, L z)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > (double)free_b) {
            char msg[320];
            std::snprintf(msg, sizeof(msg),
                          "mh_create: sampler state needs %.3f GB (ring of newest states C*window*P = %d*%d*%d doubles, samples "
                          "C*%d*P, covariance + factor + second moment 3*C*P*P) but %.3f GB of device memory are free; run "
                          "fewer chains per sampler object%s",
                          need / 1e9, C, window, P, n_store, (double)free_b / 1e9,
                          cfg->covariance_mode == SEPAIHRD_MH_COV_TWO_PASS ? " or use SEPAIHRD_MH_COV_RUNNING (no full history)" : "");
            ctx->last_error = msg;
            return nullptr;
        }
    }
    auto* mh = new sepaihrd_mh(be);
    SamplerState& st = mh->st;
    st.C = C; st.P = P; st.window = window; st.thinning = std::max(thinning, 1); st.n_store = n_store;
    st.scaling = cfg->scaling_factor; st.reg_eps = cfg->reg_eps;
    mh->covariance_mode = cfg->covariance_mode; mh->iterations = cfg->iterations;
    bool ok = true;
    auto dalloc = [&](void** p, size_t bytes) { ok = ok && mh->allocs.bytes(p, bytes); };
    auto halloc = [&](void** p, size_t bytes) { ok = ok && mh->pinned.bytes(p, bytes); };
    // the slabs: one allocation each on the device and in page-locked memory, carved below (csrc/sepaihrd_mh_layout.h).  The
    // order of the allocations is where the arrays lie relative to each other, part of what every timing of the sampler measured.
    void *d_fetch = nullptr, *d_test = nullptr, *d_out = nullptr, *d_pack = nullptr, *h_fetch = nullptr, *h_test = nullptr, *h_out = nullptr, *h_pack = nullptr;
    dalloc((void**)&st.x, CP * sizeof(double));
    dalloc((void**)&st.prop, CP * sizeof(double));
    dalloc((void**)&st.cov, CPP * sizeof(double));
    dalloc((void**)&st.chol, CPP * sizeof(double));
    dalloc((void**)&st.mean, CP * sizeof(double));
    dalloc((void**)&st.best, CP * sizeof(double));
    dalloc((void**)&st.hist, CP * (size_t)window * sizeof(double));
    if (n_store > 0) dalloc((void**)&st.store, CP * (size_t)n_store * sizeof(double));
    dalloc((void**)&st.sum, CP * sizeof(double));
    dalloc((void**)&st.wmean, CP * sizeof(double));
    dalloc((void**)&st.m2, CPP * sizeof(double));
    dalloc((void**)&st.accepted, nC * sizeof(int32_t));
    dalloc((void**)&st.fail_counts, 3 * sizeof(uint32_t));
    dalloc((void**)&st.mt, nC * 624 * sizeof(uint32_t));
    dalloc((void**)&st.mt_idx, nC * sizeof(int32_t));
    dalloc((void**)&st.mt_used, nC * 2 * sizeof(int32_t));
    dalloc((void**)&mh->d_summary, nC * (2 * nP + 2) * sizeof(double));
    dalloc((void**)&mh->d_z, CP * sizeof(double));
    dalloc((void**)&mh->d_scale, nC * sizeof(double));
    dalloc(&d_fetch, lay::fetch_bytes(nC));
    dalloc((void**)&mh->d_accept, nC);
    dalloc((void**)&mh->d_draw_todo, nC);
    dalloc((void**)&mh->d_z_stage, CP * sizeof(double));
    dalloc((void**)&mh->d_lz[0], 2 * CP * sizeof(double));
    dalloc((void**)&mh->d_lp, nC * sizeof(double));
    dalloc((void**)&mh->d_best_lp, nC * sizeof(double));
    dalloc(&d_test, lay::test_inputs_bytes(nC, nP));
    dalloc((void**)&mh->d_scale_sel, nC * sizeof(double));
    dalloc(&d_out, lay::test_outcome_bytes(nC));
    dalloc(&d_pack, lay::pack_bytes(nC, nP));
    halloc(&h_pack, lay::pack_bytes(nC, nP));
    halloc(&h_fetch, lay::fetch_bytes(nC));
    halloc(&h_test, lay::test_inputs_bytes(nC, nP));
    halloc(&h_out, lay::test_outcome_bytes(nC));
    halloc((void**)&mh->h_stage[0], CP * sizeof(double));
    halloc((void**)&mh->h_stage[1], CP * sizeof(double));
    if (ok) {  // the one place that carves the slabs
        mh->d_lz[1] = mh->d_lz[0] + CP;
        mh->d_fetch = lay::fetch_view(d_fetch, nC);
        mh->h_fetch = lay::fetch_view(h_fetch, nC);
        mh->d_test = lay::test_inputs_view(static_cast<double*>(d_test), nC);
        mh->h_test = lay::test_inputs_view(static_cast<double*>(h_test), nC);
        mh->d_out = lay::test_outcome_view(d_out, nC);
        mh->h_out = lay::test_outcome_view(h_out, nC);
        mh->d_pack = lay::pack_view(d_pack, nC);
        mh->h_pack = lay::pack_view(h_pack, nC);
    }
    if (ok && (ctx->sep ? sepaihrd_reserve(ctx->sep, C) : sepaihrd_sir_reserve(ctx->sir, C)) != SEPAIHRD_OK) ok = false;
    if (ok && hipStreamCreateWithFlags(&mh->stream, hipStreamNonBlocking) != hipSuccess) ok = false;
    if (ok && hipStreamCreateWithFlags(&mh->copy_stream, hipStreamNonBlocking) != hipSuccess) ok = false;
    if (ok && hipEventCreateWithFlags(&mh->ev_staged, hipEventDisableTiming) != hipSuccess) ok = false;
    for (hipEvent_t* e : {&mh->ev_test_up, &mh->ev_tested, &mh->ev_fetched, &mh->ev_proposed, &mh->ev_r1})
        if (ok && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) ok = false;
    if (ok) ok = hipMemsetAsync(d_out, 0, lay::test_outcome_bytes(nC), mh->stream) == hipSuccess &&
                 hipMemsetAsync(st.sum, 0, CP * sizeof(double), mh->stream) == hipSuccess &&
                 hipMemsetAsync(st.wmean, 0, CP * sizeof(double), mh->stream) == hipSuccess &&
                 hipMemsetAsync(st.m2, 0, CPP * sizeof(double), mh->stream) == hipSuccess &&
                 hipMemsetAsync(st.accepted, 0, nC * sizeof(int32_t), mh->stream) == hipSuccess &&
                 hipMemsetAsync(st.fail_counts, 0, 3 * sizeof(uint32_t), mh->stream) == hipSuccess;
    if (ok) {
        std::vector<double> cov_all(CPP);
        for (int c = 0; c < C; ++c) std::copy(cov0, cov0 + nP * nP, cov_all.begin() + (size_t)c * nP * nP);
        ok = hipMemcpy(st.x, x0, CP * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(st.mean, x0, CP * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(st.best, x0, CP * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(st.cov, cov_all.data(), CPP * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemsetAsync(st.chol, 0, CPP * sizeof(double), mh->stream) == hipSuccess;
    }
    if (ok) ok = sampler_cholesky(st, 0.0, 1, mh->stream) == 0 && sampler_commit(st, nullptr, 0, mh->stream) == 0 &&
                 hipStreamSynchronize(mh->stream) == hipSuccess;
    if (!ok) {
        ctx->last_error = "mh_create: device allocation or initialisation failed";
        delete mh;
        return nullptr;
    }
    mh->rows = 1;
    mh_resolve_form(mh);
    if (ctx->sep) ctx_adopt_lazy_stream(ctx->sep, mh->stream);
    return mh;
}

// The device's log / exp (csrc/sepaihrd_rng.inc) restate ONE libm build.  Before a sampler lets the device draw, they are
// evaluated on fixed arguments and compared, bit for bit, with the std::log / std::exp of THIS process.
int sepaihrd::device_libm_check(int device, std::string& last_error, int& log_diff, int& exp_diff, int32_t* n_log_diff, int32_t* n_exp_diff) {
    struct { int device; std::string& last_error; int& libm_log_diff; int& libm_exp_diff; } view{device, last_error, log_diff, exp_diff}, *ctx = &view;
    if (ctx->libm_log_diff < 0) {
        MH_ON_DEVICE();
        const int N = sampler_libm_check_count();
        DeviceBuf buf;
        double* d_out = nullptr;
        ALLOC_TRY(buf.get(&d_out, 4 * (size_t)N), ctx, return SEPAIHRD_E_HIP);
        std::vector<double> h(4 * (size_t)N);
        const bool ok = sampler_libm_check_values(d_out, nullptr) == 0 &&
                        hipMemcpy(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) { ctx->last_error = "device_libm_check: launch or copy failed"; return SEPAIHRD_E_HIP; }
        int dl = 0, de = 0;
        for (int i = 0; i < N; ++i) {
            // volatile: the comparison must be against the library call, not against a constant the compiler folded
            volatile double xl = h[(size_t)i], xe = h[2 * (size_t)N + i];
            const double hl = std::log(xl), he = std::exp(xe);
            if (std::memcmp(&hl, &h[(size_t)N + i], sizeof(double)) != 0) ++dl;
            if (std::memcmp(&he, &h[3 * (size_t)N + i], sizeof(double)) != 0) ++de;
        }
        // test hook: pretend this host's libm is another one (the fall-back to host-drawn streams is then exercised on a
        // box whose libm does match)
        if (const char* e = std::getenv("SEPAIHRD_LIBM_SELFCHECK")) if (std::string(e) == "fail") { dl += 1; de += 1; }
        ctx->libm_log_diff = dl;
        ctx->libm_exp_diff = de;
    }
    if (n_log_diff) *n_log_diff = ctx->libm_log_diff;
    if (n_exp_diff) *n_exp_diff = ctx->libm_exp_diff;
    return SEPAIHRD_OK;
}

extern "C" {

sepaihrd_mh* sepaihrd_mh_create(sepaihrd_ctx* ctx, const sepaihrd_mh_config* cfg, const double* x0, const double* cov0) {
    if (!ctx) return nullptr;
    return mh_create_on(mh_backend_of(ctx), cfg, x0, cov0);
}

int sepaihrd_mh_set_kernel_form(sepaihrd_mh* mh, int form) {
    if (!mh || (form != SEPAIHRD_MH_FORM_AUTO && form != SEPAIHRD_MH_FORM_BLOCK_PER_CHAIN && form != SEPAIHRD_MH_FORM_PACKED))
        return SEPAIHRD_E_INVALID_ARG;
    if (form == SEPAIHRD_MH_FORM_PACKED && mh->st.P > MH_PACKED_MAX_P) {
        mh->ctx->last_error = "mh_set_kernel_form: the packed form holds a chain in one wavefront (at most 64 parameters)";
        return SEPAIHRD_E_UNSUPPORTED;
    }
    mh->form_asked = form;
    mh_resolve_form(mh);
    return SEPAIHRD_OK;
}

int sepaihrd_mh_get_kernel_form(const sepaihrd_mh* mh) {
    if (!mh) return SEPAIHRD_E_INVALID_ARG;
    return mh->packed ? SEPAIHRD_MH_FORM_PACKED : SEPAIHRD_MH_FORM_BLOCK_PER_CHAIN;
}

void sepaihrd_mh_destroy(sepaihrd_mh* mh) {
    if (!mh) return;
    (void)hipSetDevice(mh->ctx->device);
    if (mh->copy_stream) (void)hipStreamSynchronize(mh->copy_stream);
    if (mh->stream) {
        (void)hipStreamSynchronize(mh->stream);
        if (mh->ctx->sep) ctx_forget_stream(mh->ctx->sep, mh->stream);  // all of it is done
    }
    delete mh;
}

int sepaihrd_mh_history_length(const sepaihrd_mh* mh) { return mh ? mh->rows : 0; }

int sepaihrd_mh_evaluate_current(sepaihrd_mh* mh, double* loglik, int32_t* status) {
    MH_ENTER(mh, loglik);
    return mh_eval(mh, mh->st.x, loglik, status);
}

int sepaihrd_mh_propose(sepaihrd_mh* mh, const double* z, const double* scale, double* loglik, int32_t* status) {
    MH_ENTER(mh, z && scale);
    const size_t CP = (size_t)mh->st.C * mh->st.P;
    HIP_TRY(hipMemcpyAsync(mh->d_z, z, CP * sizeof(double), hipMemcpyHostToDevice, mh->stream), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpyAsync(mh->d_scale, scale, (size_t)mh->st.C * sizeof(double), hipMemcpyHostToDevice, mh->stream), ctx,
            return SEPAIHRD_E_HIP);
    MH_LAUNCH_TRY(mh_launch_propose(mh, mh->d_z, mh->d_scale, mh->stream), "mh_propose: launch failed");
    if (!loglik)  // launch only: the caller overlaps host work and calls sepaihrd_mh_fetch
        return mh_eval_device(mh, mh->st.prop);
    return mh_eval(mh, mh->st.prop, loglik, status);
}

double* sepaihrd_mh_staging_buffer(sepaihrd_mh* mh) { return mh ? mh->h_stage[mh->stage_turn] : nullptr; }

int sepaihrd_mh_stage_normals(sepaihrd_mh* mh, const double* z) {
    MH_ARGS(mh, z);
    if (z == mh->h_stage[mh->stage_turn]) mh->stage_turn ^= 1;  // page-locked source: a real DMA; the next fill goes to the other buffer
    MH_ON_DEVICE();
    const size_t CP = (size_t)mh->st.C * mh->st.P;
    HIP_TRY(hipMemcpyAsync(mh->d_z_stage, z, CP * sizeof(double), hipMemcpyHostToDevice, mh->copy_stream), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipEventRecord(mh->ev_staged, mh->copy_stream), ctx, return SEPAIHRD_E_HIP);
    mh->staged = true;
    return SEPAIHRD_OK;
}

int sepaihrd_mh_step(sepaihrd_mh* mh, const uint8_t* accept, const double* scale, const int32_t* patch_chain, const double* patch_z,
                     int n_patch, double gamma, int adapt) {
    MH_ARGS(mh, scale && n_patch >= 0 && (n_patch == 0 || (patch_chain && patch_z)) && adapt >= 0 && adapt <= 3);
    const int C = mh->st.C, P = mh->st.P;
    if (!mh->staged) MH_REFUSE("mh_step: no staged normals (call sepaihrd_mh_stage_normals first)");
    if (n_patch > C) MH_REFUSE("mh_step: more patched rows than chains");
    for (int k = 0; k < n_patch; ++k)
        if (patch_chain[k] < 0 || patch_chain[k] >= C) MH_REFUSE("mh_step: patched chain out of range");
    if (accept && mh->rows >= mh->iterations) MH_REFUSE("mh_step: more states than the sampler was created for");
    MH_ON_DEVICE();
    hipStream_t st = mh->stream;
    const lay::Pack &h = mh->h_pack, &d = mh->d_pack;
    // one upload: accept flags, scales, and the patched chains with their rows
    if (accept) std::memcpy(h.accept, accept, (size_t)C);
    std::memcpy(h.scale, scale, (size_t)C * sizeof(double));
    if (n_patch > 0) {
        std::memcpy(h.chain, patch_chain, (size_t)n_patch * sizeof(int32_t));
        // patch_z is a full [C][P] array of which the listed chains' rows are valid: gathered straight into the upload
        for (int k = 0; k < n_patch; ++k)
            std::memcpy(h.rows + (size_t)k * P, patch_z + (size_t)patch_chain[k] * P, (size_t)P * sizeof(double));
    }
    HIP_TRY(hipMemcpyAsync(d.accept, h.accept, lay::pack_sent_bytes((size_t)C, (size_t)P, (size_t)n_patch), hipMemcpyHostToDevice, st), ctx,
            return SEPAIHRD_E_HIP);
    int rc = 0;
    if (accept) {
        rc = mh_before_commit(mh);
        if (rc == 0) rc = sampler_commit(mh->st, d.accept, mh->rows, st);
        if (rc == 0) mh->rows++;
    }
    if (rc == 0) rc = mh_adapt_step(mh, gamma, adapt);
    MH_LAUNCH_TRY(rc, "mh_step: launch failed");
    HIP_TRY(hipStreamWaitEvent(st, mh->ev_staged, 0), ctx, return SEPAIHRD_E_HIP);  // the staged normals have landed
    rc = sampler_patch_normals(mh->d_z_stage, d.chain, d.rows, n_patch, P, st);
    if (rc == 0) rc = mh_launch_propose(mh, mh->d_z_stage, d.scale, st);
    MH_LAUNCH_TRY(rc, "mh_step: launch failed");
    return mh_proposal_queued(mh);
}

int sepaihrd_mh_fetch(sepaihrd_mh* mh, double* loglik, int32_t* status) {
    MH_ENTER(mh, loglik);
    return mh_fetch_values(mh, loglik, status);
}

int sepaihrd_mh_set_values(sepaihrd_mh* mh, const double* values) {
    MH_ENTER(mh, values);
    const size_t bytes = (size_t)mh->st.C * sizeof(double);
    HIP_TRY(hipMemcpy(mh->d_lp, values, bytes, hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpy(mh->d_best_lp, values, bytes, hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    if (mh->st.lp_store)  // the value of sample 0 (:266-268)
        HIP_TRY(hipMemcpy2D(mh->st.lp_store, (size_t)mh->st.n_store * sizeof(double), values, sizeof(double), sizeof(double), (size_t)mh->st.C,
                            hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    mh->values_set = true;
    return SEPAIHRD_OK;
}

double* sepaihrd_mh_test_buffer(sepaihrd_mh* mh) { return mh ? mh->h_test.log_u : nullptr; }

int sepaihrd_mh_seed_streams(sepaihrd_mh* mh, uint32_t seed0) {
    MH_ENTER(mh, true);
    if (const int rc = mh_require_matching_libm(mh, "mh_seed_streams")) return rc;
    MH_LAUNCH_TRY(sampler_seed_streams(mh->st, seed0, mh->stream), "mh_seed_streams: launch failed");
    HIP_TRY(hipStreamSynchronize(mh->stream), ctx, return SEPAIHRD_E_HIP);
    mh->device_rng = true;
    return SEPAIHRD_OK;
}

int sepaihrd_mh_keep_scale_on_device(sepaihrd_mh* mh, int adapt_scale, double target_rate, int keep_trace) {
    MH_ENTER(mh, true);
    if (mh->rows > 1)
        MH_REFUSE("mh_keep_scale_on_device: call it before the first iteration (the accept window and the sample values start with the run)");
    if (adapt_scale)  // global_scale_ = exp(log_scale_) on the device
        if (const int rc = mh_require_matching_libm(mh, "mh_keep_scale_on_device")) return rc;
    SamplerState& st = mh->st;
    const size_t C = (size_t)st.C;
    {   // what this call adds to the sampler's state (sepaihrd_mh_create budgeted the rest): say so before failing inside
        const double need = (double)C * (1000.0 + 16.0 + 16.0) + (st.n_store > 0 && !st.lp_store ? (double)C * st.n_store * 8.0 : 0.0) +
                            (keep_trace && mh->iterations > 1 && !st.trace ? (double)C * (double)(mh->iterations - 1) : 0.0);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > (double)free_b) {
            char msg[256];
            std::snprintf(msg, sizeof(msg), "mh_keep_scale_on_device: the accept window, the sample values and %s need %.3f GB but %.3f GB "
                          "of device memory are free", keep_trace ? "the accept trace (C * (iterations - 1) bytes)" : "no trace",
                          need / 1e9, (double)free_b / 1e9);
            ctx->last_error = msg;
            return SEPAIHRD_E_HIP;
        }
    }
    auto dalloc = [&](void** p, size_t bytes) -> bool {
        return *p != nullptr || mh->allocs.bytes(p, bytes);  // each array once, never again
    };
    bool ok = dalloc((void**)&st.log_scale, C * sizeof(double)) && dalloc((void**)&st.scale, C * sizeof(double)) &&
              dalloc((void**)&st.recent, C * 1000) && dalloc((void**)&st.recent_meta, C * 4 * sizeof(int32_t));
    if (ok && st.n_store > 0) ok = dalloc((void**)&st.lp_store, C * st.n_store * sizeof(double));
    if (ok && keep_trace && mh->iterations > 1) ok = dalloc((void**)&st.trace, C * (size_t)(mh->iterations - 1));
    if (!ok) { ctx->last_error = "mh_keep_scale_on_device: device allocation failed"; return SEPAIHRD_E_HIP; }
    std::vector<double> ones(C, 1.0);
    HIP_TRY(hipMemset(st.log_scale, 0, C * sizeof(double)), ctx, return SEPAIHRD_E_HIP);            // log_scale_ = 0, global_scale_ = 1 (:252-253)
    HIP_TRY(hipMemcpy(st.scale, ones.data(), C * sizeof(double), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemset(st.recent, 0, C * 1000), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemset(st.recent_meta, 0, C * 4 * sizeof(int32_t)), ctx, return SEPAIHRD_E_HIP);
    if (st.trace) HIP_TRY(hipMemset(st.trace, 0, C * (size_t)(mh->iterations - 1)), ctx, return SEPAIHRD_E_HIP);
    if (st.lp_store && mh->values_set && mh->rows <= 1)  // called after sepaihrd_mh_set_values: sample 0's value is the chain's current one
        HIP_TRY(hipMemcpy2D(st.lp_store, (size_t)st.n_store * sizeof(double), mh->d_lp, sizeof(double), sizeof(double), C, hipMemcpyDeviceToDevice),
                ctx, return SEPAIHRD_E_HIP);
    st.adapt_scale = adapt_scale ? 1 : 0; st.target_rate = target_rate; st.device_scale = 1;
    return SEPAIHRD_OK;
}

int sepaihrd_mh_read_run_state(sepaihrd_mh* mh, double* values, double* best_values, double* scales, int32_t* accepted, int32_t* emergency) {
    MH_ARGS(mh, true);
    if (const int rc = mh_read(mh)) return rc;
    const size_t C = (size_t)mh->st.C;
    if (values) HIP_TRY(hipMemcpy(values, mh->d_lp, C * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (best_values) HIP_TRY(hipMemcpy(best_values, mh->d_best_lp, C * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (scales) {
        if (!mh->st.scale) MH_REFUSE("mh_read_run_state: the scale is not kept on the device");
        HIP_TRY(hipMemcpy(scales, mh->st.scale, C * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    }
    if (accepted) HIP_TRY(hipMemcpy(accepted, mh->st.accepted, C * sizeof(int32_t), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    if (emergency) {
        if (!mh->st.recent_meta) MH_REFUSE("mh_read_run_state: the scale is not kept on the device");
        HIP_TRY(hipMemcpy2D(emergency, sizeof(int32_t), mh->st.recent_meta + 3, 4 * sizeof(int32_t), sizeof(int32_t), C, hipMemcpyDeviceToHost), ctx,
                return SEPAIHRD_E_HIP);
    }
    return SEPAIHRD_OK;
}

// Progress reports and checkpoints of a run whose iterations are queued ahead (MetropolisHastingsSampler.cpp:363-383 reads the
// chain's value, best value, acceptance count, scale and -- for posterior_trace_checkpoint.csv -- its newest samples every
// report_interval iterations).  Reading them with the synchronous getters would drain the queue.
int sepaihrd_mh_snapshot_begin(sepaihrd_mh* mh, const int32_t* chains, int n, int first_sample, int count) {
    MH_ARGS(mh, chains && n > 0 && first_sample >= 0 && count >= 0);
    const int C = mh->st.C;
    if (mh->snap_pending) MH_REFUSE("mh_snapshot_begin: the previous snapshot has not been collected (sepaihrd_mh_snapshot_end)");
    if (!mh->values_set) MH_REFUSE("mh_snapshot_begin: the chains' values are unknown (sepaihrd_mh_set_values)");
    if (count > 0 && first_sample + count > sepaihrd_mh_sample_count(mh)) MH_REFUSE("mh_snapshot_begin: beyond the samples stored so far");
    for (int k = 0; k < n; ++k)
        if (chains[k] < 0 || chains[k] >= C) MH_REFUSE("mh_snapshot_begin: chain out of range");
    MH_ON_DEVICE();
    if (!mh->snap_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&mh->snap_stream, hipStreamNonBlocking), ctx, return SEPAIHRD_E_HIP);
        HIP_TRY(hipEventCreateWithFlags(&mh->ev_snap_gathered, hipEventDisableTiming), ctx, return SEPAIHRD_E_HIP);
        HIP_TRY(hipEventCreateWithFlags(&mh->ev_snap_done, hipEventDisableTiming), ctx, return SEPAIHRD_E_HIP);
    }
    const size_t need = (size_t)n * lay::snapshot_width((size_t)mh->st.P, (size_t)count);
    if (need > mh->snap_cap) {  // the previous snapshot has been collected: nothing reads the old buffers any more
        mh->snap_cap = 0;
        ALLOC_TRY(mh->snap_dev.get(&mh->d_snap, need), ctx, return SEPAIHRD_E_HIP);
        ALLOC_TRY(mh->snap_host.get(&mh->h_snap, need), ctx, return SEPAIHRD_E_HIP);
        mh->snap_cap = need;
    }
    if ((size_t)n > mh->snap_chain_cap) {
        mh->snap_chain_cap = 0;
        mh->snap_chain_list.clear();
        ALLOC_TRY(mh->snap_chains_dev.get(&mh->d_snap_chains, (size_t)n), ctx, return SEPAIHRD_E_HIP);
        mh->snap_chain_cap = (size_t)n;
    }
    // the chain list is uploaded when it changes (every report of a run names the same chains): a blocking copy once, none after
    if (mh->snap_chain_list.size() != (size_t)n || !std::equal(chains, chains + n, mh->snap_chain_list.begin())) {
        HIP_TRY(hipMemcpy(mh->d_snap_chains, chains, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice), ctx, return SEPAIHRD_E_HIP);
        mh->snap_chain_list.assign(chains, chains + n);
    }
    MH_LAUNCH_TRY(sampler_snapshot(mh->st, mh->d_lp, mh->d_best_lp, mh->d_snap_chains, n, first_sample, count, mh->d_snap, mh->stream),
                  "mh_snapshot_begin: launch failed");
    HIP_TRY(hipEventRecord(mh->ev_snap_gathered, mh->stream), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipStreamWaitEvent(mh->snap_stream, mh->ev_snap_gathered, 0), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipMemcpyAsync(mh->h_snap, mh->d_snap, need * sizeof(double), hipMemcpyDeviceToHost, mh->snap_stream), ctx, return SEPAIHRD_E_HIP);
    HIP_TRY(hipEventRecord(mh->ev_snap_done, mh->snap_stream), ctx, return SEPAIHRD_E_HIP);
    mh->snap_n = n; mh->snap_count = count; mh->snap_pending = true;
    return SEPAIHRD_OK;
}

// returns 1 while the snapshot has not landed (wait == 0 only), 0 with the outputs filled, < 0 on error.  May be called from
// another host thread than the one that queues the iterations (it touches the snapshot's own event and buffer only).
int sepaihrd_mh_snapshot_end(sepaihrd_mh* mh, int wait, double* state, double* samples, double* sample_values) {
    if (!mh) return SEPAIHRD_E_INVALID_ARG;
    if (!mh->snap_pending) return SEPAIHRD_E_INVALID_ARG;
    if (hipSetDevice(mh->ctx->device) != hipSuccess) return SEPAIHRD_E_HIP;
    if (!wait) {
        const hipError_t q = hipEventQuery(mh->ev_snap_done);
        if (q == hipErrorNotReady) return 1;
        if (q != hipSuccess) return SEPAIHRD_E_HIP;
    } else if (hipEventSynchronize(mh->ev_snap_done) != hipSuccess) return SEPAIHRD_E_HIP;
    const size_t P = (size_t)mh->st.P, count = (size_t)mh->snap_count;
    for (int k = 0; k < mh->snap_n; ++k) {
        const lay::SnapshotRecord o = lay::snapshot_record(mh->h_snap, (size_t)k, P, count);
        if (state) std::memcpy(state + 4 * (size_t)k, o.state, 4 * sizeof(double));
        if (samples && count) std::memcpy(samples + (size_t)k * count * P, o.samples, count * P * sizeof(double));
        if (sample_values && count) std::memcpy(sample_values + (size_t)k * count, o.sample_values, count * sizeof(double));
    }
    mh->snap_pending = false;
    return SEPAIHRD_OK;
}

int sepaihrd_mh_read_failure_counts(sepaihrd_mh* mh, int64_t counts[3]) {
    if (!mh || !counts) return SEPAIHRD_E_INVALID_ARG;
    uint32_t h[3] = {0, 0, 0};
    if (const int rc = mh_read(mh, h, mh->st.fail_counts, sizeof(h))) return rc;
    for (int k = 0; k < 3; ++k) counts[k] = (int64_t)h[k];
    return SEPAIHRD_OK;
}

int sepaihrd_mh_read_sample_values(sepaihrd_mh* mh, int first, int count, double* out) {
    MH_ARGS(mh, out && first >= 0 && count > 0);
    if (!mh->st.lp_store || first + count > sepaihrd_mh_sample_count(mh))
        MH_REFUSE("mh_read_sample_values: not kept (sepaihrd_mh_keep_scale_on_device) or beyond the samples stored so far");
    if (const int rc = mh_read(mh)) return rc;
    HIP_TRY(hipMemcpy2D(out, (size_t)count * sizeof(double), mh->st.lp_store + first, (size_t)mh->st.n_store * sizeof(double),
                        (size_t)count * sizeof(double), (size_t)mh->st.C, hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_mh_read_accept_trace(sepaihrd_mh* mh, uint8_t* out) {
    MH_ARGS(mh, out);
    if (!mh->st.trace) MH_REFUSE("mh_read_accept_trace: no trace kept");
    return mh_read(mh, out, mh->st.trace, (size_t)mh->st.C * (size_t)(mh->iterations - 1));
}

int sepaihrd_mh_draw_first(sepaihrd_mh* mh) {
    MH_ARGS(mh, true);
    if (!mh->device_rng) MH_REFUSE("mh_draw_first: call sepaihrd_mh_seed_streams first");
    MH_ON_DEVICE();
    // proposal 1: the normals from the start of every stream, into the staged-normals buffer
    MH_LAUNCH_TRY(mh_launch_draw(mh, nullptr, 1, nullptr, mh->d_z_stage, nullptr, 1, mh->copy_stream), "mh_draw_first: launch failed");
    HIP_TRY(hipEventRecord(mh->ev_staged, mh->copy_stream), ctx, return SEPAIHRD_E_HIP);
    mh->staged = true;
    return SEPAIHRD_OK;
}

int sepaihrd_mh_step_tested(sepaihrd_mh* mh, double gamma, int adapt, int last) {
    MH_ARGS(mh, adapt >= 0 && adapt <= 3);
    if (!mh->values_set) MH_REFUSE("mh_step_tested: call sepaihrd_mh_set_values first");
    const bool self_contained = mh->device_rng && mh->st.device_scale != 0;  // nothing of the caller's goes into the test
    if (self_contained)
        if (const int rc = mh_throttle_look_ahead(mh)) return rc;
    if (mh->test_pending && !self_contained) MH_REFUSE("mh_step_tested: the previous test has not been fetched");
    if (!last && !mh->staged && !mh->device_rng) MH_REFUSE("mh_step_tested: no staged normals (call sepaihrd_mh_stage_normals first)");
    if (mh->rows >= mh->iterations) MH_REFUSE("mh_step_tested: more states than the sampler was created for");
    MH_ON_DEVICE();
    if (const int rc = mh_stage_test_inputs(mh, self_contained, adapt, last)) return rc;
    MH_LAUNCH_TRY(mh_before_commit(mh), "mh_step_tested: catch-up of the queued updates failed");
    const lay::TestInputs& in = mh->d_test;
    const SamplerTestArgs a{mh->d_fetch.loglik, mh->d_fetch.status, in.log_u, in.scale_reject, in.scale_accept, mh->d_lp, mh->d_best_lp, mh->d_scale_sel,
                            mh->d_out.flags, mh->d_out.values, mh->d_z_stage, in.z_plain, mh->lz_ready ? mh->d_lz[0] : nullptr,
                            mh->lz_ready ? mh->d_lz[1] : nullptr, mh->rows};
    if (!last && adapt <= 1) return mh_step_fused(mh, a, self_contained, gamma, adapt);
    return mh_step_split(mh, a, self_contained, gamma, adapt, last);
}

int sepaihrd_mh_fetch_test(sepaihrd_mh* mh, double* values, uint8_t* flags) {
    MH_ARGS(mh, values && flags);
    if (!mh->test_pending) MH_REFUSE("mh_fetch_test: no test pending");
    MH_ON_DEVICE();
    HIP_TRY(hipEventSynchronize(mh->ev_fetched), ctx, return SEPAIHRD_E_HIP);
    const size_t C = (size_t)mh->st.C;
    std::memcpy(values, mh->h_out.values, C * sizeof(double));
    std::memcpy(flags, mh->h_out.flags, C);
    mh->test_pending = false;
    return SEPAIHRD_OK;
}

int sepaihrd_mh_commit(sepaihrd_mh* mh, const uint8_t* accept) {
    MH_ARGS(mh, accept);
    if (mh->rows >= mh->iterations) MH_REFUSE("mh_commit: more states than the sampler was created for");
    MH_ON_DEVICE();
    MH_LAUNCH_TRY(mh_before_commit(mh), "mh_commit: catch-up of the queued updates failed");
    HIP_TRY(hipMemcpyAsync(mh->d_accept, accept, (size_t)mh->st.C, hipMemcpyHostToDevice, mh->stream), ctx, return SEPAIHRD_E_HIP);
    MH_LAUNCH_TRY(sampler_commit(mh->st, mh->d_accept, mh->rows, mh->stream), "mh_commit: launch failed");
    mh->rows++;
    return SEPAIHRD_OK;
}

int sepaihrd_mh_adapt(sepaihrd_mh* mh, double gamma, int refresh, int recompute_full) {
    MH_ENTER(mh, true);
    MH_LAUNCH_TRY(mh_adapt_step(mh, gamma, refresh ? (recompute_full ? 3 : 2) : 1), "mh_adapt: launch failed");
    return SEPAIHRD_OK;
}

int sepaihrd_mh_read_history(sepaihrd_mh* mh, const int32_t* rows, int n_rows, double* out) {
    MH_ENTER(mh, rows && n_rows > 0 && out);
    const int C = mh->st.C, P = mh->st.P, W = mh->st.window;
    for (int r = 0; r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= mh->rows || rows[r] < mh->rows - W)
            MH_REFUSE("mh_read_history: state not committed yet, or no longer among the newest `window` states "
                      "(the thinned samples are read with sepaihrd_mh_read_samples)");
    HIP_TRY(hipStreamSynchronize(mh->stream), ctx, return SEPAIHRD_E_HIP);
    // strided copies straight out of the ring: state r of every chain = a 2-D region
    for (int r = 0; r < n_rows; ++r)
        HIP_TRY(hipMemcpy2D(out + (size_t)r * P, (size_t)n_rows * P * sizeof(double),
                            mh->st.hist + (size_t)(rows[r] % W) * P, (size_t)W * P * sizeof(double),
                            (size_t)P * sizeof(double), (size_t)C, hipMemcpyDeviceToHost),
                ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_mh_sample_count(const sepaihrd_mh* mh) {
    if (!mh || mh->st.n_store <= 0 || mh->rows <= 0) return 0;
    return std::min(mh->st.n_store, (mh->rows - 1) / mh->st.thinning + 1);
}

int sepaihrd_mh_read_samples(sepaihrd_mh* mh, int first, int count, double* out) {
    MH_ARGS(mh, out && first >= 0 && count > 0);
    if (first + count > sepaihrd_mh_sample_count(mh)) MH_REFUSE("mh_read_samples: beyond the samples stored so far");
    if (const int rc = mh_read(mh)) return rc;
    const size_t P = (size_t)mh->st.P;
    HIP_TRY(hipMemcpy2D(out, (size_t)count * P * sizeof(double), mh->st.store + (size_t)first * P,
                        (size_t)mh->st.n_store * P * sizeof(double), (size_t)count * P * sizeof(double), (size_t)mh->st.C,
                        hipMemcpyDeviceToHost),
            ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_mh_summary_records(sepaihrd_mh* mh, int first_sample, double* out, double* d_out) {
    MH_ARGS(mh, out || d_out);
    const int ns = sepaihrd_mh_sample_count(mh);
    if (first_sample < 0 || first_sample >= ns) MH_REFUSE("mh_summary_records: first_sample beyond the samples stored so far");
    if (!mh->values_set) MH_REFUSE("mh_summary_records: the chains' values are unknown (sepaihrd_mh_set_values)");
    MH_ON_DEVICE();
    double* const dst = d_out ? d_out : mh->d_summary;
    MH_LAUNCH_TRY(sampler_summary_records(mh->st, mh->d_best_lp, first_sample, ns, dst, mh->stream), "mh_summary_records: launch failed");
    HIP_TRY(hipStreamSynchronize(mh->stream), ctx, return SEPAIHRD_E_HIP);
    if (out)
        HIP_TRY(hipMemcpy(out, dst, (size_t)mh->st.C * (2 * (size_t)mh->st.P + 2) * sizeof(double), hipMemcpyDeviceToHost), ctx,
                return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_mh_diagnostics(sepaihrd_mh* mh, int first_sample, int count, int with_values, double* out, int32_t* max_lag) {
    MH_ARGS(mh, true);
    if (!out) MH_REFUSE("mh_diagnostics: out is required");
    if (ctx->pending_B > 0) MH_REFUSE("mh_diagnostics: a sepaihrd_eval_batch_begin is pending on this context");
    const int ns = sepaihrd_mh_sample_count(mh);
    if (mh->st.n_store <= 0 || !mh->st.store) MH_REFUSE("mh_diagnostics: the sampler stores no samples");
    if (with_values && !mh->st.lp_store) MH_REFUSE("mh_diagnostics: no values stored (sepaihrd_mh_keep_scale_on_device)");
    if (first_sample < 0 || first_sample >= ns || (count > 0 && first_sample + count > ns))
        MH_REFUSE("mh_diagnostics: range beyond the samples stored so far");
    const int N = count > 0 ? count : ns - first_sample;
    int rc = diag_check_shape(ctx, "mh_diagnostics", mh->st.C, N, mh->st.P);
    if (rc == SEPAIHRD_OK) rc = mh_read(mh);
    if (rc != SEPAIHRD_OK) return rc;
    const size_t P = (size_t)mh->st.P, n_store = (size_t)mh->st.n_store;
    // the stored samples in place: chain stride n_store P, sample stride P; the values column [C][n_store]
    const DiagInput in{mh->st.store + (size_t)first_sample * P, n_store * P, P, mh->st.P, with_values ? mh->st.lp_store + first_sample : nullptr,
                       n_store, mh->st.C, N};
    return diag_run(ctx, "mh_diagnostics", in, out, max_lag, mh->stream);
}

int sepaihrd_mh_read_moments(sepaihrd_mh* mh, double* mean, double* m2) {
    MH_ARGS(mh, mean || m2);
    if (mh->covariance_mode != SEPAIHRD_MH_COV_RUNNING) MH_REFUSE("mh_read_moments: the sampler keeps no running sums (two-pass mode)");
    const size_t CP = (size_t)mh->st.C * mh->st.P;
    const int rc = mh_read(mh, mean, mh->st.wmean, CP * sizeof(double), +[](sepaihrd_mh* m) { return mh_flush_moments(m, 0); },
                           "mh_read_moments: catch-up failed");
    if (rc != SEPAIHRD_OK) return rc;
    if (m2) HIP_TRY(hipMemcpy(m2, mh->st.m2, CP * mh->st.P * sizeof(double), hipMemcpyDeviceToHost), ctx, return SEPAIHRD_E_HIP);
    return SEPAIHRD_OK;
}

int sepaihrd_mh_read_proposal(sepaihrd_mh* mh, double* prop) {
    if (!mh || !prop) return SEPAIHRD_E_INVALID_ARG;
    return mh_read(mh, prop, mh->st.prop, (size_t)mh->st.C * mh->st.P * sizeof(double));
}

int sepaihrd_mh_read_best(sepaihrd_mh* mh, double* best) {
    if (!mh || !best) return SEPAIHRD_E_INVALID_ARG;
    return mh_read(mh, best, mh->st.best, (size_t)mh->st.C * mh->st.P * sizeof(double));
}

int sepaihrd_mh_busy(sepaihrd_mh* mh) {
    if (!mh) return 0;
    return hipStreamQuery(mh->stream) == hipErrorNotReady ? 1 : 0;
}

int sepaihrd_mh_read_covariance(sepaihrd_mh* mh, double* cov) {
    if (!mh || !cov) return SEPAIHRD_E_INVALID_ARG;
    return mh_read(mh, cov, mh->st.cov, (size_t)mh->st.C * mh->st.P * mh->st.P * sizeof(double), mh_flush_rank1,
                   "mh_read_covariance: rank-one catch-up failed");
}

}  // extern "C"
