// csrc/sepaihrd_mh_backend.h -- what the device-resident sampler (sepaihrd_mh, csrc/sepaihrd_mh_capi.cpp) needs of the context
// it samples on, and the packed small-P form of its per-iteration kernels (csrc/sepaihrd_sampler.hip).  Internal: not part of
// the C ABI.  Two contexts make samplers: sepaihrd_ctx (sepaihrd_mh_create) and sepaihrd_sir_ctx (sepaihrd_sir_mh_create).
#pragma once
#include <stdint.h>

#include <string>

#include "sepaihrd_device.h"

struct sepaihrd_ctx;
struct sepaihrd_sir_ctx;
struct sepaihrd_mh;
struct sepaihrd_mh_config;

namespace sepaihrd {

// The record between a sampler and its context.  The members that are references name fields of the context itself, so
// that what the sampler writes (the error text, the result of the libm self-check) is read through the context's own entry
// points, and what the context changes later (DevProblem::constraint_mode) is seen by the next proposal.
struct MhBackend {
    int device;
    int P;
    std::string& last_error;
    // lower / upper / has_bounds / constraint_mode as constrain() of the propose kernels reads them, and lpc (chains per
    // evaluation wave: where the draws queue behind the evaluation).  The SEPAIHRD context's own problem; a SIR context
    // keeps a record of which only these fields are set.
    const DevProblem& dp;
    int& libm_log_diff;
    int& libm_exp_diff;
    const int& pending_B;      // a host-pointer evaluation begun on the context and not collected yet (SEPAIHRD only)
    sepaihrd_ctx* sep;         // exactly one of the two is set
    sepaihrd_sir_ctx* sir;
};

// sepaihrd_mh_create's body over either context (csrc/sepaihrd_mh_capi.cpp)
sepaihrd_mh* mh_create_on(const MhBackend& be, const sepaihrd_mh_config* cfg, const double* x0, const double* cov0);
// sepaihrd_device_libm_check's body: runs the self-check once per context (diffs < 0: not run yet)
int device_libm_check(int device, std::string& last_error, int& log_diff, int& exp_diff, int32_t* n_log_diff, int32_t* n_exp_diff);

// What a sampler needs of a SEPAIHRD context beyond the record, defined beside the context (csrc/sepaihrd_capi.cpp): the record
// itself, and the context's bookkeeping of the streams it has launched on (fence_before / fence_after there).  Between the
// library's own translation units only: not among its dynamic symbols.
#pragma GCC visibility push(hidden)
MhBackend mh_backend_of(sepaihrd_ctx* ctx);
// a sampler's stream is now the context's lazy stream: launches after the first on it record no event
void ctx_adopt_lazy_stream(sepaihrd_ctx* ctx, void* stream);
// the context forgets this (drained) stream before it is destroyed
void ctx_forget_stream(sepaihrd_ctx* ctx, void* stream);
#pragma GCC visibility pop

// ---- packed form: a chain is a group of G = pow2(P) adjacent lanes, 64 / G chains per wavefront (P <= 64) ----
constexpr int MH_PACKED_MAX_P = 64;
inline int mh_packed_group(int P) {
    int g = 1;
    while (g < P) g <<= 1;
    return g;
}
// the fields of DevProblem that constrain() reads: the packed kernels take these 32 bytes instead of the whole problem
struct MhBounds {
    const double* lower;
    const double* upper;
    const int32_t* has_bounds;
    int32_t constraint_mode;
};
inline MhBounds mh_bounds_of(const DevProblem& pb) { return MhBounds{pb.lower, pb.upper, pb.has_bounds, pb.constraint_mode}; }
// same arguments, same results (bit for bit) as sampler_propose / sampler_propose_select / sampler_lz /
// sampler_test_commit_propose; -4 for P > MH_PACKED_MAX_P
int sampler_propose_packed(const SamplerState& s, const MhBounds& b, const double* d_z, const double* d_scale, void* stream);
int sampler_propose_select_packed(const SamplerState& s, const MhBounds& b, const double* d_z_uniform, const double* d_z_plain,
                                  const uint8_t* d_flags, const double* d_scale, void* stream);
// sampler_draw in the packed form: a lane per chain over the window of words a proposal touches, the block-per-chain kernel
// for the chains whose window leaves the stored state (d_todo: [C] bytes of scratch).  Same values, same words consumed.
int sampler_draw_packed(const SamplerState& s, const uint8_t* d_flags, int first, double* d_log_u, double* d_z_uniform, double* d_z_plain,
                        int want_normals, uint8_t* d_todo, void* stream);
int sampler_lz_packed(const SamplerState& s, const double* d_z_uniform, const double* d_z_plain, double* d_lz_uniform, double* d_lz_plain,
                      void* stream);
int sampler_test_commit_propose_packed(const SamplerState& s, const MhBounds& b, const SamplerTestArgs& a, void* stream);

}  // namespace sepaihrd
