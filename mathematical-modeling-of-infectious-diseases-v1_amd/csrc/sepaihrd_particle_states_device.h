// csrc/sepaihrd_particle_states_device.h -- what csrc/sepaihrd_capi.cpp (sepaihrd_particle_filter_states),
// csrc/sepaihrd_particle_wide.hip (the launch plan that calls the summary after every row) and
// csrc/sepaihrd_particle_states.hip (the summary kernels) share.  DESIGN.md section 6n; the rule is
// csrc/sepaihrd_particle_states.inc.
//
// Scratch.  The wide form's scratch (csrc/sepaihrd_particle_wide_device.h) plus, per theta of a chunk, the row table
//     11 x (n_age + 1) x pad x 8 bytes     double [b][11][n_age + 1][pad], pad = particle_states_pad(J)
// so particle_states_scratch_bytes(lpc, n, J, chunk) = chunk (J (88 lpc + 44) + 88 (n + 1) pad).  The table is sorted in place
// (in LDS up to ENSEMBLE_MAX_SAMPLES values, in the table itself beyond) and the sums are formed by the workgroup that sorts:
// there is no table of sums and no sort scratch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_device.h"
#include "sepaihrd_particle_wide_device.h"

namespace sepaihrd {

// doubles between two segments of the row table: the power of two >= max(J, 64) -- plan_segments' pad up to
// ENSEMBLE_MAX_SAMPLES, and a power of two beyond it as well, which the in-place bitonic sort needs
constexpr size_t particle_states_pad(int J) {
    size_t pad = WAVE;
    while (pad < (size_t)J) pad <<= 1;
    return pad;
}
constexpr size_t particle_states_table_doubles(int n, int J, size_t chunk) { return chunk * NUM_COMP * (size_t)(n + 1) * particle_states_pad(J); }
constexpr size_t particle_states_scratch_bytes(int lpc, int n, int J, size_t chunk) {
    return particle_wide_scratch_bytes(lpc, J, chunk) + sizeof(double) * particle_states_table_doubles(n, J, chunk);
}
// particle_wide_chunk with the row table counted
constexpr size_t particle_states_chunk(int lpc, int n, int J, int B, int theta_chunk) {
    size_t c = theta_chunk > 0 ? (size_t)theta_chunk : PARTICLE_WIDE_AUTO_SCRATCH / particle_states_scratch_bytes(lpc, n, J, 1);
    c = c < 1 ? 1 : c;
    return c < (size_t)B ? c : (size_t)B;
}

// What launch_particle_filter_wide needs to summarise every row (ParticleWideArgs::states).  Host only.
struct ParticleStatesArgs {
    int n_probs;              // 0 .. 64
    const double* probs;      // device [n_probs]
    double* table;            // device, particle_states_table_doubles(n, J, chunk) doubles
    double* state_mean;       // device [B][T][11][n + 1]
    double* state_quantiles;  // device [B][T][11][n + 1][n_probs] or null
    void* const* ev;          // n_ev events, or null: the i-th summary of the call's FIRST chunk records ev[2 i] before and ev[2 i + 1] after
    size_t n_ev;
    size_t used_ev;           // events recorded so far: the launch advances it
};

// Once per call, before the first row: raises the sort kernel's dynamic-LDS limit where a segment of J values needs more than
// 48 KiB.  0 or -3.
int prepare_particle_states(int J);

// The cloud after output row k of one chunk (thetas b0 .. b0 + Bc - 1 of the call) into the row's slice of the outputs: the
// gather launch and the sort-and-pick launch, on the stream.  `state`, `anc`, `status` are the chunk's; the cloud is copy `cur`,
// through anc where `gather`.  0, -3 (a launch failed) or -4 (arguments).
int launch_particle_states_row(const DevProblem& pb, ParticleStatesArgs& a, int Bc, size_t b0, int J, int k, int cur, int gather,
                               const int32_t* state, const int32_t* anc, const int32_t* status, void* stream);

}  // namespace sepaihrd
