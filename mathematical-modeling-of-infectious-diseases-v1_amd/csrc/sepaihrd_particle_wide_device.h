// csrc/sepaihrd_particle_wide_device.h -- what csrc/sepaihrd_capi.cpp (sepaihrd_particle_loglik_wide) and
// csrc/sepaihrd_particle_wide.hip (the wide form of the bootstrap particle filter: its kernels, its launch plan and the probe of
// one row's normalisation and resampling) share.  DESIGN.md section 6l.  The rules are csrc/sepaihrd_particle.inc, the decode
// from theta to model values is launch_stoch_epi_decode (csrc/sepaihrd_stoch_sepaihrd_device.h), both unchanged.
//
// The particles of a chunk of thetas live in device memory, in scratch the caller owns.  Per theta of the chunk and particle
// (lpc = n_age rounded up to a power of two):
//     2 x 11 counts x 4 bytes x lpc      the two copies of the state, int32 [copy][b][11][J][lpc]
//     8                                  lw, double [b][J]
//     4 x 8                              the prefix sums C and Q, each twice (the scans ping-pong), double [b][J]
//     4                                  the ancestor, int32 [b][J]
// so particle_wide_scratch_bytes(lpc, J, chunk) = chunk J (88 lpc + 44).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_device.h"
#include "sepaihrd_particle_device.h"

namespace sepaihrd {

constexpr int PARTICLE_WIDE_MAX_J = 65536;
constexpr size_t PARTICLE_WIDE_AUTO_SCRATCH = (size_t)1 << 30;  // theta_chunk = 0: as many thetas as keep the scratch within this
constexpr size_t particle_wide_scratch_bytes(int lpc, int J, size_t chunk) {
    return chunk * (size_t)J * ((size_t)2 * NUM_COMP * 4 * (size_t)lpc + 8 + 4 * 8 + 4);
}
// the thetas per chunk: theta_chunk where it is positive, else the automatic choice; never more than B, never fewer than one
constexpr size_t particle_wide_chunk(int lpc, int J, int B, int theta_chunk) {
    size_t c = theta_chunk > 0 ? (size_t)theta_chunk : PARTICLE_WIDE_AUTO_SCRATCH / particle_wide_scratch_bytes(lpc, J, 1);
    c = c < 1 ? 1 : c;
    return c < (size_t)B ? c : (size_t)B;
}

// where count c of (theta bl of a chunk of Bc, particle p, age) lies in copy `copy` of the state: int32 [copy][b][11][J][lpc]
constexpr size_t particle_wide_state_index(int Bc, int J, int lpc, int copy, int bl, int c, int p, int age) {
    return ((((size_t)copy * Bc + bl) * NUM_COMP + c) * (size_t)J + p) * lpc + age;
}

struct ParticleStatesArgs;  // csrc/sepaihrd_particle_states_device.h

// the arguments of the LDS filter's negative-binomial launch and what the wide form needs beside them.  Host only: the kernels take
// their own records.  row_const null: the Poisson path, the k are not read.
struct ParticleWideArgs : ParticleArgsNB {
    size_t chunk;             // thetas per chunk (particle_wide_chunk)
    void* scratch;            // device, particle_wide_scratch_bytes(lpc, J, chunk) bytes, 8-byte aligned
    const double* host_grid;  // [T][lpc][4] HOST copy of DevProblem::grid: which rows are weighted is planned from it
    // sepaihrd_particle_filter_states alone, null in every other call: every output row ends a segment and
    // launch_particle_states_row summarises the row's cloud
    ParticleStatesArgs* states;
};
// The whole filter as plain launches on the stream, chunk after chunk: a fill of the outputs, then per segment one
// propagate-and-weight launch and, where the segment ends in a weighted row, one normalise-and-resample launch; the final state
// last.  With ParticleWideArgs::states a segment is one row and the row's summary follows its launches.  No synchronisation inside.  0, -3 (a launch failed) or -4 (arguments).
int launch_particle_filter_wide(const DevProblem& pb, const ParticleWideArgs& a, void* stream);

}  // namespace sepaihrd
