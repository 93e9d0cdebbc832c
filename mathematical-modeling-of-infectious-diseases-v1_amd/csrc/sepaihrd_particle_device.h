// csrc/sepaihrd_particle_device.h -- what csrc/sepaihrd_capi.cpp (sepaihrd_particle_loglik) and csrc/sepaihrd_particle.hip (the
// filter kernel and the probe of one row's normalisation and resampling) share.  The decode from theta to model values is
// launch_stoch_epi_decode (csrc/sepaihrd_stoch_sepaihrd_device.h), unchanged.
//
// The J limit.  One workgroup of PARTICLE_BLOCK = 512 lanes (8 wavefronts: what the 213 registers of the model step leave room
// for on one CU) holds every particle of its theta in LDS, twice, because a resampled slot is read from one copy and written to
// the other.  Per particle and lane-per-chain slot (lpc = n_age rounded up to a power of two):
//     2 x (11 counts + 3 previous-row values) x 4 bytes = 112 lpc bytes
// and per particle 28 bytes more: lw (8), the prefix sums C (8) and Q (8), the ancestor (4); 64 bytes hold the waves' maxima.
// The block stays inside the 64 KiB every HIP launch may ask for without opting in (the CU's LDS is 160 KiB, so two blocks of
// J up to that limit still share a CU), less 448 bytes left to the static LDS of the block-wide vote (256 bytes in this build):
//     sepaihrd_particle_max_particles(n) = min(512, (65536 - 512) / (112 lpc + 28))  = 464, 258, 136, 70, 35 for lpc = 1 .. 16.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_device.h"

namespace sepaihrd {

constexpr int PARTICLE_BLOCK = 512;
constexpr size_t PARTICLE_LDS_LIMIT = 65536 - 448, PARTICLE_LDS_FIXED = 64;  // of the dynamic allocation
constexpr size_t particle_lds_bytes(int lpc, int J) {
    return PARTICLE_LDS_FIXED + (size_t)J * ((size_t)2 * (NUM_COMP + 3) * 4 * (size_t)lpc + 28);
}
constexpr int particle_max_particles_for(int lpc) {
    const size_t j = (PARTICLE_LDS_LIMIT - PARTICLE_LDS_FIXED) / ((size_t)2 * (NUM_COMP + 3) * 4 * (size_t)lpc + 28);
    return j < (size_t)PARTICLE_BLOCK ? (int)j : PARTICLE_BLOCK;
}

struct ParticleArgs {
    int B, J, m, W;           // thetas, particles per theta, steps per output interval, width of a model-values row
    uint64_t seed;
    const double* values;     // [B][W] device: launch_stoch_epi_decode's rows
    const int32_t* status;    // [B] device: 0, or SEPAIHRD_STATUS_INVALID
    double* loglik;           // [B] device
    double* increments;       // [B][Tp] device or null
    double* ess;              // [B][Tp] device or null
    double* final_state;      // [B][J][11][n] device or null
};
// one workgroup per theta: propagate, weight, scan and resample without leaving the device between output rows
int launch_particle_filter(const DevProblem& pb, const ParticleArgs& a, void* stream);

// The negative-binomial observation model: the arguments above and, for the kernel's dispersed
// instantiation alone, the three k (+inf: that series stays Poisson; at least one finite) and the row constants.
struct ParticleArgsNB : ParticleArgs {
    double k_H, k_ICU, k_D;
    const double* row_const;  // [Tp] device: G of every output time >= 0, added by lane 0 to the row's increment
};
int launch_particle_filter_nb(const DevProblem& pb, const ParticleArgsNB& a, void* stream);

}  // namespace sepaihrd
