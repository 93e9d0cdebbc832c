// csrc/sepaihrd_particle_states.inc -- the per-row summaries of the bootstrap particle filter (sepaihrd_particle_filter_states;
// DESIGN.md section 6n) as one text for host and device: the filtered state means and quantile bands of every output row.
// The filter itself is csrc/sepaihrd_particle.inc, untouched: the weights, M, the scans, the ESS, the resampling uniform, the
// ancestors, the skipped rows and the negative-binomial row constants are sections 6k's and 6m's.
//
// The summarised set.  Every output row k in 0 .. T - 1, run-up rows included, is summarised over the J particles the next
// interval starts from: after a weighted row slot i holds the state of anc[i] (the filter resamples at every weighted row, so the
// set is equally weighted); after an unweighted row (run-up, blank row) the particles as propagated.  Row T - 1 is therefore the
// set final_state holds.
//
// The series.  For each of the 11 counts c one series per age class a in 0 .. n - 1 and one more at index n: the particle's sum
// over its n age classes, formed in integers.
//
// The mean.  mean[k][c][a] = (double)(sum_j count_j) / (double)J with the sum in 64-bit integers: exact and independent of the
// order of the additions (2^31 x 65 536 x 16 < 2^53).
//
// The quantiles.  For each probability p of the caller's list, the rule of csrc/sepaihrd_quantile.inc over the J values sorted
// ascending, as the ensemble summaries and the predictive twin apply it.  The values are integers below 2^35; sorting them as
// integers and converting the two picked ones is sorting them as doubles.
//
// An invalid theta has NaN everywhere.
// Included by csrc/sepaihrd_particle_states.hip and by the host library (host/src/HipParticleFilter.cpp), contraction off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_particle.inc"
#include "sepaihrd_quantile.inc"

namespace sepaihrd_particle_states {

constexpr int MAX_PROBS = 64;  // probabilities per call

SEP_RNG_FN double mean_of(int64_t sum, int J) { return (double)sum / (double)J; }

// a probability the call takes: in [0, 1] (a NaN fails both comparisons)
SEP_RNG_FN bool probability_ok(double p) { return p >= 0.0 && p <= 1.0; }

}  // namespace sepaihrd_particle_states
