// csrc/sepaihrd_adapt_scale.inc -- the Robbins-Monro rule of the global proposal scale (MetropolisHastingsSampler::adaptGlobalScale,
// MetropolisHastingsSampler.cpp:104-152) as ONE text for host and device: adapt_global_scale of csrc/sepaihrd_sampler.hip,
// MultiChainMetropolisHastings::run and the device-resident host loop (its look-ahead candidates and its bookkeeping) all compile
// these functions.  The tests demand that the three agree bit for bit; with one text they cannot part.  oracle/sepaihrd_oracle.hpp
// keeps its own statement: it is the independent side of that comparison.
// exp() of the new log-scale stays with the caller (sepaihrd_rng::glibc_exp on the device, std::exp on the host;
// sepaihrd_device_libm_check guards that the two are one function).
// Contraction: every includer is built with -ffp-contract=off (csrc/Makefile's sampler.o, host/Makefile); `ls += g * (...)` fused
// into one operation would round differently from the reference's two.
#pragma once

#if defined(__HIPCC__)
#define SEP_ADAPT_FN __host__ __device__ __forceinline__
#else
#define SEP_ADAPT_FN inline
#endif

#define SEP_ADAPT_WINDOW 1000  // recent_accepts_ holds the last 1000 flags (:107-110)

// The window once `accepted` is pushed: push_back, pop_front beyond 1000 (:107-110).  The window is a byte ring the caller owns,
// with its write position, its length and the running sum of its flags.  window_after_push leaves ring and position alone (the
// look-ahead asks for both outcomes of a test that has not run yet).
SEP_ADAPT_FN void window_after_push(const unsigned char* ring, const int pos, const bool accepted, int& len, int& sum) {
    if (len == SEP_ADAPT_WINDOW) sum -= ring[pos]; else ++len;
    sum += accepted ? 1 : 0;
}
SEP_ADAPT_FN void window_push(unsigned char* ring, int& pos, int& len, int& sum, const bool accepted) {
    window_after_push(ring, pos, accepted, len, sum);
    ring[pos] = accepted ? 1 : 0;
    pos = (pos + 1) % SEP_ADAPT_WINDOW;
}

// The new log_scale_: next_log_scale, below its two halves.  The three branches (:112-141) from the current log_scale_, the window's
// sum and length AFTER the push, the flag pushed, the step and the target rate -- *emergency says whether the emergency branch
// (:118-123) fired -- then the recovery from the floor (:146-148, on global_scale_ BEFORE this update) and the clamp to [-6.9, 2.3].
// The host calls the whole; the device kernel calls the halves and loads global_scale_ between them, where the reference reads it
// (loaded ahead of the branches it stays live across their square root and division: two more registers in three kernels).
// The (a < b) ? a : b forms equal std::min / std::max for every operand that is not a NaN.
SEP_ADAPT_FN double log_scale_step(const double log_scale, const int sum, const int len, const bool accepted, const int step,
                                   const double target, bool* emergency) {
    const double rate = (double)sum / (double)len;
    double ls = log_scale;
    *emergency = false;
    if (len >= SEP_ADAPT_WINDOW && rate < 0.001) {
        ls -= 0.7;
        *emergency = true;
    } else if (rate < 0.02 && len >= 500) {
        double g = 5.0 / sqrt((double)step + 1.0);
        g = (0.3 < g) ? 0.3 : g;                     // std::min(gamma_fast, 0.3)
        ls += g * (0.0 - target);
    } else {
        double g = 1.0 / sqrt((double)step + 1.0);
        g = (0.1 < g) ? 0.1 : g;
        ls += g * ((accepted ? 1.0 : 0.0) - target);
    }
    return ls;
}
SEP_ADAPT_FN double log_scale_recover_and_clamp(double ls, const double scale_before, const int sum, const int len) {
    const double rate = (double)sum / (double)len;
    if (scale_before <= 0.011 && rate > 0.15 && rate < 0.30) ls += 0.01;
    ls = (2.3 < ls) ? 2.3 : ls;                      // std::max(std::min(log_scale_, 2.3), -6.9)
    ls = (ls < -6.9) ? -6.9 : ls;
    return ls;
}
SEP_ADAPT_FN double next_log_scale(const double log_scale, const double scale_before, const int sum, const int len, const bool accepted,
                                   const int step, const double target, bool* emergency) {
    return log_scale_recover_and_clamp(log_scale_step(log_scale, sum, len, accepted, step, target, emergency), scale_before, sum, len);
}
