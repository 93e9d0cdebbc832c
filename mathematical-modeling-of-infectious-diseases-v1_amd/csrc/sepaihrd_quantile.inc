// csrc/sepaihrd_quantile.inc -- the project's quantile rule as one text for host and device.
//
// Quantile p of n >= 1 values sorted ascending: the exact-sort rule of the reference's PostCalibrationAnalyser
// (src/model/PostCalibrationAnalyser.cpp:316-326),
//     pos = p (n - 1), idx = floor pos, frac = pos - idx,
//     v[idx] (1 - frac) + v[idx + 1] frac   where idx + 1 < n, else v[idx]
// -- two products and one sum in this order.  Every translation unit that includes this file is compiled with contraction
// off (csrc/Makefile: -ffp-contract=off on the object's line; host/Makefile: CXXFLAGS), so that the device kernels and their
// host twins give the same bits.  Values past n (the +inf padding of a sorted segment) are never read.  V is a floating or an
// integer type; an integer is converted before it is multiplied.
// Self-contained: nothing but the function qualifier below, so that a user does not pull in the random streams.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define SEP_QUANTILE_FN __host__ __device__ inline
#else
#define SEP_QUANTILE_FN inline
#endif

namespace sepaihrd_quantile {

template <class V>
SEP_QUANTILE_FN double sorted_quantile(const V* v, size_t n, double p) {
    const double pos = p * (double)(n - 1);
    const size_t idx = (size_t)pos;
    const double frac = pos - (double)idx;
    return idx + 1 < n ? (double)v[idx] * (1.0 - frac) + (double)v[idx + 1] * frac : (double)v[idx];
}

}  // namespace sepaihrd_quantile
