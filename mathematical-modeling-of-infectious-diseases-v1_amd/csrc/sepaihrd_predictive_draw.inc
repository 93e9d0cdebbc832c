// csrc/sepaihrd_predictive_draw.inc -- the one text of a posterior predictive draw on the device, compiled by the daily draw kernel
// (csrc/sepaihrd_predictive_nb.hip) and the target draw kernel (csrc/sepaihrd_predictive_targets.hip): which draw, age and series
// a lane owns, the mean of a row, its variate and the stores into means and draws.  What a kernel does with the variate -- the
// daily table, the window totals -- is its own.  The sampler is csrc/sepaihrd_nb_draw.inc, the text the host twin compiles too;
// its includers are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sepaihrd_device.h"
#include "sepaihrd_nb_draw.inc"
#include "sepaihrd_predictive_device.h"

namespace sepaihrd {
namespace {

constexpr int DRAW_BLOCK = 256;

// One lane per (sample s, replicate r, age, series): consecutive lanes along idx = s R + r, so the loads of a sample's increments
// are broadcasts and the stores into a segment contiguous; the age comes from the grid's y dimension (the kernel says which), the
// series is its z dimension.  Each lane walks only the T_pos output times of its own running sum.
struct DrawLane {
    size_t idx, s, col;  // slot of every segment, sample, the sample's column of this age in the integrator's workspace
    uint32_t r;
    int age, ser, comp;  // comp: the cum row of the series
    bool in_range, ok;   // a slot of a sample; of a sample that has draws (integrated, k not NaN)
    double k;            // the sample's dispersion for the series; +inf (the Poisson draw) where the call has none
};

// false: the lane is beyond the padded table and has nothing to do
__device__ __forceinline__ bool draw_lane(const PredictiveArgs& a, const double* __restrict__ k_used, const int age, DrawLane& l) {
    l.idx = (size_t)blockIdx.x * DRAW_BLOCK + threadIdx.x;
    if (l.idx >= (size_t)a.N_pad) return false;
    l.age = age;
    l.ser = (int)blockIdx.z;
    l.s = l.idx / (size_t)a.R;
    l.r = (uint32_t)(l.idx % (size_t)a.R);
    l.in_range = l.s < (size_t)a.S;
    l.ok = l.in_range && a.wstatus[l.s] == 0;
    l.comp = (l.ser == 0) ? 1 : (l.ser == 1) ? 2 : 0;  // cum rows are D, CumH, CumICU; series are H, ICU, D
    l.k = (l.ok && k_used != nullptr) ? k_used[l.s * 3 + (size_t)l.ser] : INFINITY;
    l.col = l.s * (size_t)a.lpc + (size_t)age;
    return true;
}

// row of the daily table, and third stream coordinate, of the lane's output time t
__device__ __forceinline__ size_t draw_cell(const PredictiveArgs& a, const DrawLane& l, const int t) {
    return ((size_t)l.ser * a.Tp + t) * a.n + l.age;
}

// Output time t of the lane: m = max(0, increment) into means, y ~ NegativeBinomial(m + 1e-10, k) at stream coordinates
// (s, r, (series Tp + t) n + age) into draws, y returned.  The variate is drawn where the kernel needs it or draws is wanted;
// undrawn, and for a failed sample, y and m are NaN.
__device__ __forceinline__ double draw_row(const PredictiveArgs& a, const DrawLane& l, const int t, const bool needed) {
    double m = NAN, y = NAN;
    if (l.ok) {
        const double inc = a.cum[cum_index(a.T, l.col, a.runup_offset + t, l.comp)];
        m = (0.0 < inc) ? inc : 0.0;  // std::max(0.0, cur - prev)
        if (needed || a.draws != nullptr) y = sepaihrd_nb_draw::nb_variate(a.seed, (uint32_t)l.s, l.r, (uint32_t)draw_cell(a, l, t), m + 1e-10, l.k);
    }
    if (l.in_range) {
        if (a.means != nullptr && l.r == 0) a.means[((l.s * 3 + l.ser) * a.Tp + t) * a.n + l.age] = m;
        if (a.draws != nullptr) a.draws[((l.idx * 3 + l.ser) * a.Tp + t) * a.n + l.age] = y;
    }
    return y;
}

// what the launch of either kernel asks: sizes, the third stream coordinate below 2^32, and n_age on the grid's y dimension, which
// holds at most 65 535 blocks (the context refuses n_age > 64, so the bound refuses no call it accepts)
inline bool draw_args_ok(const PredictiveArgs& a) {
    return a.S > 0 && a.R > 0 && a.n > 0 && a.n <= 65535 && a.Tp > 0 && (size_t)a.S * a.R <= (size_t)a.N_pad && a.N_pad % WAVE == 0 &&
           (uint64_t)3 * a.Tp * a.n < ((uint64_t)1 << 32);
}

}  // namespace
}  // namespace sepaihrd
