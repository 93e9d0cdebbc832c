// csrc/sepaihrd_predictive_score.inc -- the scoring rules of the posterior predictive draws as one text for host and device
// (sepaihrd_ensemble_predictive_scores and its twin hostPosteriorPredictiveScores; DESIGN.md section 6q).
//
// A segment holds the m = n_valid R draws of one (series, time, age) cell of a daily series, sorted ascending:
// x(0) <= ... <= x(m-1), integers held in doubles.  Its sums
//     S1 = sum x,  S2 = sum x^2,  S_less = sum of the draws below y,  G = sum_i (2 i - m + 1) x(i),
//     n_less, n_eq = the draws below and at the observation y
// are sums of integers: exact, and so independent of the order they are formed in, as long as each stays below 2^53
// (sums_exact).  The device reduces them across lanes and waves, the twin serially (segment_sums); what follows the sums --
// cell_rule, summary_walk -- is a fixed sequence of IEEE operations, and every translation unit that includes this file is
// compiled with contraction off (csrc/Makefile: -ffp-contract=off on the object's line; host/Makefile: CXXFLAGS), so the two
// give the same bits.
//
// Per cell, 5 + 4 L fields (L central coverage levels c_l, alpha_l = 1 - c_l; q(p) the rule of csrc/sepaihrd_quantile.inc):
//     0 mean      S1 / m
//     1 variance  (S2 - S1 S1 / m) / (m - 1); NaN for m = 1
//     2 median    q(0.5)
//     3 CRPS      A / m - G / (m m),  A = y (n_less - n_greater) + S1 - 2 S_less - y n_eq  (= sum |x - y|;  G = 1/2 sum_ij |x_i - x_j|)
//     4 WIS       (0.5 |y - median| + sum_l (alpha_l / 2) IS_l) / (L + 0.5)
//     5 + 4 l ..  lo = q(0.5 - 0.5 c), hi = q(0.5 + 0.5 c), IS = (hi - lo) + (2 / alpha)(max(0, lo - y) + max(0, y - hi)),
//                 covered = 1.0 if lo <= y <= hi else 0.0
// Mean, variance, median, lo and hi for every cell with m > 0; CRPS, WIS, IS and covered NaN where the observation is not usable
// (usable: finite and >= 0, the likelihood's rule); every field NaN when m = 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_quantile.inc"

#if defined(__HIPCC__)
#define SEP_SCORE_FN __host__ __device__ inline
#else
#define SEP_SCORE_FN inline
#endif

namespace sepaihrd_score {

constexpr int MAX_LEVELS = 8;
constexpr int CELL_FIXED = 5, CELL_PER_LEVEL = 4;  // fields of a cell: CELL_FIXED + CELL_PER_LEVEL L
constexpr int SUMMARY_FIXED = 4, SUMMARY_PER_LEVEL = 2;

SEP_SCORE_FN int cell_width(int L) { return CELL_FIXED + CELL_PER_LEVEL * L; }
SEP_SCORE_FN int summary_width(int L) { return SUMMARY_FIXED + SUMMARY_PER_LEVEL * L; }

struct SegmentSums {
    int64_t n_less, n_eq;
    double S1, S2, S_less, G;
};

SEP_SCORE_FN bool usable_observation(double y) { return y >= 0.0 && y <= 0x1.fffffffffffffp+1023; }

// what draw i of m (sorted position i; m < 2^31) adds to the sums; y NaN: nothing is below or at it.  The coefficient
// 2 i - m + 1 is formed in doubles, where it is exact.
SEP_SCORE_FN void add_draw(SegmentSums& s, double x, int i, int m, double y) {
    s.n_less += (x < y);
    s.n_eq += (x == y);
    s.S1 += x;
    s.S2 += x * x;
    s.S_less += (x < y) ? x : 0.0;
    s.G += (2.0 * (double)i - (double)(m - 1)) * x;
}

// the serial form: the twin's, and the statement of what the kernels reduce
SEP_SCORE_FN SegmentSums segment_sums(const double* sorted, size_t m, double y) {
    SegmentSums s = {0, 0, 0.0, 0.0, 0.0, 0.0};
    for (size_t i = 0; i < m; ++i) add_draw(s, sorted[i], (int)i, (int)m, y);
    return s;
}

// every sum of a segment of m draws, the largest x_max, stays below 2^53: m x_max max(m, x_max) < 2^53
SEP_SCORE_FN bool sums_exact(size_t m, double x_max) {
    const double dm = (double)m;
    return dm * x_max * (dm > x_max ? dm : x_max) < 9007199254740992.0;
}

// mid-PIT from the counts: the expression of sepaihrd_poisson::mid_pit
SEP_SCORE_FN double pit_of(const SegmentSums& s, size_t m, double y) {
    return usable_observation(y) && m > 0 ? ((double)s.n_less + 0.5 * (double)s.n_eq) / (double)m : __builtin_nan("");
}

// the fields of one cell from its sorted segment, its sums and the observation
SEP_SCORE_FN void cell_rule(const double* sorted, size_t m, double y, const SegmentSums& s, const double* levels, int L, double* out) {
    const double qnan = __builtin_nan("");
    if (m == 0) {
        for (int f = 0; f < cell_width(L); ++f) out[f] = qnan;
        return;
    }
    const bool usable = usable_observation(y);
    const double dm = (double)m;
    const double median = sepaihrd_quantile::sorted_quantile(sorted, m, 0.5);
    out[0] = s.S1 / dm;
    out[1] = m > 1 ? (s.S2 - s.S1 * s.S1 / dm) / (dm - 1.0) : qnan;
    out[2] = median;
    const int64_t n_greater = (int64_t)m - s.n_less - s.n_eq;
    const double A = y * (double)(s.n_less - n_greater) + s.S1 - 2.0 * s.S_less - y * (double)s.n_eq;
    out[3] = usable ? A / dm - s.G / (dm * dm) : qnan;
    double wis = 0.5 * __builtin_fabs(y - median);
    for (int l = 0; l < L; ++l) {
        const double c = levels[l], alpha = 1.0 - c;
        const double lo = sepaihrd_quantile::sorted_quantile(sorted, m, 0.5 - 0.5 * c);
        const double hi = sepaihrd_quantile::sorted_quantile(sorted, m, 0.5 + 0.5 * c);
        const double below = lo - y, above = y - hi;
        const double is = (hi - lo) + (2.0 / alpha) * (((0.0 < below) ? below : 0.0) + ((0.0 < above) ? above : 0.0));
        wis += (alpha / 2.0) * is;
        double* f = out + CELL_FIXED + CELL_PER_LEVEL * l;
        f[0] = lo;
        f[1] = hi;
        f[2] = usable ? is : qnan;
        f[3] = usable ? ((lo <= y && y <= hi) ? 1.0 : 0.0) : qnan;
    }
    out[4] = usable ? wis / ((double)L + 0.5) : qnan;
}

// Field f of entry (series, age) of the summary, age == n_age pooling all ages: f = 0 the count of usable cells, then the means of
// CRPS, WIS and |y - median|, per level the coverage fraction and the mean IS.  The sum starts from 0.0 and runs over the usable
// cells with time ascending, for the pooled entry over the ages ascending within a time; a count of 0 gives a NaN mean.  The cells
// are read eight at a time ahead of their sums (the loads do not wait for the chain of additions), and added in their order.
// cell_scores [3][T_pos][n_age][5 + 4 L], observed [3][T_pos][n_age], m the draws per segment.
constexpr int SUMMARY_BATCH = 8;
SEP_SCORE_FN double summary_field(const double* cell_scores, const double* observed, size_t m, int T_pos, int n_age, int L, int series, int age,
                                  int f) {
    const int W = cell_width(L);
    const int lf = f - SUMMARY_FIXED;
    // the cell field that f averages: CRPS, WIS, the median (for |y - median|), covered and IS of level lf / 2
    const int col = f <= 1 ? 3 : f == 2 ? 4 : f == 3 ? 2 : CELL_FIXED + CELL_PER_LEVEL * (lf / 2) + (lf % 2 == 0 ? 3 : 2);
    const int a0 = age < n_age ? age : 0, a1 = age < n_age ? age + 1 : n_age;
    double sum = 0.0, count = 0.0;
    int t = 0, a = a0;
    while (t < T_pos) {
        double y[SUMMARY_BATCH], v[SUMMARY_BATCH];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int d = 0; d < SUMMARY_BATCH; ++d) {
            const bool in = t < T_pos;
            const size_t cell = ((size_t)series * T_pos + (in ? t : 0)) * n_age + a;
            y[d] = in ? observed[cell] : __builtin_nan("");
            v[d] = in ? cell_scores[cell * W + col] : 0.0;
            if (++a == a1) { a = a0; ++t; }
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int d = 0; d < SUMMARY_BATCH; ++d)
            if (m > 0 && usable_observation(y[d])) {
                count += 1.0;
                sum += f == 3 ? __builtin_fabs(y[d] - v[d]) : v[d];
            }
    }
    return f == 0 ? count : (count > 0.0 ? sum / count : __builtin_nan(""));
}

// entry (series, age) whole: out [4 + 2 L]
SEP_SCORE_FN void summary_walk(const double* cell_scores, const double* observed, size_t m, int T_pos, int n_age, int L, int series, int age,
                               double* out) {
    for (int f = 0; f < summary_width(L); ++f) out[f] = summary_field(cell_scores, observed, m, T_pos, n_age, L, series, age, f);
}

}  // namespace sepaihrd_score
