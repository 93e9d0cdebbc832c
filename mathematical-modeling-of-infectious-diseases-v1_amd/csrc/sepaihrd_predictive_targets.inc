// csrc/sepaihrd_predictive_targets.inc -- the targets of the posterior predictive scores as one text for host and device
// (sepaihrd_ensemble_predictive_targets and its twin hostPosteriorPredictiveTargets; DESIGN.md section 6r).
//
// A target is an age group x a window of output rows, plus the running sums of those window totals.
//   age_group [n_age]  -1 leaves the age out, otherwise a group id; the ids in use are exactly 0 .. G - 1, 1 <= G <= n_age
//   window w >= 1, origin o >= 0, counted in output rows with t >= 0:  W = (T_pos - o) / w windows (integer division, W >= 1),
//   window v covers rows o + v w .. o + (v + 1) w - 1; rows before o and the incomplete tail belong to no target
// For series k, window v, group g and one draw (s, r), y the daily draw of sepaihrd_ensemble_predictive_scores:
//   k = 0, 1, 2 (H, ICU, D)   tot[k][v][g] = sum over the rows j of window v and the ages a with age_group[a] = g of y[k][j][a]
//   k = 3, 4, 5               cum[k - 3][v][g] = sum over u <= v of tot[k - 3][u][g]
// Target (k, v, g) is segment (k W + v) G + g of the table, and entry [k][v][g] of every output.  The draws are integers held in
// doubles: a target value is exact, and independent of the order it is formed in, while it stays below 2^53.
//
// The observed target is formed the same way from the observation table, whose values need not be integers -- so its order is
// fixed here (observed_targets): a window total is the sum from 0.0 over the rows ascending and, within a row, the ages
// ascending; the running sum adds the window totals in their order.  A window target is usable when every daily observation it
// sums is usable (finite and >= 0), a cumulative target when every window u <= v of its series and group is; an unusable target
// is NaN.  Every translation unit that includes this file is compiled with contraction off, as for
// csrc/sepaihrd_predictive_score.inc, whose cell_rule and summary_field score the targets with T_pos = W and n_age = G.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sepaihrd_predictive_score.inc"

namespace sepaihrd_targets {

constexpr int N_SERIES = 6;  // H, ICU, D window totals, then their running sums

SEP_SCORE_FN int window_count(int T_pos, int window, int origin) { return (window >= 1 && origin >= 0 && origin <= T_pos) ? (T_pos - origin) / window : 0; }
SEP_SCORE_FN int window_first_row(int v, int window, int origin) { return origin + v * window; }
// the window of output row t, or -1 where the row belongs to no target
SEP_SCORE_FN int window_of_row(int t, int window, int origin, int W) {
    if (t < origin) return -1;
    const int v = (t - origin) / window;
    return v < W ? v : -1;
}
SEP_SCORE_FN size_t target_index(int k, int v, int g, int W, int G) { return ((size_t)k * W + v) * G + g; }

// The groups of age_group: their number G, or the first rule it breaks -- -1: an id < -1 or >= n_age (at *where), -2: no age in
// any group, -3: a gap in the ids (*where is the first id without an age).
SEP_SCORE_FN int group_count(const int32_t* age_group, int n_age, int* where) {
    int top = -1;
    for (int a = 0; a < n_age; ++a) {
        if (age_group[a] < -1 || age_group[a] >= n_age) { *where = a; return -1; }
        if (age_group[a] > top) top = age_group[a];
    }
    if (top < 0) return -2;
    for (int g = 0; g <= top; ++g) {
        bool seen = false;
        for (int a = 0; a < n_age; ++a) seen = seen || age_group[a] == g;
        if (!seen) { *where = g; return -3; }
    }
    return top + 1;
}

// The observed targets of daily series k (0..2) and group g: tot into out[(k W + v) G + g], cum into out[((k + 3) W + v) G + g]
// for every window v.  obs(k, t, a) is the daily observation of output row t and age a.
template <class Obs>
SEP_SCORE_FN void observed_targets(const Obs& obs, const int32_t* age_group, int n_age, int window, int origin, int W, int G, int k, int g,
                                   double* out) {
    const double qnan = __builtin_nan("");
    double run = 0.0;
    bool run_usable = true;
    for (int v = 0; v < W; ++v) {
        double tot = 0.0;
        bool usable = true;
        const int j0 = window_first_row(v, window, origin);
        for (int j = j0; j < j0 + window; ++j)
            for (int a = 0; a < n_age; ++a) {
                if (age_group[a] != g) continue;
                const double y = obs(k, j, a);
                usable = usable && sepaihrd_score::usable_observation(y);
                tot += y;
            }
        run_usable = run_usable && usable;
        if (run_usable) run += tot;
        out[target_index(k, v, g, W, G)] = usable ? tot : qnan;
        out[target_index(k + 3, v, g, W, G)] = run_usable ? run : qnan;
    }
}

// field f of entry (series k of 6, group g, g == G pooling the groups) of the summary [6][G + 1][4 + 2 L]: summary_field of
// csrc/sepaihrd_predictive_score.inc over series k's W x G targets -- windows ascending, groups ascending within a window
SEP_SCORE_FN double target_summary_field(const double* target_scores, const double* target_obs, size_t m, int W, int G, int L, int k, int g, int f) {
    const size_t first = (size_t)k * W * G;
    return sepaihrd_score::summary_field(target_scores + first * (size_t)sepaihrd_score::cell_width(L), target_obs + first, m, W, G, L, 0, g, f);
}

}  // namespace sepaihrd_targets
