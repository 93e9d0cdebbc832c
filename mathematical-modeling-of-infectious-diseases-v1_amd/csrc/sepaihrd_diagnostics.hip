// =============================================================================
// csrc/sepaihrd_diagnostics.hip -- convergence diagnostics of C chains x N draws on gfx950.
//
// Per column (a parameter, or the chains' log-likelihood values) the rank-normalised split R-hat and the bulk / tail
// effective sample sizes of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), as the R package `posterior` (1.x)
// computes them function by function (split_chains, z_scale, fold_draws, .rhat, .ess, ess_quantile).  Output row:
//   mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, r_hat
// and the Geyer truncation lag max_t of each ESS series (raw, z, I[x <= q05], I[x <= q95]).
//
// Pipeline for a GROUP of columns (group size set by a scratch budget; every column is computed independently of the
// group it falls in, so the table has the same bits however the columns are grouped):
//   gather     [C][n][P]-strided draws -> split layout xs[g][2C][M] (split chain j = 2c + h, M = floor(N/2)) plus, for
//              odd N, the dropped middle draws mid[g][C]
//   stats      fixed-order partial sums per 16384-draw chunk, then the chunks in order: mean, sd (n - 1), finite / constant
//   quantiles  odd N: a keys-only radix sort of all C N draws (q05 / q95 see the middle draws too)
//   ranks      radix sort of (split draw, split index) pairs; average ranks over runs of equal keys found by
//              binary search (-0.0 == +0.0 under ==, and rocPRIM orders the two as equal); z = normcdfinv((r - 3/8) / (S + 1/4))
//   fold       |x - median(split draws)|, sorted and ranked the same way
//   moments    one wavefront per (column, series, split chain): mean and variance in a fixed butterfly order
//   R-hat      per (column, series) over the 2C split chains: R = sqrt(((M - 1)/M W + var(m_j)) / W) for z and folded z
//   acov       direct sums d_i d_{i+t} over blocks of 64 lags: lane = lag, a workgroup per (pair, chain partition),
//              partitions added in order; only pairs still live run a block
//   Geyer      one thread per (column, series) walks the new lags of the block; one int read back per block says whether
//              another block is needed.  Work O(C N lags needed), not O(C N^2).
// Compiled with -ffp-contract=off: every product is rounded before its sum, as in the numpy restatement (diagnostics.py).
// =============================================================================
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <float.h>

#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "sepaihrd_device.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_quantile.inc"  // the project's type-7 rule

namespace sepaihrd {
namespace {

constexpr int LAG_BLOCK = 64;           // lags per acov block (one per lane)
constexpr int STAT_CHUNK = 256 * 64;    // draws per partial of the column statistics
constexpr int N_KINDS = 5;              // moment series: x, z, folded z, I[x <= q05], I[x <= q95]
constexpr int N_ESS = 4;                // ESS series: x, z, I05, I95 (moment kinds 0, 1, 3, 4)
constexpr int INFO_W = 16;              // doubles per column in DiagArgs::info

// info[g][*]
enum { I_MEAN = 0, I_SD, I_BAD, I_MED, I_Q05, I_Q95, I_XS_CONST, I_Z_CONST, I_ZF_CONST, I_I05_CONST, I_I95_CONST,
       I_RHAT_Z, I_RHAT_ZF };

struct DiagArgs {
    int G, C, N, M;           // columns in the group, chains, draws per chain, split length floor(N/2)
    size_t S;                 // split draws per column, 2 C M
    size_t CN;                // all draws per column
    int npart, chains_per_part;
    double* xs;               // [G][S]
    double* mid;              // [G][C] (odd N)
    double* zs;               // [G][S]
    double* zf;               // [G][S]
    double* info;             // [G][INFO_W]
    double* part;             // [G][nb][4] column statistics partials
    int nb;
    double* cmean;            // [G][N_KINDS][2C]
    double* cvar;             // [G][N_KINDS][2C]
    double* kstat;            // [G][N_KINDS][3]: mean of chain means, var of chain means, mean of chain variances
    double* acm;              // [G N_ESS][M_pad] mean over chains of acov_t
    double* apart;            // [G N_ESS][npart][LAG_BLOCK]
    size_t M_pad;
    int32_t* tstate;          // [G N_ESS] Geyer walk position (even t)
    int32_t* live;            // [G N_ESS]
    double* ess;              // [G N_ESS]
    int32_t* maxlag;          // [G N_ESS]
    int32_t* live_count;      // [1]
    double* out;              // [G][7]
};

__device__ inline int ess_kind(int s) { return s < 2 ? s : s + 1; }

__device__ inline double series_value(const DiagArgs& a, int g, int kind, size_t pos) {
    const size_t e = (size_t)g * a.S + pos;
    switch (kind) {
        case 0: return a.xs[e];
        case 1: return a.zs[e];
        case 2: return a.zf[e];
        case 3: return a.xs[e] <= a.info[g * INFO_W + I_Q05] ? 1.0 : 0.0;
        default: return a.xs[e] <= a.info[g * INFO_W + I_Q95] ? 1.0 : 0.0;
    }
}

// number of sorted values <= x
__device__ inline size_t count_le(const double* v, size_t n, double x) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t m = lo + (hi - lo) / 2;
        if (v[m] <= x) lo = m + 1; else hi = m;
    }
    return lo;
}

__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// ---- gather: (chain c, draw n) row of the source -> split layout, one thread per row, the group's columns in turn
__global__ __launch_bounds__(256) void diag_gather_kernel(const DiagArgs a, const double* src, size_t chain_stride,
                                                          size_t sample_stride, int g0, int ng) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= a.CN) return;
    const int c = (int)(row / a.N), n = (int)(row % a.N);
    const double* p = src + (size_t)c * chain_stride + (size_t)n * sample_stride;
    size_t dst;
    bool split = true;
    if (n < a.M) dst = ((size_t)2 * c) * a.M + n;
    else if (n >= a.N - a.M) dst = ((size_t)2 * c + 1) * a.M + (n - (a.N - a.M));
    else { split = false; dst = c; }
    for (int k = 0; k < ng; ++k) {
        const double v = p[k];
        const int g = g0 + k;
        if (split) a.xs[(size_t)g * a.S + dst] = v;
        else a.mid[(size_t)g * a.C + dst] = v;
    }
}

__device__ inline double column_draw(const DiagArgs& a, int g, size_t e) {
    return e < a.S ? a.xs[(size_t)g * a.S + e] : a.mid[(size_t)g * a.C + (e - a.S)];
}

// ---- column statistics, pass 0: sum, min, max, non-finite count; pass 1: sum of squared deviations from the mean
__global__ __launch_bounds__(256) void diag_stats_partial_kernel(const DiagArgs a, const int pass) {
    __shared__ double s0[256], s1[256], s2[256], s3[256];
    const int g = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const size_t e0 = (size_t)b * STAT_CHUNK, e1 = e0 + STAT_CHUNK < a.CN ? e0 + STAT_CHUNK : a.CN;
    const double mean = a.info[g * INFO_W + I_MEAN];
    double sum = 0.0, mn = INFINITY, mx = -INFINITY, bad = 0.0;
    for (size_t e = e0 + t; e < e1; e += 256) {
        const double v = column_draw(a, g, e);
        if (pass == 0) {
            if (isfinite(v)) { sum += v; mn = fmin(mn, v); mx = fmax(mx, v); } else bad += 1.0;
        } else {
            const double d = v - mean;
            sum += d * d;
        }
    }
    s0[t] = sum; s1[t] = mn; s2[t] = mx; s3[t] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            s0[t] += s0[t + w];
            s1[t] = fmin(s1[t], s1[t + w]);
            s2[t] = fmax(s2[t], s2[t + w]);
            s3[t] += s3[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        double* p = a.part + ((size_t)g * a.nb + b) * 4;
        p[0] = s0[0]; p[1] = s1[0]; p[2] = s2[0]; p[3] = s3[0];
    }
}

__global__ void diag_stats_final_kernel(const DiagArgs a, const int pass) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    double sum = 0.0, mn = INFINITY, mx = -INFINITY, bad = 0.0;
    for (int b = 0; b < a.nb; ++b) {
        const double* p = a.part + ((size_t)g * a.nb + b) * 4;
        sum += p[0]; mn = fmin(mn, p[1]); mx = fmax(mx, p[2]); bad += p[3];
    }
    double* info = a.info + g * INFO_W;
    if (pass == 0) {
        info[I_MEAN] = sum / (double)a.CN;
        // posterior's should_return_NA: a non-finite draw, or max - min < DBL_EPSILON
        info[I_BAD] = (bad > 0.0 || !(mx - mn >= DBL_EPSILON)) ? 1.0 : 0.0;
    } else {
        info[I_SD] = sqrt(sum / (double)(a.CN - 1));
    }
}

// ---- sort inputs
__global__ __launch_bounds__(256) void diag_all_keys_kernel(const DiagArgs a, double* keys) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.G * a.CN) return;
    const int g = (int)(e / a.CN);
    keys[e] = column_draw(a, g, e % a.CN);
}

__global__ __launch_bounds__(256) void diag_split_keys_kernel(const DiagArgs a, double* keys, int32_t* vals, const int fold) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.G * a.S) return;
    const int g = (int)(e / a.S);
    const double x = a.xs[e];
    keys[e] = fold ? fabs(x - a.info[g * INFO_W + I_MED]) : x;
    vals[e] = (int32_t)(e % a.S);
}

// odd N: q05 / q95 of all C N draws (sorted)
__global__ void diag_all_quantiles_kernel(const DiagArgs a, const double* sorted) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    const double* v = sorted + (size_t)g * a.CN;
    a.info[g * INFO_W + I_Q05] = sepaihrd_quantile::sorted_quantile(v, a.CN, 0.05);
    a.info[g * INFO_W + I_Q95] = sepaihrd_quantile::sorted_quantile(v, a.CN, 0.95);
}

// ---- average ranks -> normal scores, written back to the draw's split position
__global__ __launch_bounds__(256) void diag_rank_kernel(const DiagArgs a, const double* keys, const int32_t* vals, double* z) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.G * a.S) return;
    const size_t S = a.S;
    const size_t g0 = (e / S) * S, i = e - g0;
    const double* v = keys + g0;
    const double k = v[i];
    size_t lo = i, hi = i + 1;
    if (i > 0 && v[i - 1] == k) {   // first position of the run of keys equal to k
        size_t l = 0, h = i;
        while (l < h) { const size_t m = l + (h - l) / 2; if (v[m] < k) l = m + 1; else h = m; }
        lo = l;
    }
    if (i + 1 < S && v[i + 1] == k) {   // one past its last position
        size_t l = i + 1, h = S;
        while (l < h) { const size_t m = l + (h - l) / 2; if (v[m] <= k) l = m + 1; else h = m; }
        hi = l;
    }
    const double r = 0.5 * ((double)lo + (double)hi + 1.0);   // mean of the 1-based ranks lo + 1 .. hi
    z[g0 + (size_t)vals[e]] = normcdfinv((r - 0.375) / ((double)S + 0.25));
}

// after the sort of the split draws: median, (even N) the tail quantiles, the constancy of each series
__global__ void diag_split_info_kernel(const DiagArgs a, const double* sorted, const int even) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    const size_t S = a.S;
    const double* v = sorted + (size_t)g * S;
    double* info = a.info + g * INFO_W;
    info[I_MED] = (v[S / 2 - 1] + v[S / 2]) / 2.0;
    if (even) {
        info[I_Q05] = sepaihrd_quantile::sorted_quantile(v, S, 0.05);
        info[I_Q95] = sepaihrd_quantile::sorted_quantile(v, S, 0.95);
    }
    info[I_XS_CONST] = !(v[S - 1] - v[0] >= DBL_EPSILON) ? 1.0 : 0.0;
    info[I_Z_CONST] = (v[0] == v[S - 1]) ? 1.0 : 0.0;
    const size_t n05 = count_le(v, S, info[I_Q05]), n95 = count_le(v, S, info[I_Q95]);
    info[I_I05_CONST] = (n05 == 0 || n05 == S) ? 1.0 : 0.0;
    info[I_I95_CONST] = (n95 == 0 || n95 == S) ? 1.0 : 0.0;
}

__global__ void diag_fold_info_kernel(const DiagArgs a, const double* sorted) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    const double* v = sorted + (size_t)g * a.S;
    a.info[g * INFO_W + I_ZF_CONST] = (v[0] == v[a.S - 1]) ? 1.0 : 0.0;
}

// ---- per split chain: mean and variance (n - 1) of each series; one wavefront per (column, kind, chain)
__global__ __launch_bounds__(256) void diag_chain_moments_kernel(const DiagArgs a) {
    const size_t wid = ((size_t)blockIdx.x * 256 + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    const size_t nchain = (size_t)2 * a.C;
    if (wid >= (size_t)a.G * N_KINDS * nchain) return;
    const int j = (int)(wid % nchain);
    const int kind = (int)((wid / nchain) % N_KINDS);
    const int g = (int)(wid / (nchain * N_KINDS));
    const size_t base = (size_t)j * a.M;
    double s = 0.0;
    for (int i = lane; i < a.M; i += WAVE) s += series_value(a, g, kind, base + i);
    const double m = wave_sum(s) / (double)a.M;
    double q = 0.0;
    for (int i = lane; i < a.M; i += WAVE) { const double d = series_value(a, g, kind, base + i) - m; q += d * d; }
    const double var = wave_sum(q) / (double)(a.M - 1);
    if (lane == 0) { a.cmean[wid] = m; a.cvar[wid] = var; }
}

// ---- per (column, kind) over the 2C split chains: mean and variance of the chain means, mean of the chain variances;
// R-hat of z and of folded z.  One workgroup each, strided partial sums then a fixed tree.
__global__ __launch_bounds__(256) void diag_kind_stats_kernel(const DiagArgs a) {
    __shared__ double s0[256], s1[256];
    const int gk = blockIdx.x, t = threadIdx.x;
    const int nchain = 2 * a.C;
    const double* cm = a.cmean + (size_t)gk * nchain;
    const double* cv = a.cvar + (size_t)gk * nchain;
    double sm = 0.0, sv = 0.0;
    for (int j = t; j < nchain; j += 256) { sm += cm[j]; sv += cv[j]; }
    s0[t] = sm; s1[t] = sv;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { s0[t] += s0[t + w]; s1[t] += s1[t + w]; }
        __syncthreads();
    }
    const double mm = s0[0] / nchain, W = s1[0] / nchain;
    __syncthreads();
    double sq = 0.0;
    for (int j = t; j < nchain; j += 256) { const double d = cm[j] - mm; sq += d * d; }
    s0[t] = sq;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) s0[t] += s0[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double var_m = s0[0] / (nchain - 1);
        double* k = a.kstat + (size_t)gk * 3;
        k[0] = mm; k[1] = var_m; k[2] = W;
        const int g = gk / N_KINDS, kind = gk % N_KINDS;
        if (kind == 1 || kind == 2) {
            const double M = (double)a.M;
            a.info[g * INFO_W + (kind == 1 ? I_RHAT_Z : I_RHAT_ZF)] = sqrt(((M - 1.0) / M * W + var_m) / W);
        }
    }
}

// which (column, series) pairs need autocovariances at all
__global__ void diag_init_pairs_kernel(const DiagArgs a) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.G * N_ESS) return;
    const int g = p / N_ESS, s = p % N_ESS;
    const double* info = a.info + g * INFO_W;
    const int flag[N_ESS] = {I_XS_CONST, I_Z_CONST, I_I05_CONST, I_I95_CONST};
    const bool on = a.M >= 3 && info[I_BAD] == 0.0 && info[flag[s]] == 0.0;
    a.live[p] = on ? 1 : 0;
    a.tstate[p] = 0;
    a.ess[p] = NAN;
    a.maxlag[p] = -1;
}

// ---- autocovariance block: lags t0 .. t0 + 63 (lane = lag) of every split chain of one partition, summed over its chains
__global__ __launch_bounds__(256) void diag_acov_kernel(const DiagArgs a, const int t0) {
    __shared__ double red[4][LAG_BLOCK];
    const int p = blockIdx.x, part = blockIdx.y;
    if (a.live[p] == 0) return;
    const int g = p / N_ESS, kind = ess_kind(p % N_ESS);
    const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int t = t0 + lane;
    const int M = a.M;
    const int j0 = part * a.chains_per_part, j1 = min(j0 + a.chains_per_part, 2 * a.C);
    const double* cm = a.cmean + ((size_t)g * N_KINDS + kind) * (2 * a.C);
    double tot = 0.0;
    for (int j = j0 + w; j < j1; j += 4) {
        const double m = cm[j];
        const size_t base = (size_t)j * M;
        double acc = 0.0;
        for (int i = 0; i + t < M; ++i)
            acc += (series_value(a, g, kind, base + i) - m) * (series_value(a, g, kind, base + i + t) - m);
        tot += acc / (double)M;
    }
    red[w][lane] = tot;
    __syncthreads();
    if (w == 0) a.apart[((size_t)p * a.npart + part) * LAG_BLOCK + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

__global__ __launch_bounds__(LAG_BLOCK) void diag_acov_reduce_kernel(const DiagArgs a, const int t0) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (a.live[p] == 0 || t0 + lane >= a.M) return;
    double s = 0.0;
    for (int q = 0; q < a.npart; ++q) s += a.apart[((size_t)p * a.npart + q) * LAG_BLOCK + lane];
    a.acm[(size_t)p * a.M_pad + t0 + lane] = s / (double)(2 * a.C);
}

// ---- Geyer's initial positive sequence over the lags computed so far; at its end the monotone sequence and the ESS
// (posterior's .ess; rho_t = 1 - (mean_var - mean_j acov_t) / var_plus, rho_0 = 1)
__global__ void diag_geyer_kernel(const DiagArgs a, const int computed) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.G * N_ESS || a.live[p] == 0) return;
    const int g = p / N_ESS, kind = ess_kind(p % N_ESS);
    const double M = (double)a.M;
    const double* acm = a.acm + (size_t)p * a.M_pad;
    const double mean_var = acm[0] * M / (M - 1.0);
    const double var_plus = mean_var * (M - 1.0) / M + a.kstat[((size_t)g * N_KINDS + kind) * 3 + 1];
    auto rho = [&](int t) { return 1.0 - (mean_var - acm[t]) / var_plus; };
    int t = a.tstate[p];
    double re, ro;
    for (;;) {
        re = t == 0 ? 1.0 : rho(t);
        ro = rho(t + 1);
        if (!(t < a.M - 5 && !isnan(re + ro) && re + ro > 0.0)) break;   // the loop of .ess ends at pair t
        if (t + 3 >= computed) {   // pair t + 2 is not there yet
            a.tstate[p] = t;
            atomicAdd(a.live_count, 1);
            return;
        }
        t += 2;
    }
    const int max_t = t;
    // pair max_t was kept when its sum was >= 0 (t = 0: always); else its even term is re where re > 0, 0 otherwise
    const bool kept = max_t == 0 || re + ro >= 0.0;
    const double r_last = kept ? re : (re > 0.0 ? re : 0.0);
    // initial monotone sequence over the kept pairs before max_t, streamed: a pair larger than the previous (already
    // adjusted) pair is set to the mean of that one
    double prev = 1.0 + rho(1);
    double sum = prev;   // rho_0 + rho_1
    for (int u = 2; u <= max_t - 2; u += 2) {
        double e = rho(u), o = rho(u + 1);
        if (e + o > prev) { e = prev / 2.0; o = e; }
        prev = e + o;
        sum += e + o;
    }
    // tau = -1 + 2 sum_{t < max_t} rho_t + rho_{max_t}; with max_t = 0, R's rho_hat_t[1:0] is rho_hat_t[1] = rho_0 = 1
    const double head = max_t == 0 ? 1.0 : sum;
    double tau = -1.0 + 2.0 * head + r_last;
    const double total = 2.0 * a.C * M;
    tau = fmax(tau, 1.0 / log10(total));
    a.ess[p] = total / tau;
    a.maxlag[p] = max_t;
    a.live[p] = 0;
}

__global__ void diag_finalize_kernel(const DiagArgs a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    const double* info = a.info + g * INFO_W;
    double* o = a.out + (size_t)g * 7;
    if (info[I_BAD] != 0.0) {
        for (int k = 0; k < 7; ++k) o[k] = NAN;
        return;
    }
    const double* e = a.ess + (size_t)g * N_ESS;
    const double sd = info[I_SD];
    o[0] = info[I_MEAN];
    o[1] = sd;
    o[2] = sd / sqrt(e[0]);
    o[3] = e[0];
    o[4] = e[1];
    o[5] = (isnan(e[2]) || isnan(e[3])) ? NAN : fmin(e[2], e[3]);
    const double rz = info[I_Z_CONST] != 0.0 ? NAN : info[I_RHAT_Z];
    const double rf = info[I_ZF_CONST] != 0.0 ? NAN : info[I_RHAT_ZF];
    o[6] = (isnan(rz) || isnan(rf)) ? NAN : fmax(rz, rf);
}

inline unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

int chain_diagnostics(const DiagInput& in, double* out, int32_t* max_lag, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int C = in.C, N = in.N, M = N / 2;
    const int ncols = in.P + (in.values ? 1 : 0);
    if (C < 1 || in.P < 1 || N < 4 || (int64_t)C * N >= ((int64_t)1 << 31)) return -4;
    const size_t CN = (size_t)C * N, S = (size_t)2 * C * M;
    const bool even = (N % 2) == 0;
    const int npart = std::min(64, std::max(1, (2 * C) / 32));
    const int chains_per_part = (2 * C + npart - 1) / npart;
    const size_t M_pad = ((size_t)M + LAG_BLOCK - 1) / LAG_BLOCK * LAG_BLOCK;
    const int nb = (int)((CN + STAT_CHUNK - 1) / STAT_CHUNK);
    // scratch per column: draws (split, z, folded z), sort keys in / out (all draws), sort values in / out, pair arrays;
    // rocPRIM's temporary storage is about one more keys + values
    const size_t per_col = CN * 8 * 7 + S * 4 * 4 + (size_t)N_ESS * M_pad * 8 + (size_t)N_KINDS * 2 * C * 16;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return -3;
    const size_t budget = std::min((size_t)4 << 30, free_b / 2);
    int G = (int)std::min<size_t>((size_t)ncols, std::max<size_t>(1, budget / per_col));
    G = (int)std::min<size_t>((size_t)G, (((size_t)1 << 31) - 1) / CN);
    if (G < 1) return -4;

    CallScratch sc;
    DiagArgs a{};
    a.C = C; a.N = N; a.M = M; a.S = S; a.CN = CN; a.npart = npart; a.chains_per_part = chains_per_part;
    a.nb = nb; a.M_pad = M_pad;
    double *keys_in = nullptr, *keys_out = nullptr;
    int32_t *vals_in = nullptr, *vals_out = nullptr;
    if (!(sc.alloc(&a.xs, (size_t)G * S) && sc.alloc(&a.mid, (size_t)G * C) && sc.alloc(&a.zs, (size_t)G * S) &&
          sc.alloc(&a.zf, (size_t)G * S) && sc.alloc(&a.info, (size_t)G * INFO_W) &&
          sc.alloc(&a.part, (size_t)G * nb * 4) && sc.alloc(&a.cmean, (size_t)G * N_KINDS * 2 * C) &&
          sc.alloc(&a.cvar, (size_t)G * N_KINDS * 2 * C) && sc.alloc(&a.kstat, (size_t)G * N_KINDS * 3) &&
          sc.alloc(&a.acm, (size_t)G * N_ESS * M_pad) && sc.alloc(&a.apart, (size_t)G * N_ESS * npart * LAG_BLOCK) &&
          sc.alloc(&a.tstate, (size_t)G * N_ESS) && sc.alloc(&a.live, (size_t)G * N_ESS) &&
          sc.alloc(&a.ess, (size_t)G * N_ESS) && sc.alloc(&a.maxlag, (size_t)G * N_ESS) &&
          sc.alloc(&a.live_count, 1) && sc.alloc(&a.out, (size_t)G * 7) && sc.alloc(&keys_in, (size_t)G * CN) &&
          sc.alloc(&keys_out, (size_t)G * CN) && sc.alloc(&vals_in, (size_t)G * S) &&
          sc.alloc(&vals_out, (size_t)G * S)))
        return -3;
    // rocPRIM's device-wide radix sort, one column at a time: a column's S or C N draws fill the whole device (the
    // segmented form gives each segment one workgroup, which is what a column of millions of draws cannot afford)
    size_t need_pairs = 0, need_keys = 0;
    if (rocprim::radix_sort_pairs(nullptr, need_pairs, keys_in, keys_out, vals_in, vals_out, S, 0, 64, st) != hipSuccess) return -3;
    if (!even && rocprim::radix_sort_keys(nullptr, need_keys, keys_in, keys_out, CN, 0, 64, st) != hipSuccess) return -3;
    size_t tmp_bytes = std::max(need_pairs, need_keys);
    char* tmp = nullptr;
    if (!sc.alloc(&tmp, tmp_bytes)) return -3;
    auto sort_pairs = [&](int ng) {
        for (int g = 0; g < ng; ++g) {
            const size_t o = (size_t)g * S;
            size_t tb = tmp_bytes;
            if (rocprim::radix_sort_pairs(tmp, tb, keys_in + o, keys_out + o, vals_in + o, vals_out + o, S, 0, 64, st) != hipSuccess)
                return false;
        }
        return true;
    };
    auto sort_all_keys = [&](int ng) {
        for (int g = 0; g < ng; ++g) {
            const size_t o = (size_t)g * CN;
            size_t tb = tmp_bytes;
            if (rocprim::radix_sort_keys(tmp, tb, keys_in + o, keys_out + o, CN, 0, 64, st) != hipSuccess) return false;
        }
        return true;
    };

    std::vector<double> h_out((size_t)G * 7);
    std::vector<int32_t> h_lag((size_t)G * N_ESS);
    for (int k0 = 0; k0 < ncols; k0 += G) {
        const int ng = std::min(G, ncols - k0);
        a.G = ng;
        const unsigned tiles = blocks_for(CN, 256);
        // gather: parameter columns k0 .. of the samples, then the values column
        const int np = std::max(0, std::min(ng, in.P - k0));
        if (np > 0)
            hipLaunchKernelGGL(diag_gather_kernel, dim3(tiles), dim3(256), 0, st, a, in.samples + k0, in.chain_stride, in.sample_stride, 0, np);
        if (np < ng)
            hipLaunchKernelGGL(diag_gather_kernel, dim3(tiles), dim3(256), 0, st, a, in.values, in.value_chain_stride, (size_t)1, np, 1);
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(diag_stats_partial_kernel, dim3(nb, ng), dim3(256), 0, st, a, pass);
            hipLaunchKernelGGL(diag_stats_final_kernel, dim3(blocks_for(ng, 64)), dim3(64), 0, st, a, pass);
        }
        if (!even) {
            hipLaunchKernelGGL(diag_all_keys_kernel, dim3(blocks_for((size_t)ng * CN, 256)), dim3(256), 0, st, a, keys_in);
            if (!sort_all_keys(ng)) return -3;
            hipLaunchKernelGGL(diag_all_quantiles_kernel, dim3(blocks_for(ng, 64)), dim3(64), 0, st, a, keys_out);
        }
        const unsigned sblocks = blocks_for((size_t)ng * S, 256);
        for (int fold = 0; fold < 2; ++fold) {
            hipLaunchKernelGGL(diag_split_keys_kernel, dim3(sblocks), dim3(256), 0, st, a, keys_in, vals_in, fold);
            if (!sort_pairs(ng)) return -3;
            hipLaunchKernelGGL(diag_rank_kernel, dim3(sblocks), dim3(256), 0, st, a, keys_out, vals_out, fold ? a.zf : a.zs);
            if (fold)
                hipLaunchKernelGGL(diag_fold_info_kernel, dim3(blocks_for(ng, 64)), dim3(64), 0, st, a, keys_out);
            else
                hipLaunchKernelGGL(diag_split_info_kernel, dim3(blocks_for(ng, 64)), dim3(64), 0, st, a, keys_out, even ? 1 : 0);
        }
        hipLaunchKernelGGL(diag_chain_moments_kernel, dim3(blocks_for((size_t)ng * N_KINDS * 2 * C * WAVE, 256)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(diag_kind_stats_kernel, dim3(ng * N_KINDS), dim3(256), 0, st, a);
        const int npairs = ng * N_ESS;
        hipLaunchKernelGGL(diag_init_pairs_kernel, dim3(blocks_for(npairs, 64)), dim3(64), 0, st, a);
        for (int t0 = 0; t0 < M; t0 += LAG_BLOCK) {
            hipLaunchKernelGGL(diag_acov_kernel, dim3(npairs, npart), dim3(256), 0, st, a, t0);
            hipLaunchKernelGGL(diag_acov_reduce_kernel, dim3(npairs), dim3(LAG_BLOCK), 0, st, a, t0);
            if (hipMemsetAsync(a.live_count, 0, sizeof(int32_t), st) != hipSuccess) return -3;
            hipLaunchKernelGGL(diag_geyer_kernel, dim3(blocks_for(npairs, 64)), dim3(64), 0, st, a, std::min(t0 + LAG_BLOCK, M));
            int32_t live = 0;
            if (hipMemcpyAsync(&live, a.live_count, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess) return -3;
            if (hipStreamSynchronize(st) != hipSuccess) return -3;
            if (live == 0) break;
        }
        hipLaunchKernelGGL(diag_finalize_kernel, dim3(blocks_for(ng, 64)), dim3(64), 0, st, a);
        if (hipMemcpyAsync(h_out.data(), a.out, (size_t)ng * 7 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return -3;
        if (hipMemcpyAsync(h_lag.data(), a.maxlag, (size_t)ng * N_ESS * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess) return -3;
        if (hipStreamSynchronize(st) != hipSuccess) return -3;
        std::copy(h_out.begin(), h_out.begin() + (size_t)ng * 7, out + (size_t)k0 * 7);
        if (max_lag) std::copy(h_lag.begin(), h_lag.begin() + (size_t)ng * N_ESS, max_lag + (size_t)k0 * N_ESS);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd
