"""Convergence diagnostics of C chains x N draws in numpy / scipy: the restatement of csrc/sepaihrd_diagnostics.hip.

The rank-normalised split R-hat and the bulk / tail effective sample sizes of Vehtari, Gelman, Simpson, Carpenter and
Buerkner (2021), following the R package `posterior` (1.x) function by function: split_chains, z_scale, fold_draws,
.rhat, .ess (Geyer's initial positive and monotone sequences) and ess_quantile.  Autocovariances are direct sums, formed
only up to the lag Geyer's truncation needs (posterior and Stan use an FFT over every lag).  This is the checker of the
device path and a CPU path for small sample sets; `chain_diagnostics` has the shape of sepaihrd_chain_diagnostics.
"""
from __future__ import annotations

import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

COLUMNS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "r_hat")
LAG_BLOCK = 64  # lags formed at a time, as on the device
EPS = np.finfo(np.float64).eps


def split_chains(x: np.ndarray) -> np.ndarray:
    """[C][N] -> [2C][M], M = N // 2: first and last M draws of each chain (odd N drops the middle draw)."""
    x = np.asarray(x, dtype=np.float64)
    C, N = x.shape
    M = N // 2
    out = np.empty((2 * C, M))
    out[0::2] = x[:, :M]
    out[1::2] = x[:, N - M:]
    return out


def quantile7(sorted_values: np.ndarray, q: float) -> float:
    """The project's type-7 rule on sorted values: v[floor pos] (1 - frac) + v[floor pos + 1] frac, pos = q (n - 1)."""
    n = sorted_values.size
    pos = q * (n - 1)
    idx = int(math.floor(pos))
    frac = pos - idx
    if idx + 1 < n:
        return float(sorted_values[idx] * (1.0 - frac) + sorted_values[idx + 1] * frac)
    return float(sorted_values[idx])


def z_scale(x: np.ndarray) -> np.ndarray:
    """Average ranks over all draws, z = Phi^-1((r - 3/8) / (S + 1/4))."""
    r = rankdata(x, method="average").reshape(x.shape)
    return ndtri((r - 0.375) / (x.size + 0.25))


def autocovariance(x: np.ndarray, max_lag: int | None = None) -> np.ndarray:
    """Biased autocovariance of one series by direct sums: acov_t = (1/M) sum_{i < M - t} d_i d_{i+t}, d = x - mean."""
    x = np.asarray(x, dtype=np.float64)
    M = x.size
    d = x - x.mean()
    T = M if max_lag is None else min(M, max_lag + 1)
    return np.array([np.dot(d[:M - t], d[t:]) / M for t in range(T)])


def _constant(x: np.ndarray) -> bool:
    return not (x.max() - x.min() >= EPS)


def rhat_basic(sims: np.ndarray) -> float:
    """posterior's .rhat of split chains [2C][M]: R = sqrt(((M - 1)/M W + var(m_j)) / W)."""
    if not np.all(np.isfinite(sims)) or _constant(sims):
        return math.nan
    M = sims.shape[1]
    W = np.mean(np.var(sims, axis=1, ddof=1))
    var_m = np.var(np.mean(sims, axis=1), ddof=1)
    return math.sqrt(((M - 1) / M * W + var_m) / W)


def ess_basic(sims: np.ndarray) -> tuple[float, int]:
    """posterior's .ess of split chains [2C][M] and Geyer's truncation lag max_t (NaN, -1 when it does not apply)."""
    nch, M = sims.shape
    if M < 3 or not np.all(np.isfinite(sims)) or _constant(sims):
        return math.nan, -1
    d = sims - sims.mean(axis=1, keepdims=True)
    acm = np.empty(M)
    have = 0

    def acov(t):  # mean over chains of acov_t, formed LAG_BLOCK lags at a time
        nonlocal have
        while t >= have:
            for u in range(have, min(have + LAG_BLOCK, M)):
                acm[u] = np.mean(np.einsum("ji,ji->j", d[:, :M - u], d[:, u:]) / M)
            have = min(have + LAG_BLOCK, M)
        return acm[t]

    mean_var = acov(0) * M / (M - 1)
    var_plus = mean_var * (M - 1) / M + np.var(sims.mean(axis=1), ddof=1)
    rho_t = np.zeros(M)
    t = 0
    rho_even = 1.0
    rho_t[0] = rho_even
    rho_odd = 1 - (mean_var - acov(1)) / var_plus
    rho_t[1] = rho_odd
    while t < M - 5 and not math.isnan(rho_even + rho_odd) and rho_even + rho_odd > 0:
        t += 2
        rho_even = 1 - (mean_var - acov(t)) / var_plus
        rho_odd = 1 - (mean_var - acov(t + 1)) / var_plus
        if rho_even + rho_odd >= 0:
            rho_t[t] = rho_even
            rho_t[t + 1] = rho_odd
    max_t = t
    if rho_even > 0:  # the improved estimate's last even term
        rho_t[max_t] = rho_even
    t = 0
    while t <= max_t - 4:  # initial monotone sequence
        t += 2
        if rho_t[t] + rho_t[t + 1] > rho_t[t - 2] + rho_t[t - 1]:
            rho_t[t] = (rho_t[t - 2] + rho_t[t - 1]) / 2
            rho_t[t + 1] = rho_t[t]
    # tau = -1 + 2 sum_{t < max_t} rho_t + rho_{max_t}; for max_t = 0 R's rho_hat_t[1:0] is rho_hat_t[1] = rho_0
    head = rho_t[0] if max_t == 0 else np.sum(rho_t[:max_t])
    tau = -1 + 2 * head + rho_t[max_t]
    total = nch * M
    tau = max(tau, 1 / math.log10(total))
    return total / tau, max_t


def column_diagnostics(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """One column, draws [C][N] -> (mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, r_hat), max_t [4] of the raw,
    z, I[x <= q05] and I[x <= q95] series."""
    x = np.asarray(x, dtype=np.float64)
    row = np.full(7, np.nan)
    lags = np.full(4, -1, dtype=np.int32)
    if not np.all(np.isfinite(x)) or _constant(x):
        return row, lags
    sims = split_chains(x)
    ess_mean, lags[0] = ess_basic(sims)
    z = z_scale(sims)
    ess_bulk, lags[1] = ess_basic(z)
    s_all = np.sort(x, axis=None)
    ess_q = []
    for k, q in enumerate((0.05, 0.95)):
        e, lags[2 + k] = ess_basic((sims <= quantile7(s_all, q)).astype(np.float64))
        ess_q.append(e)
    folded = np.abs(sims - np.median(sims))
    rz, rf = rhat_basic(z), rhat_basic(z_scale(folded))
    sd = float(np.std(x, ddof=1))
    row[:] = [float(np.mean(x)), sd, sd / math.sqrt(ess_mean), ess_mean, ess_bulk,
              math.nan if math.isnan(ess_q[0]) or math.isnan(ess_q[1]) else min(ess_q),
              math.nan if math.isnan(rz) or math.isnan(rf) else max(rz, rf)]
    return row, lags


def chain_diagnostics(samples: np.ndarray, values: np.ndarray | None = None, threads: int = 16) -> dict:
    """samples [C][N][P] (+ values [C][N]) -> table [P + (values given)][7] (values row last), max_lag [..][4]: what
    sepaihrd_chain_diagnostics computes, one column per task on `threads` threads."""
    s = np.asarray(samples, dtype=np.float64)
    if s.ndim != 3:
        raise ValueError("samples must be [C][N][P]")
    cols = [s[:, :, p] for p in range(s.shape[2])]
    if values is not None:
        cols.append(np.asarray(values, dtype=np.float64).reshape(s.shape[0], s.shape[1]))
    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        res = list(ex.map(column_diagnostics, cols))
    return {"table": np.array([r for r, _ in res]), "columns": list(COLUMNS),
            "max_lag": np.array([m for _, m in res], dtype=np.int32)}
