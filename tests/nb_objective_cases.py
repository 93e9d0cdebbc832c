"""What the tests of the negative-binomial observation model of the deterministic objective share (DESIGN.md section 6o;
tests/test_nb_objective_cpu.py, tests/test_gpu_nb_objective.py): the problems with dispersion entries, the increments of a
trajectory as the likelihood differences them, the observation grid of the twin, and the likelihood written out in Python."""
import math

import numpy as np

INF = float("inf")
DISPERSION_BOUNDS = (0.05, 200.0)
LGAMMA_K = (1e-3, 0.01, 0.5, 1.0, 3.0, 50.0, 1e6)


def with_dispersion(pb, names=("dispersion_H",), fixed=None, bounds=DISPERSION_BOUNDS):
    """pb with the named dispersions appended to its calibrated parameters (base value 5) and `fixed` [3] as the fixed values"""
    names = list(names)
    base = None if pb.base_theta is None else np.concatenate([pb.base_theta, np.full(len(names), 5.0)])
    bnd, sig = dict(pb.bounds), dict(pb.sigmas)
    for nm in names:
        bnd[nm], sig[nm] = bounds, 0.5
    return pb.with_(param_names=list(pb.param_names) + names, bounds=bnd, sigmas=sig, base_theta=base,
                    dispersion=None if fixed is None else [float(v) for v in fixed])


def increments(traj, n):
    """[B][T][3][n]: the daily differences of CumH, CumICU and D (series H, ICU, D) of traj [B][T][11 n]; row 0 has none"""
    B, T, _ = traj.shape
    inc = np.zeros((B, T, 3, n))
    for s, comp in enumerate((9, 10, 8)):
        x = traj[:, :, comp * n:(comp + 1) * n]
        inc[:, 1:, s, :] = x[:, 1:, :] - x[:, :-1, :]
    return inc


def observation_grid(pb):
    """obs_H, obs_ICU, obs_D as [T][n] on the output grid: NaN before t = 0 and beyond the observed rows"""
    out = []
    for obs in (pb.obs_H, pb.obs_ICU, pb.obs_D):
        g = np.full((pb.n_times, pb.n), np.nan)
        rows = min(pb.n_obs, pb.n_times - pb.runup_offset)
        g[pb.runup_offset:pb.runup_offset + rows] = obs[:rows]
        out.append(g)
    return out


def nb_logpmf(obs, sim, k):
    """log of the negative-binomial pmf with mean sim and size k at obs (tests/test_particle_nb_cpu.py writes the same)"""
    return (math.lgamma(obs + k) - math.lgamma(k) - math.lgamma(obs + 1.0) + k * math.log(k / (k + sim)) + obs * math.log(sim / (k + sim)))


def nb_logpmf_sound(obs, sim, k):
    """The same log-pmf for an integer obs without the two cancellations that cost nb_logpmf 1.2e-9 at k = 1e6 (measured against a
    40-digit evaluation; this form: 2e-15): lgamma(obs + k) - lgamma(k) as the sum of log(k + j), j < obs, and
    k log(k / (k + sim)) as -k log1p(sim / k)"""
    o = int(obs)
    assert o == obs and o >= 0
    head = math.fsum(math.log1p(j / k) for j in range(o)) + o * math.log(k)
    return head - math.lgamma(obs + 1.0) - k * math.log1p(sim / k) + obs * math.log(sim / (k + sim))


def python_cell(obs, inc, k):
    if not (obs >= 0.0 and math.isfinite(obs)):
        return 0.0
    sim = max(0.0, inc) + 1e-10
    if k == INF:
        return obs * math.log(sim) - sim
    return nb_logpmf(obs, sim, k) + math.lgamma(obs + 1.0)


def python_reference(inc, obs, k):
    """The likelihood in Python, summed in the stated order: ages ascending within a day, days ascending from 0.0 per series,
    total = (H + ICU) + D.  inc [B][T][3][n], obs = three [T][n], k [B][3] -> loglik [B], parts [B][3]"""
    B, T, _, n = inc.shape
    parts = np.zeros((B, 3))
    for b in range(B):
        for s in range(3):
            acc = 0.0
            for t in range(T):
                row = 0.0
                for a in range(n):
                    row += python_cell(obs[s][t, a], inc[b, t, s, a], k[b, s])
                acc += row
            parts[b, s] = acc
    return (parts[:, 0] + parts[:, 1]) + parts[:, 2], parts


def lgamma_grid(seed=20261021, n_random=400000):
    """10^U(-3, 6.1) and k + obs for k in LGAMMA_K, obs in 0 .. 3000"""
    rs = np.random.RandomState(seed)
    parts = [10.0 ** rs.uniform(-3.0, 6.1, n_random)]
    obs = np.arange(3001.0)
    for k in LGAMMA_K:
        parts.append(k + obs)
    return np.concatenate(parts)
