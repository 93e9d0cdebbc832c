"""Posterior predictive draws under the negative-binomial observation model, the parts that need no GPU:
the gamma sampler and the negative-binomial variate of csrc/sepaihrd_nb_draw.inc through the host twin (distribution, special
cases, stream coordinates), the dispersed twin of sepaihrd_ensemble_predictive_nb over the oracle's increments of the 30-day
fixture, the calibration of the mid-PIT under dispersed data, the declarations and the refused arguments."""
import math
import os

import numpy as np
import pytest

from nb_objective_cases import increments

DRAWS = 200_000
INF = float("inf")
SEED = 0x0F1E_2D3C_4B5A_6978
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
GAMMA_SHAPES = (0.05, 0.5, 1.0, 1.0001, 2.5, 10.0, 1e3, 1e6)
NB_CASES = ((1e-3, 100.0), (0.5, 3.0), (1.0, 9.5), (10.0, 30.0), (100.0, 0.5), (1e6, 30.0))


def test_declarations_are_present(mm):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sepaihrd_hip.h")).read()
    for name in ("sepaihrd_ensemble_predictive_nb", "sepaihrd_gamma_device", "sepaihrd_nb_draw_device"):
        assert name in mm.hipabi.EXPORTED_SYMBOLS and name + "(" in header
        assert hasattr(mm.hipabi.load_library(), name)
    assert mm.hipabi.ABI_VERSION == 3
    lib = mm.hostabi.load_library()
    for name in ("host_gamma_at", "host_nb_draw_at", "host_nb_draw_probe", "host_gamma_probe", "host_predictive_nb_from_means",
                 "host_predictive_dispersed"):
        assert hasattr(lib, name)
    for name in ("gamma_device", "nb_draw_device", "ensemble_predictive"):
        assert hasattr(mm.HipObjective, name)


# ---- the gamma sampler
@pytest.mark.parametrize("shape", GAMMA_SHAPES)
def test_gamma_distribution_against_scipy(mm, shape):
    from scipy import stats
    x = mm.hostabi.gamma_probe(np.full(DRAWS, shape), 20261021)
    assert np.all(x >= 0) and np.isfinite(x).all()
    pval = float(stats.kstest(x, stats.gamma(shape).cdf).pvalue)
    z = (float(x.mean()) - shape) / math.sqrt(shape / DRAWS)
    print("shape", shape, "KS p", pval, "z of the mean", z)
    assert pval >= 1e-6 and abs(z) <= 6.0


def test_gamma_below_the_smallest_double_is_zero_and_the_probe_is_the_variate(mm):
    host = mm.hostabi
    tiny = host.gamma_probe(np.full(4096, 1e-3), 5)  # the median of Gamma(1e-3) is about 1e-301: most variates underflow
    assert np.all(tiny >= 0) and np.isfinite(tiny).all() and 0.2 < np.mean(tiny == 0.0) < 0.9
    shapes = np.array([1e-3, 0.3, 1.0, 7.0, 1e6])
    x = host.gamma_probe(shapes, 77)
    for i, a in enumerate(shapes):
        assert host.gamma_at(77, i, 0, 0, a) == x[i]
    assert np.array_equal(host.gamma_probe(shapes, 77), x) and not np.array_equal(host.gamma_probe(shapes, 78), x)
    # no variate outside the open half line's closure for a shape that is none
    assert np.isnan(host.gamma_at(1, 2, 3, 4, float("nan"))) and np.isnan(host.gamma_at(1, 2, 3, 4, 0.0)) and np.isnan(host.gamma_at(1, 2, 3, 4, -1.0))


# ---- the negative-binomial variate
def chi_square_against(dist, draws):
    """p-value with the pooling rule of tests/test_predictive_cpu.py's chi_square_against_poisson: support cut at the 1e-9 tails
    with the tail mass folded into the end bins, neighbouring bins pooled left to right until the expected count is at least 10"""
    from scipy import stats
    lo, hi = int(dist.ppf(1e-9)), int(dist.isf(1e-9))
    k = np.arange(lo, hi + 1)
    prob = dist.pmf(k)
    prob[0] += dist.cdf(lo - 1)
    prob[-1] += dist.sf(hi)
    obs = np.bincount(np.clip(draws, lo, hi).astype(np.int64) - lo, minlength=len(k)).astype(np.float64)
    exp = prob * len(draws)
    O, E, o, e = [], [], 0.0, 0.0
    for oi, ei in zip(obs, exp):
        o, e = o + oi, e + ei
        if e >= 10.0:
            O.append(o); E.append(e)
            o = e = 0.0
    if e > 0.0 or o > 0.0:
        if O:
            O[-1] += o; E[-1] += e
        else:
            O.append(o); E.append(e)
    O, E = np.array(O), np.array(E)
    return 1.0 if len(O) < 2 else float(stats.chi2.sf(np.sum((O - E) ** 2 / E), len(O) - 1))


@pytest.mark.parametrize("k,mu", NB_CASES)
def test_nb_variate_distribution_against_scipy(mm, k, mu):
    from scipy import stats
    x = mm.hostabi.nb_draw_probe(np.full(DRAWS, mu), k, 20261021)
    assert np.all(x >= 0) and np.array_equal(x, np.floor(x))
    pval = chi_square_against(stats.nbinom(k, k / (k + mu)), x)
    var = mu + mu * mu / k
    z = (float(x.mean()) - mu) / math.sqrt(var / DRAWS)
    print("k", k, "mu", mu, "chi-square p", pval, "z of the mean", z)
    assert pval >= 1e-6 and abs(z) <= 6.0


def test_nb_variate_mean_and_variance(mm):
    """k = 5, mu = 1000: mean mu, variance mu + mu^2 / k.  The sample variance of N draws has standard error
    sqrt((m4 - var^2) / N) with the fourth central moment m4 = var^2 (3 + excess kurtosis); the negative binomial's excess
    kurtosis is 6 / k + p^2 / (k (1 - p)), p = k / (k + mu)."""
    k, mu = 5.0, 1000.0
    x = mm.hostabi.nb_draw_probe(np.full(DRAWS, mu), k, 11)
    var = mu + mu * mu / k
    p = k / (k + mu)
    kurt = 6.0 / k + p * p / (k * (1.0 - p))
    se_var = var * math.sqrt((2.0 + kurt) / DRAWS)
    z = (float(x.mean()) - mu) / math.sqrt(var / DRAWS)
    zv = (float(x.var(ddof=1)) - var) / se_var
    print("mean", x.mean(), "z", z, "variance", x.var(ddof=1), "expected", var, "z", zv)
    assert abs(z) <= 6.0 and abs(zv) <= 6.0


def test_special_cases(mm):
    host = mm.hostabi
    rs = np.random.RandomState(4)
    lam = np.exp(rs.uniform(np.log(1e-3), np.log(1e4), 1000))
    # k = +inf is the Poisson variate of the same coordinates, bit for bit
    for i in range(1000):
        c0, c1, c2 = i, (7 * i) % 13, 1000 + i
        assert host.nb_draw_at(SEED, c0, c1, c2, lam[i], INF) == host.poisson_at(SEED, c0, c1, c2, lam[i])
    assert np.array_equal(host.nb_draw_probe(lam, INF, 9), host.poisson_probe(lam, 9))
    for k in (INF, 1e-3, 0.5, 10.0, 1e6):
        x = host.nb_draw_probe([0.0, -0.0, -1.0, -1e300, -np.inf, np.nan, np.inf], k, 5)
        assert np.array_equal(x[:5], np.zeros(5)) and np.isnan(x[5]) and np.isnan(x[6])
    assert np.isnan(host.nb_draw_at(1, 2, 3, 4, 30.0, float("nan")))


def test_the_gamma_and_the_poisson_draw_have_coordinates_of_their_own(mm):
    """y = Poisson(mu (G / k)) on the Poisson call's own counters and G on the gamma's: with the gamma variate in hand the
    variate is reproduced from poisson_at; the gamma variate does not move with mu, the Poisson uniforms do not move with k."""
    host = mm.hostabi
    rs = np.random.RandomState(8)
    for i in range(300):
        c = (i, 3, 5 * i + 1)
        mu = float(np.exp(rs.uniform(np.log(0.05), np.log(3e3))))
        k = float(np.exp(rs.uniform(np.log(1e-2), np.log(1e4))))
        G = host.gamma_at(SEED, *c, k)
        assert host.nb_draw_at(SEED, *c, mu, k) == host.poisson_at(SEED, *c, mu * (G / k))
        assert host.nb_draw_at(SEED, *c, 7.0 * mu, k) == host.poisson_at(SEED, *c, 7.0 * mu * (G / k))
    # a k so large that G / k is 1 to within 1e-3: the finite-k variate stays next to the k = +inf variate of the cell, which it
    # could not if the change of k had moved the Poisson uniforms (PTRS maps its uniform to the count monotonically)
    mu = np.full(4096, 400.0)
    a, b = host.nb_draw_probe(mu, 1e6, 21), host.nb_draw_probe(mu, INF, 21)
    assert np.mean(np.abs(a - b) <= 3.0) > 0.95 and not np.array_equal(a, b)


# ---- the dispersed twin over the oracle's increments of the 30-day fixture
@pytest.fixture(scope="module")
def oracle_means(mm, oracle_py):
    """means [S][3][T_pos][n] of S = 6 jittered samples of the reference fixture (no run-up: every output time is >= 0), the
    problem and its observation table; computed once"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    pb = mm.SEPAIHRDProblem.load(os.path.join(golden, "reference_test_fixture.json")).with_(arith=mm.ARITH_STRICT)
    theta = mm.draws.jitter_draws(pb, 11, 6)
    theta[0] = pb.base_theta
    traj = oracle_py.Oracle(pb).eval_batch(theta, want_traj=True)["traj"]
    inc = increments(traj, pb.n)                                  # [S][T][3][n]
    means = np.ascontiguousarray(np.maximum(inc, 0.0).transpose(0, 2, 1, 3))
    means.setflags(write=False)
    return pb, means


def test_dispersed_twin_over_the_oracles_increments(mm, oracle_means):
    host = mm.hostabi
    pb, means = oracle_means
    S, _, Tp, n = means.shape
    R = 5
    obs = host.observed_table(pb)
    status = np.zeros(S, dtype=np.int32)
    status[4] = 2
    k_used = np.column_stack([np.array([0.07, 0.9, 5.0, 37.0, 180.0, 2e3]), np.full(S, INF), np.array([3.0, 3.0, 0.5, 0.5, 1e6, 1e-3])])
    assert len({tuple(r) for r in k_used}) == S  # the rows differ between samples
    got = host.predictive_from_means(means, status, obs, R, SEED, PROBS, k_used=k_used)
    plain = host.predictive_from_means(means, status, obs, R, SEED, PROBS)
    valid = status == 0
    assert got["n_valid"] == plain["n_valid"] == 5
    d = got["draws"]
    assert d.shape == (S, R, 3, Tp, n) and np.isnan(d[~valid]).all() and np.isfinite(d[valid]).all()
    assert np.array_equal(d[valid], np.floor(d[valid])) and (d[valid] >= 0).all()
    # the series at +inf has the undispersed twin's draws, quantiles (daily and cumulative) and PIT
    assert np.array_equal(d[:, :, 1], plain["draws"][:, :, 1], equal_nan=True)
    assert np.array_equal(got["pred"][[1, 4]], plain["pred"][[1, 4]]) and np.array_equal(got["pit"][1], plain["pit"][1], equal_nan=True)
    assert not np.array_equal(d[valid][:, :, 0], plain["draws"][valid][:, :, 0])
    # every draw is the variate at (s, r, (series T_pos + j) n + a) with the sample's own k
    for s, r, ser, j, a in ((0, 0, 0, 1, 0), (1, 4, 2, 7, 3), (2, 2, 0, 29, 1), (5, 3, 2, 12, 2), (3, 1, 1, 5, 0)):
        assert d[s, r, ser, j, a] == host.nb_draw_at(SEED, s, r, (ser * Tp + j) * n + a, means[s, ser, j, a] + 1e-10, k_used[s, ser])
    # the failed sample is left out of the counts: the quantiles are those of the pooled draws of the five others
    pooled = d[valid].reshape(-1, 3, Tp, n)
    both = np.sort(np.concatenate([pooled, np.cumsum(pooled, axis=2)], axis=1), axis=0)
    assert both.shape[0] == 25
    assert np.array_equal(got["pred"][:, 2], both[12])  # 25 draws: the median is an order statistic
    usable = np.isfinite(obs) & (obs >= 0)
    want = ((pooled < obs).sum(axis=0) + 0.5 * (pooled == obs).sum(axis=0)) / 25.0
    assert usable.any() and np.array_equal(got["pit"][usable], want[usable]) and np.isnan(got["pit"][~usable]).all()
    # all three series at +inf: the undispersed twin throughout
    allinf = host.predictive_from_means(means, status, obs, R, SEED, PROBS, k_used=np.full((S, 3), INF))
    for key in ("draws", "pred", "pit"):
        assert np.array_equal(allinf[key], plain[key], equal_nan=True)
    # the failed sample's k is not looked at (the device leaves a NaN there when a NaN theta entry failed the sample)
    k2 = k_used.copy()
    k2[4] = np.nan
    again = host.predictive_from_means(means, status, obs, R, SEED, PROBS, k_used=k2)
    for key in ("draws", "pred", "pit"):
        assert np.array_equal(again[key], got[key], equal_nan=True)


# ---- the point of the feature: replicates that match the noise the data has
GENERATING_K = 5.0
PIT_REPLICATES = 4000


def test_mid_pit_is_calibrated_under_the_dispersed_twin_and_not_under_the_poisson_twin(mm, oracle_means):
    """Observations synthesised as negative-binomial counts (k = GENERATING_K) around the oracle's increments at the base theta;
    the mid-PIT at that theta with S = 1 and R = 4000.  Of the N usable H cells those with a PIT outside [0.025, 0.975] number
    Binomial(N, 0.05) under a calibrated check (up to the discreteness of the counts, which only lowers the rate): at most
    0.05 N + 6 sqrt(0.05 0.95 N) under the dispersed twin at the generating k, more than that under the Poisson twin.
    On the 30-day fixture (H means from 0.21 to 141; N = 116, bound 19.9) with k = 5: 5 under the dispersed twin, 39 under the
    Poisson twin."""
    host = mm.hostabi
    pb, means = oracle_means
    m = means[:1]
    rs = np.random.RandomState(20261021)
    mu = m[0] + 1e-10
    obs = rs.poisson(rs.gamma(GENERATING_K, mu / GENERATING_K)).astype(np.float64)  # [3][T_pos][n]
    obs[:, 0] = np.nan  # the first output time has no increment
    status = np.zeros(1, dtype=np.int32)
    k_used = np.full((1, 3), GENERATING_K)
    nb = host.predictive_from_means(m, status, obs, PIT_REPLICATES, SEED, [0.5], want_draws=False, k_used=k_used)["pit"]
    po = host.predictive_from_means(m, status, obs, PIT_REPLICATES, SEED, [0.5], want_draws=False)["pit"]
    usable = np.isfinite(obs[0])
    N = int(usable.sum())
    bound = 0.05 * N + 6.0 * math.sqrt(0.05 * 0.95 * N)
    outside_nb = int(np.sum((nb[0][usable] < 0.025) | (nb[0][usable] > 0.975)))
    outside_po = int(np.sum((po[0][usable] < 0.025) | (po[0][usable] > 0.975)))
    print("usable H cells", N, "bound", bound, "outside under the dispersed twin", outside_nb, "under the Poisson twin", outside_po,
          "H means from", m[0, 0, 1:].min(), "to", m[0, 0, 1:].max())
    assert N >= 100
    assert outside_nb <= bound
    assert outside_po > bound


# ---- refused arguments
def test_refused_arguments_name_what_is_wrong(mm, oracle_means):
    host = mm.hostabi
    pb, means = oracle_means
    S = means.shape[0]
    status = np.zeros(S, dtype=np.int32)
    obs = host.observed_table(pb)
    for bad, word in ((0.0, "is not positive"), (1e-4, "1e-3"), (float("nan"), "NaN"), (-2.0, "is not positive"), (1e7, "1e6")):
        k = np.full((S, 3), 5.0)
        k[2, 1] = bad
        with pytest.raises(ValueError) as e:
            host.predictive_from_means(means, status, obs, 2, SEED, PROBS, k_used=k)
        assert word in str(e.value), (bad, str(e.value))
        with pytest.raises(ValueError) as e2:
            host.particle_nb_validate([5.0, bad, 5.0])   # the message is that function's
        assert str(e2.value) == str(e.value) and "k_ICU" in str(e.value)
    with pytest.raises(ValueError, match=r"k_used must be \[S\]\[3\]"):
        host.predictive_from_means(means, status, obs, 2, SEED, PROBS, k_used=np.full((S, 2), 5.0))
    with pytest.raises(ValueError, match="R must be >= 1"):
        host.predictive_from_means(means, status, obs, 0, SEED, PROBS, k_used=np.full((S, 3), 5.0))
    with pytest.raises(ValueError, match="probabilities"):
        host.predictive_from_means(means, status, obs, 2, SEED, [1.5], k_used=np.full((S, 3), 5.0))
