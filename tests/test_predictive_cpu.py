"""Posterior predictive draws with Poisson noise, the parts that need no GPU: the sampler of csrc/sepaihrd_poisson.inc
through the host twin (distribution, edge values, purity), the twin of sepaihrd_ensemble_predictive on hand-made means,
the calibration of the mid-PIT, the argument rules and the writers."""
import math
import os

import numpy as np
import pytest

DRAWS = 200_000
LAMBDAS = (1e-10, 1e-3, 0.5, 3, 9.999, 10, 10.001, 30, 1e3)


def chi_square_against_poisson(draws, lam):
    """(p-value, z of the sample mean) with the pooling rule of tests/test_stoch_sir_cpu.py's chi_square_against_binomial:
    support cut at the 1e-9 tails with the tail mass folded into the end bins, neighbouring bins pooled left to right until
    the expected count is at least 10."""
    from scipy import stats
    d = stats.poisson(lam)
    lo, hi = int(d.ppf(1e-9)), int(d.isf(1e-9))
    k = np.arange(lo, hi + 1)
    prob = d.pmf(k)
    prob[0] += d.cdf(lo - 1)
    prob[-1] += d.sf(hi)
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
    pval = 1.0 if len(O) < 2 else float(stats.chi2.sf(np.sum((O - E) ** 2 / E), len(O) - 1))
    z = (float(np.mean(draws, dtype=np.float64)) - lam) / math.sqrt(lam / len(draws))
    return pval, z


@pytest.mark.parametrize("lam", LAMBDAS)
def test_sampler_distribution_against_scipy(mm, lam):
    x = mm.hostabi.poisson_probe(np.full(DRAWS, lam), 20261018)
    assert np.all(x >= 0) and np.array_equal(x, np.floor(x))
    pval, z = chi_square_against_poisson(x, lam)
    print("lambda", lam, "p", pval, "z", z)
    assert pval >= 1e-6 and abs(z) <= 6.0


@pytest.mark.parametrize("lam", (1e6, 1e9))
def test_sampler_moments_at_large_means(mm, lam):
    x = mm.hostabi.poisson_probe(np.full(DRAWS, lam), 99)
    assert np.all(x >= 0) and np.array_equal(x, np.floor(x))
    z = (x.mean() - lam) / math.sqrt(lam / DRAWS)
    ratio = x.var(ddof=1) / lam
    # the sample variance of a near-normal variate has standard error sigma^2 sqrt(2 / (N - 1))
    se = math.sqrt(2.0 / (DRAWS - 1))
    print("lambda", lam, "z", z, "variance ratio", ratio, "se", se)
    assert abs(z) <= 6.0 and abs(ratio - 1.0) <= 6.0 * se


def test_sampler_edge_values(mm):
    host = mm.hostabi
    x = host.poisson_probe([0.0, -0.0, -1.0, -1e300, -np.inf, np.nan, np.inf], 5)
    assert np.array_equal(x[:5], np.zeros(5)) and np.isnan(x[5]) and np.isnan(x[6])
    assert np.isnan(host.poisson_at(1, 2, 3, 4, float("nan"))) and host.poisson_at(1, 2, 3, 4, 0.0) == 0.0
    big = host.poisson_probe(np.full(1000, 4e9), 6)  # beyond any 32-bit integer: the variate is a double
    assert np.all(big > 2.0 ** 31) and np.array_equal(big, np.floor(big))


def test_a_draw_is_a_pure_function_of_its_coordinates(mm):
    host = mm.hostabi
    rs = np.random.RandomState(3)
    lam = np.exp(rs.uniform(np.log(1e-3), np.log(1e4), 4096))
    a = host.poisson_probe(lam, 42)
    assert np.array_equal(a, host.poisson_probe(lam, 42))
    # the same (seed, index, lambda) whatever the array around it
    other = lam.copy()
    keep = np.arange(0, 4096, 7)
    mask = np.ones(4096, dtype=bool)
    mask[keep] = False
    other[mask] = rs.uniform(0.1, 50.0, int(mask.sum()))
    assert np.array_equal(host.poisson_probe(other, 42)[keep], a[keep])
    assert np.array_equal(host.poisson_probe(lam[:100], 42), a[:100])
    for i in (0, 1, 777, 4095):
        assert host.poisson_at(42, i, 0, 0, lam[i]) == a[i]
    # another seed, another coordinate: other draws
    assert np.mean(host.poisson_probe(lam, 43) != a) > 0.5
    big = lam > 20.0
    assert np.mean(np.array([host.poisson_at(42, i, 1, 0, lam[i]) for i in np.nonzero(big)[0][:200]]) != a[big][:200]) > 0.5
    # a seed's two words are both part of the key
    assert np.mean(host.poisson_probe(lam, 42 + (1 << 32)) != a) > 0.5


# ---- the twin of sepaihrd_ensemble_predictive on hand-made means
S_, TP_, N_, R_ = 5, 6, 2, 3
PROBS = [0.0, 0.025, 0.5, 0.9, 1.0]


def _hand_made():
    rs = np.random.RandomState(17)
    means = np.exp(rs.uniform(np.log(0.05), np.log(300.0), (S_, 3, TP_, N_)))
    means[1, 0, 2, 0] = 0.0
    status = np.zeros(S_, dtype=np.int32)
    status[3] = 3  # one failed sample
    obs = np.floor(means[0] * rs.uniform(0.5, 1.5, (3, TP_, N_)))
    obs[0, 1, 1] = np.nan
    obs[2, 4, 0] = -1.0
    return means, status, obs


def _np_quantile(pooled_sorted, q):
    pos = q * (len(pooled_sorted) - 1)
    idx = int(pos)
    frac = pos - idx
    return pooled_sorted[idx] * (1.0 - frac) + pooled_sorted[idx + 1] * frac if idx + 1 < len(pooled_sorted) else pooled_sorted[idx]


def test_twin_semantics_on_hand_made_means(mm):
    host = mm.hostabi
    means, status, obs = _hand_made()
    r = host.predictive_from_means(means, status, obs, R_, 7, PROBS)
    draws, pred, pit = r["draws"], r["pred"], r["pit"]
    assert draws.shape == (S_, R_, 3, TP_, N_) and pred.shape == (6, len(PROBS), TP_, N_) and pit.shape == (3, TP_, N_)
    assert r["n_valid"] == 4
    valid = status == 0
    assert np.isnan(draws[~valid]).all() and np.isfinite(draws[valid]).all()
    assert np.array_equal(draws[valid], np.floor(draws[valid])) and (draws[valid] >= 0).all()
    # every draw is the sampler's variate at (s, r, (k T_pos + j) n + a) with mean m + 1e-10
    for s, rr, k, j, a in ((0, 0, 0, 0, 0), (1, 2, 0, 2, 0), (2, 1, 2, 5, 1), (4, 2, 1, 3, 1)):
        assert draws[s, rr, k, j, a] == host.poisson_at(7, s, rr, (k * TP_ + j) * N_ + a, means[s, k, j, a] + 1e-10)
    # the quantiles: daily series of the pooled draws of the valid samples, series 3 .. 5 of their running sums in time
    pooled = draws[valid].reshape(-1, 3, TP_, N_)
    both = np.concatenate([pooled, np.cumsum(pooled, axis=2)], axis=1)  # [draw][6][T_pos][n]
    srt = np.sort(both, axis=0)
    for p, q in enumerate(PROBS):
        want = np.array([[[_np_quantile(srt[:, ser, j, a], q) for a in range(N_)] for j in range(TP_)] for ser in range(6)])
        assert np.array_equal(pred[:, p], want)
    # mid-PIT: the formula, NaN at the unusable observations
    usable = np.isfinite(obs) & (obs >= 0)
    assert not usable[0, 1, 1] and not usable[2, 4, 0] and usable.sum() == obs.size - 2
    want = ((pooled < obs).sum(axis=0) + 0.5 * (pooled == obs).sum(axis=0)) / (4 * R_)
    assert np.array_equal(pit[usable], want[usable]) and np.isnan(pit[~usable]).all()
    # the failed sample's means change nothing else
    other = means.copy()
    other[3] = 1234.5
    r2 = host.predictive_from_means(other, status, obs, R_, 7, PROBS)
    assert np.array_equal(r2["pred"], pred) and np.array_equal(r2["pit"], pit, equal_nan=True)
    assert np.array_equal(r2["draws"], draws, equal_nan=True)
    # the first 2 replicates of the R = 3 run are the R = 2 run
    assert np.array_equal(host.predictive_from_means(means, status, obs, 2, 7, PROBS)["draws"], draws[:, :2], equal_nan=True)
    # dropping the last sample leaves the others' draws unchanged (a sample's stream is set by its position in theta)
    assert np.array_equal(host.predictive_from_means(means[:4], status[:4], obs, R_, 7, PROBS)["draws"], draws[:4], equal_nan=True)
    # and the draws of a sample do not depend on which other samples failed
    st2 = status.copy()
    st2[0] = 2
    d2 = host.predictive_from_means(means, st2, obs, R_, 7, PROBS)["draws"]
    assert np.array_equal(d2[[1, 2, 4]], draws[[1, 2, 4]]) and np.isnan(d2[0]).all()
    # another seed: other draws
    assert np.mean(host.predictive_from_means(means, status, obs, R_, 8, PROBS)["draws"][valid] != draws[valid]) > 0.3


def test_twin_order_statistics_with_an_odd_count(mm):
    """S R = 15 values per segment and probs {0, 0.5, 1}: positions 0, 7 and 14, no interpolation."""
    host = mm.hostabi
    means, _, obs = _hand_made()
    r = host.predictive_from_means(means, np.zeros(S_, dtype=np.int32), obs, R_, 11, [0.0, 0.5, 1.0])
    pooled = r["draws"].reshape(-1, 3, TP_, N_)
    srt = np.sort(np.concatenate([pooled, np.cumsum(pooled, axis=2)], axis=1), axis=0)
    assert srt.shape[0] == 15
    assert np.array_equal(r["pred"], np.stack([srt[0], srt[7], srt[14]], axis=1))
    # no valid sample at all: NaN everywhere
    none = host.predictive_from_means(means, np.full(S_, 3, dtype=np.int32), obs, R_, 11, [0.5])
    assert np.isnan(none["pred"]).all() and np.isnan(none["pit"]).all() and np.isnan(none["draws"]).all()


def test_mid_pit_is_calibrated_under_the_model_and_not_under_a_shifted_one(mm):
    """Observations drawn from Poisson(mean): the mid-PIT of a correctly specified count has mean exactly 0.5 and variance at
    most 1/12; its estimate from N draws adds at most 1/(4 N) per cell.  So the mean over the cells lies within
    6 sqrt((1/12 + 1/(4 N)) / cells) of 0.5 -- and far outside when the observations come from Poisson(2 mean)."""
    host = mm.hostabi
    Tp, n, N = 170, 4, 256
    cells = 3 * Tp * n
    assert cells >= 2000
    means = np.exp(np.linspace(np.log(0.2), np.log(500.0), cells)).reshape(1, 3, Tp, n)
    rs = np.random.RandomState(20261018)
    bound = 6.0 * math.sqrt((1.0 / 12.0 + 1.0 / (4.0 * N)) / cells)
    status = np.zeros(1, dtype=np.int32)
    good = host.predictive_from_means(means, status, rs.poisson(means[0]).astype(np.float64), N, 5, [0.5], want_draws=False)["pit"]
    bad = host.predictive_from_means(means, status, rs.poisson(2.0 * means[0]).astype(np.float64), N, 5, [0.5], want_draws=False)["pit"]
    print("mean mid-PIT", good.mean(), "shifted", bad.mean(), "bound", bound)
    assert np.isfinite(good).all() and abs(good.mean() - 0.5) <= bound
    assert abs(bad.mean() - 0.5) > bound


def test_refused_arguments_name_what_is_wrong(mm):
    host = mm.hostabi
    host.predictive_validate(5, 3, 6, 2, [0.0, 0.5, 1.0])
    for args, word in (((5, 0, 6, 2, [0.5]), "R must be >= 1"),
                       ((5, -4, 6, 2, [0.5]), "R must be >= 1"),
                       ((0, 3, 6, 2, [0.5]), "S must be >= 1"),
                       ((2, 2 ** 30, 6, 2, [0.5]), "S x R must stay below 2^31"),
                       ((2 ** 16, 2 ** 15, 6, 2, [0.5]), "S x R must stay below 2^31"),
                       ((5, 3, 2 ** 27, 16, [0.5]), "3 x T_pos x n_age must stay below 2^32"),
                       ((5, 3, 6, 2, [0.5, 1.5]), "probabilities must lie in [0, 1]"),
                       ((5, 3, 6, 2, [-1e-9]), "probabilities must lie in [0, 1]"),
                       ((5, 3, 6, 2, [float("nan")]), "probabilities must lie in [0, 1]")):
        with pytest.raises(ValueError) as e:
            host.predictive_validate(*args)
        assert word in str(e.value), (args, str(e.value))
    host.predictive_validate(1, 2 ** 31 - 1, 6, 2, [0.5])  # the largest count of draws that passes
    means, status, obs = _hand_made()
    with pytest.raises(ValueError, match="R must be >= 1"):
        host.predictive_from_means(means, status, obs, 0, 7, PROBS)
    with pytest.raises(ValueError, match="probabilities"):
        host.predictive_from_means(means, status, obs, R_, 7, [2.0])
    with pytest.raises(ValueError, match="S x R"):
        host.predictive_from_means(means[:2], status[:2], obs, 2 ** 30, 7, PROBS, want_draws=False)
    # the entry points are declared and exported
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sepaihrd_hip.h")).read()
    for name in ("sepaihrd_ensemble_predictive", "sepaihrd_poisson_device", "sepaihrd_predictive_validate"):
        assert name in mm.hipabi.EXPORTED_SYMBOLS and name + "(" in header
    assert mm.hipabi.ABI_VERSION == 3


def test_writers(mm, tmp_path):
    cio = mm.config_io
    Tp, n = 4, 2
    times = [0.0, 1.0, 2.0, 3.5]
    rs = np.random.RandomState(1)
    pred = np.sort(rs.poisson(20.0, (6, 5, Tp, n)).astype(np.float64), axis=1)
    pred[:, 2] += 0.5  # an interpolated median
    pit = rs.randint(0, 97, (3, Tp, n)) / 96.0 / 3.0
    pit[1, 2, 0] = np.nan
    inside = 0.5 * (pred[:3, 1] + pred[:3, 3])  # within the 90 % band of every cell
    observed = {"daily_hospitalizations": inside[0], "daily_icu_admissions": pred[1, 4] + 1.0, "daily_deaths": inside[2].copy()}
    observed["daily_deaths"][0, 0] = np.nan
    observed["daily_deaths"][1, 0] = -2.0
    out = str(tmp_path / "posterior_predictive")
    written = cio.write_posterior_predictive_draws(out, times, pred, pit, observed)
    names = sorted(os.path.basename(p) for p in written)
    want = sorted([f"{s}_predictive_{q}.csv" for s in cio.PPC_SERIES for q in ("median", "lower90", "upper90", "lower95", "upper95")] +
                  [f"pit_{s}.csv" for s in cio.PPC_SERIES[:3]] + ["predictive_coverage.csv"])
    assert names == want and sorted(os.listdir(out)) == want
    suffix_of = dict(zip(("lower95", "lower90", "median", "upper90", "upper95"), range(5)))
    for si, s in enumerate(cio.PPC_SERIES):
        for q, pi in suffix_of.items():
            lines = open(os.path.join(out, f"{s}_predictive_{q}.csv")).read().split("\n")
            assert lines[0] == "time,age_0,age_1" and lines[-1] == "" and len(lines) == Tp + 2
            assert [l.split(",")[0] for l in lines[1:-1]] == ["0", "1", "2", "3.5"]
            got = np.array([[float(c) for c in l.split(",")[1:]] for l in lines[1:-1]])
            assert np.array_equal(got, pred[si, pi])  # counts and halves: exact in 6 digits
    for si, s in enumerate(cio.PPC_SERIES[:3]):
        lines = open(os.path.join(out, f"pit_{s}.csv")).read().split("\n")
        assert lines[0] == "time,age_0,age_1"
        got = np.array([[float(c) for c in l.split(",")[1:]] for l in lines[1:-1]])
        assert np.array_equal(got, pit[si], equal_nan=True)  # 17 significant digits: the round trip is exact
    cov = open(os.path.join(out, "predictive_coverage.csv")).read().split("\n")
    assert cov[0] == "series,age,n_observations,coverage_90,coverage_95" and len(cov) == 1 + 3 * n + 1
    rows = {(c.split(",")[0], int(c.split(",")[1])): c.split(",")[2:] for c in cov[1:-1]}
    assert rows[("daily_hospitalizations", 0)] == ["4", "1.000000", "1.000000"]     # bands that contain everything
    assert rows[("daily_icu_admissions", 1)] == ["4", "0.000000", "0.000000"]       # bands that contain nothing
    assert rows[("daily_deaths", 0)] == ["2", "1.000000", "1.000000"]               # the unusable observations do not count
    # no PIT, no observations: the bands alone and an empty coverage table
    out2 = str(tmp_path / "bands_only")
    w2 = cio.write_posterior_predictive_draws(out2, times, pred, None, {})
    assert len(w2) == 31 and open(os.path.join(out2, "predictive_coverage.csv")).read() == "series,age,n_observations,coverage_90,coverage_95\n"
    # the tree writer adds the files only when it is given predictive results
    ens = {"ppc": pred}
    samples = rs.normal(size=(8, 2))
    cio.write_post_calibration_tree(str(tmp_path / "a"), times, ens, samples, ["p", "q"], n)
    cio.write_post_calibration_tree(str(tmp_path / "b"), times, ens, samples, ["p", "q"], n, observed=observed, predictive={"pred": pred, "pit": pit})
    a, b = (set(os.listdir(str(tmp_path / d / "posterior_predictive"))) for d in ("a", "b"))
    assert not any("predictive_" in f or f.startswith("pit_") for f in a)
    assert {f for f in b - a if "observed" not in f} == set(want)
    for f in a:
        assert open(str(tmp_path / "a" / "posterior_predictive" / f)).read() == open(str(tmp_path / "b" / "posterior_predictive" / f)).read()
