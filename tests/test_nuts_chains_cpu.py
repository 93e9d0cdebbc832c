"""MultiChainNUTSSampler without a GPU: the lock-step scheduler over an analytic objective (a correlated Gaussian's
log-density with its exact gradient, host_nuts_chains_analytic) against chain-by-chain HipNUTSSampler runs on the same
objective, and against the Gaussian itself."""
import numpy as np
import pytest

TRACES = ("samples", "sample_values", "epsilon_trace", "depth_trace", "n_samples", "gradient_calls", "best", "best_value")


def _gaussian(D, rho=0.9):
    """Mean, covariance and precision of an AR(1)-correlated Gaussian with unequal scales: narrow and tilted enough that
    trees have to double several times, and differently from start to start."""
    scale = np.linspace(0.3, 3.0, D)
    corr = rho ** np.abs(np.subtract.outer(np.arange(D), np.arange(D)))
    cov = corr * np.outer(scale, scale)
    return np.linspace(-1.0, 2.0, D), cov, np.linalg.inv(cov)


def _starts(C, mean, cov, seed):
    rng = np.random.default_rng(seed)
    return mean + rng.standard_normal((C, len(mean))) @ np.linalg.cholesky(cov).T * 1.5


@pytest.fixture(scope="module")
def runs(mm):
    """lock-step and solo runs of the shared cases, computed once"""
    out = {}
    for D in (3, 6):
        mean, cov, prec = _gaussian(D)
        th0 = _starts(5, mean, cov, 10 + D)
        kw = dict(seed0=21, iterations=30, adaptation_window=10, max_tree_depth=5)
        out[D] = (mm.hostabi.nuts_chains_analytic(mean, prec, th0, **kw),
                  mm.hostabi.nuts_chains_analytic(mean, prec, th0, lock_step=False, **kw))
    return out


@pytest.mark.parametrize("D", [3, 6])
def test_lock_step_equals_solo(runs, D):
    lock, solo = runs[D]
    depth = lock["depth_trace"]
    # the inputs put the chains out of phase: deep trees, and not the same ones in every chain
    assert depth.max() >= 3 and any(not np.array_equal(depth[0], depth[c]) for c in range(1, 5))
    assert np.all(lock["n_samples"] == 30) and np.all(lock["failure_status"] == 0)
    for k in TRACES:
        assert np.array_equal(lock[k], solo[k]), k
    # the rows that ran are the solo sampler's launches plus the value-only rows its cache would have answered or not
    assert np.all(lock["rows_evaluated"] >= solo["rows_evaluated"])
    assert np.all(lock["rows_evaluated"] <= solo["rows_evaluated"] + 30)


def test_single_chain_equals_the_single_chain_sampler(mm):
    mean, cov, prec = _gaussian(4)
    th0 = _starts(1, mean, cov, 3)
    kw = dict(seed0=5, iterations=25, adaptation_window=8, max_tree_depth=6)
    lock = mm.hostabi.nuts_chains_analytic(mean, prec, th0, **kw)
    solo = mm.hostabi.nuts_chains_analytic(mean, prec, th0, lock_step=False, **kw)
    for k in TRACES:
        assert np.array_equal(lock[k], solo[k]), k
    assert lock["depth_trace"].max() >= 2 and lock["mean_rows_per_tick"] == 1.0


def test_failing_chain_stops_and_the_others_run_on(mm):
    mean, cov, prec = _gaussian(3)
    th0 = _starts(5, mean, cov, 13)
    kw = dict(seed0=21, iterations=30, adaptation_window=10, max_tree_depth=5)
    free = mm.hostabi.nuts_chains_analytic(mean, prec, th0, lock_step=False, **kw)
    # a failure ball around a state chain 2 visits late in its run (and that is not its starting point)
    victim, when = 2, 17
    centre = free["samples"][victim, when]
    radius = 1e-3
    dist = np.linalg.norm(np.concatenate([free["samples"].reshape(-1, 3), th0]) - centre, axis=1)
    others = np.ones(len(dist), dtype=bool)
    others[victim * 30:(victim + 1) * 30] = False
    others[150 + victim] = False
    assert dist[others].min() > 10 * radius and np.linalg.norm(th0[victim] - centre) > 10 * radius
    lock = mm.hostabi.nuts_chains_analytic(mean, prec, th0, fail_centre=centre, fail_radius=radius, **kw)
    solo = mm.hostabi.nuts_chains_analytic(mean, prec, th0, lock_step=False, fail_centre=centre, fail_radius=radius, **kw)
    assert solo["failure_status"][victim] == 2 and solo["n_samples"][victim] == 0  # the exception took its samples
    assert lock["failure_status"][victim] == 2
    kept = lock["n_samples"][victim]
    # it met the ball while building the tree of iteration `when` + 1 at the latest; what it had sampled before stays
    assert 0 < kept <= when and lock["failure_iteration"][victim] == kept + 1
    assert np.array_equal(lock["samples"][victim, :kept], free["samples"][victim, :kept])
    assert np.array_equal(lock["sample_values"][victim, :kept], free["sample_values"][victim, :kept])
    assert np.all(np.isnan(lock["samples"][victim, kept:]))
    for c in range(5):
        if c == victim:
            continue
        assert lock["failure_status"][c] == 0 and lock["failure_iteration"][c] == -1
        for k in TRACES:
            assert np.array_equal(lock[k][c], solo[k][c]), (k, c)
            assert np.array_equal(lock[k][c], free[k][c]), (k, c)


@pytest.mark.parametrize("D", [3, 6])
def test_requests_are_batched(runs, D):
    lock, _ = runs[D]
    # in lock step every live chain has one row in every tick: the slowest chain sets the length
    assert lock["ticks"] <= 1.2 * lock["rows_evaluated"].max()
    assert lock["rows_total"] == lock["rows_evaluated"].sum()
    assert lock["mean_rows_per_tick"] > 0.8 * 5


def test_pooled_draws_follow_the_gaussian(mm):
    """64 chains x 400 iterations after a window of 200: pooled mean and covariance within 5 Monte-Carlo standard
    errors.  The error is measured, not tuned: the chains are independent, so the standard error of the pooled estimate
    is the spread of the 64 per-chain means over sqrt(64) -- autocorrelation within a chain included, which is the
    Monte-Carlo error at the effective sample size the run has."""
    mean = np.array([0.5, -1.0])
    cov = np.array([[1.0, 0.8], [0.8, 2.0]])
    C, warm, keep = 64, 200, 400
    th0 = _starts(C, mean, cov, 99)
    r = mm.hostabi.nuts_chains_analytic(mean, np.linalg.inv(cov), th0, seed0=1000, iterations=warm + keep, adaptation_window=warm,
                                        max_tree_depth=8)
    assert np.all(r["n_samples"] == warm + keep) and np.all(r["failure_status"] == 0)
    x = r["samples"][:, warm:, :]  # [C][keep][2]
    # statistics whose expectation is known: the coordinates and the centred products
    d = x - mean
    stats = np.stack([x[..., 0], x[..., 1], d[..., 0] * d[..., 0], d[..., 0] * d[..., 1], d[..., 1] * d[..., 1]], axis=-1)
    truth = np.array([mean[0], mean[1], cov[0, 0], cov[0, 1], cov[1, 1]])
    per_chain = stats.mean(axis=1)                      # [C][5], independent across chains
    pooled = per_chain.mean(axis=0)
    stderr = per_chain.std(axis=0, ddof=1) / np.sqrt(C)  # Monte-Carlo error of the pooled estimate at the measured ESS
    ess = stats.reshape(-1, 5).var(axis=0, ddof=1) / (stderr ** 2)
    assert np.all(ess > 0.05 * C * keep), ess           # the sampler mixes: far from one draw per chain
    assert np.all(np.abs(pooled - truth) <= 5.0 * stderr), (pooled, truth, stderr)
    # and the error bar itself is small enough to catch a wrong scale: a tenth of each statistic's spread at most
    assert np.all(stderr < 0.1 * np.sqrt(stats.reshape(-1, 5).var(axis=0)))
