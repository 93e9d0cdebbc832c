"""Posterior predictive draws with Poisson noise on the device (sepaihrd_ensemble_predictive, sepaihrd_poisson_device)
against the host twin, bit for bit: the twin is fed the device's own means and status and the problem's observations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
SEED = 0x1234_5678_9ABC_DEF0  # both words of the key in use


def _problem(mm, name, shipped, ref_fixture):
    if name == "ref":      # n = 4, 30 times, no run-up: x(t0) by the multiplier branch
        return ref_fixture, 0
    if name == "shipped":  # n = 4, 326 times, run-up offset 20
        return shipped, 1
    wide = mm.problem.widen_age_classes(shipped, 4)  # n = 16: sixteen lanes per chain
    return mm.workloads.with_synthetic_observations(wide, lambda p: mm.HipObjective(p)), 1


def _objective(mm, pb, mode, arith=None):
    hip = mm.HipObjective(pb.with_(arith=mm.ARITH_STRICT if arith is None else arith))
    hip.set_initial_state_mode(mode)
    return hip


def _check_against_twin(mm, pb, got, R, seed=SEED, probs=PROBS):
    twin = mm.hostabi.predictive_from_means(got["means"], got["status"], mm.hostabi.observed_table(pb), R, seed, probs)
    assert got["n_valid"] == twin["n_valid"] == int(np.sum(got["status"] == 0))
    assert np.array_equal(got["draws"], twin["draws"], equal_nan=True)
    assert np.array_equal(got["pred"], twin["pred"], equal_nan=True)
    assert np.array_equal(got["pit"], twin["pit"], equal_nan=True)
    return twin


@pytest.mark.parametrize("name,S,R,fma", [("ref", 1, 64, False), ("ref", 37, 3, False), ("ref", 37, 7, False), ("shipped", 5, 3, False), ("shipped", 37, 1, False),
                                          ("shipped", 5, 3, True), ("wide", 1, 3, False), ("wide", 5, 64, False)])
def test_device_equals_twin(mm, shipped, ref_fixture, name, S, R, fma):
    pb, mode = _problem(mm, name, shipped, ref_fixture)
    hip = _objective(mm, pb, mode, mm.ARITH_FMA if fma else mm.ARITH_STRICT)
    theta = mm.draws.jitter_draws(pb, 11, S)
    got = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True)
    Tp = int(np.sum(np.asarray(pb.times) >= 0))
    assert got["draws"].shape == (S, R, 3, Tp, pb.n) and got["n_valid"] > 0
    valid = got["status"] == 0
    assert (got["means"][valid] >= 0).all() and np.isnan(got["means"][~valid]).all()
    _check_against_twin(mm, pb, got, R)
    obs = mm.hostabi.observed_table(pb)
    usable = np.isfinite(obs) & (obs >= 0)
    assert usable.any() and np.isfinite(got["pit"][usable]).all() and np.isnan(got["pit"][~usable]).all()
    assert (got["pit"][usable] >= 0).all() and (got["pit"][usable] <= 1).all()


def test_means_are_the_ensembles_increments_and_the_context_is_left_unchanged(mm, shipped):
    S = 37
    hip = _objective(mm, shipped, 1)
    theta = mm.draws.jitter_draws(shipped, 11, S)
    before = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    got = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_means=True)
    after = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    assert before["n_valid"] == got["n_valid"] == S and np.array_equal(before["status"], got["status"])
    # S odd, all valid: positions 0, (S - 1) / 2 and S - 1 are order statistics, no interpolation
    srt = np.sort(got["means"], axis=0)  # [S][3][T_pos][n]
    assert np.array_equal(before["ppc"][:3], np.stack([srt[0], srt[(S - 1) // 2], srt[S - 1]], axis=1))
    for key in ("ppc", "sero", "rt", "status"):
        assert np.array_equal(before[key], after[key])
    ll = hip.eval_batch(theta[:4])["loglik"]
    assert np.array_equal(ll, _objective(mm, shipped, 1).eval_batch(theta[:4])["loglik"])


def test_failed_samples_are_padded_and_skipped(mm, oracle_py, shipped):
    """The attempt budget as tests/test_ensemble.py's test_hip_ensemble_skips_failed_samples sets it."""
    S, R = 50, 2
    theta = oracle_py.Oracle(shipped).jitter_draws(shipped.base_theta, 11, S, mode=1)
    probe = _objective(mm, shipped, 1)
    r = probe.eval_batch(theta)
    attempts = r["n_accept"] + r["n_reject"]
    budget = int(np.sort(attempts)[S // 2])
    hip = _objective(mm, shipped.with_(max_attempts=budget), 1)
    plain = hip.ensemble_quantiles(theta, PROBS)
    got = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True)
    assert 0 < got["n_valid"] < S and got["n_valid"] == plain["n_valid"]
    assert np.array_equal(got["status"], plain["status"])
    failed = got["status"] != 0
    assert np.isnan(got["draws"][failed]).all() and np.isnan(got["means"][failed]).all() and np.isfinite(got["draws"][~failed]).all()
    _check_against_twin(mm, shipped, got, R)
    # a valid sample's draws are those of the run in which nothing failed
    full = probe.ensemble_predictive(theta, R, SEED, PROBS, want_draws=True)
    assert np.array_equal(full["draws"][~failed], got["draws"][~failed])


def test_both_sort_paths(mm, ref_fixture):
    """R = 128: S = 128 gives 16384 draws per segment, the longest the LDS sort takes; S = 129 gives 16512, a multiple of 64
    and no power of two, sorted by the segmented radix sort."""
    R = 128
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 129)
    lds = hip.ensemble_predictive(theta[:128], R, SEED, PROBS, want_means=True, want_draws=True)
    _check_against_twin(mm, ref_fixture, lds, R)
    glob = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True)
    _check_against_twin(mm, ref_fixture, glob, R)
    assert lds["n_valid"] == 128 and glob["n_valid"] == 129
    assert np.array_equal(glob["draws"][:128], lds["draws"])


def test_draws_do_not_depend_on_the_call_around_them(mm, shipped):
    S = 12
    hip = _objective(mm, shipped, 1)
    theta = mm.draws.jitter_draws(shipped, 11, S)
    r4 = hip.ensemble_predictive(theta, 4, SEED, PROBS, want_draws=True)["draws"]
    r2 = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_draws=True)["draws"]
    assert np.array_equal(r2, r4[:, :2])
    sub = hip.ensemble_predictive(theta[:5], 4, SEED, PROBS, want_draws=True)["draws"]
    assert np.array_equal(sub, r4[:5])
    other = hip.ensemble_predictive(theta, 4, SEED + 1, PROBS, want_draws=True)["draws"]
    assert np.mean(other != r4) > 0.05  # most cells of the shipped problem have small means: equal draws are common


def test_probe_equals_the_host_sampler(mm, shipped):
    hip = mm.HipObjective(shipped)
    lam = np.repeat(np.array([1e-10, 1e-3, 0.5, 3, 9.999, 10, 10.001, 30, 1e3, 1e6, 1e9, 0.0, -1.0, np.nan, np.inf]), 4096)
    got = hip.poisson(lam, SEED)
    assert np.array_equal(got, mm.hostabi.poisson_probe(lam, SEED), equal_nan=True)
    assert not np.array_equal(got, hip.poisson(lam, SEED + 1), equal_nan=True)


def test_refused_arguments_on_the_device(mm, ref_fixture):
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 3)
    for R, probs, word in ((0, PROBS, "R must be >= 1"), (2 ** 30, PROBS, "S x R must stay below 2^31"), (2, [0.5, 1.5], "probabilities"),
                           (2 ** 29, PROBS, "device memory")):
        with pytest.raises(RuntimeError) as e:
            hip.ensemble_predictive(theta, R, SEED, probs)
        assert word in str(e.value), str(e.value)
    th = np.ascontiguousarray(theta)
    assert hip.lib.sepaihrd_eval_batch_begin(hip.ctx, th.ctypes.data, 3) == 0
    with pytest.raises(RuntimeError, match="sepaihrd_eval_batch_begin is pending"):
        hip.ensemble_predictive(theta, 2, SEED, PROBS)
    ll = np.empty(3)
    assert hip.lib.sepaihrd_eval_batch_end(hip.ctx, ll.ctypes.data, None, None, None, None) == 0
    assert hip.ensemble_predictive(theta, 2, SEED, PROBS)["n_valid"] >= 0
