"""Scores of the posterior predictive draws against data on the device (sepaihrd_ensemble_predictive_scores)
against the host twin, bit for bit: the twin is fed the device's own means, status and k_used and the table scored against.  The
shapes are those of tests/test_gpu_predictive_nb.py: one draw in a pad of 64, exactly one wavefront, a padded segment across a
256-lane workgroup, the run-up offset, sixteen ages, the longest LDS sort and the radix route."""
import numpy as np
import pytest

from nb_objective_cases import with_dispersion

pytestmark = pytest.mark.gpu

INF = float("inf")
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
LEVELS = [0.5, 0.9, 0.95]
SEED = 0x1234_5678_9ABC_DEF0  # both words of the key in use
MIXED = (0.5, 10.0, INF)      # the boost branch, Cheng's branch and a Poisson series in one launch
TWIN_KEYS = ("cell_scores", "summary", "pit", "pred", "draws")
NB_KEYS = ("pred", "pit", "means", "draws", "k_used", "status")


def _problem(mm, name, shipped, ref_fixture):
    if name == "ref":      # n = 4, 30 times, no run-up
        return ref_fixture, 0
    if name == "shipped":  # n = 4, 326 times, run-up offset 20
        return shipped, 1
    wide = mm.problem.widen_age_classes(shipped, 4)  # n = 16
    return mm.workloads.with_synthetic_observations(wide, lambda p: mm.HipObjective(p)), 1


def _objective(mm, pb, mode, arith=None):
    hip = mm.HipObjective(pb.with_(arith=mm.ARITH_STRICT if arith is None else arith))
    hip.set_initial_state_mode(mode)
    return hip


def _score(hip, theta, R, dispersion=MIXED, observed=None, levels=LEVELS, seed=SEED, probs=PROBS):
    return hip.ensemble_predictive_scores(theta, R, seed, probs, levels, observed=observed, dispersion=dispersion, want_means=True,
                                          want_draws=True)


def _check_against_twin(mm, got, R, levels=LEVELS, seed=SEED, probs=PROBS):
    twin = mm.hostabi.predictive_scores_from_means(got["means"], got["status"], got["observed"], R, seed, probs, levels, k_used=got["k_used"])
    assert got["n_valid"] == twin["n_valid"] == int(np.sum(got["status"] == 0))
    assert got["exact"] is True and twin["exact"] is True
    for key in TWIN_KEYS:
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    return twin


@pytest.mark.parametrize("name,S,R,fma", [("ref", 1, 1, False), ("ref", 1, 64, False), ("ref", 37, 7, False), ("shipped", 5, 3, False),
                                          ("shipped", 5, 3, True), ("wide", 5, 64, False)])
def test_device_equals_twin(mm, shipped, ref_fixture, name, S, R, fma):
    pb, mode = _problem(mm, name, shipped, ref_fixture)
    hip = _objective(mm, pb, mode, mm.ARITH_FMA if fma else mm.ARITH_STRICT)
    theta = mm.draws.jitter_draws(pb, 11, S)
    got = _score(hip, theta, R)
    Tp = int(np.sum(np.asarray(pb.times) >= 0))
    L = len(LEVELS)
    assert got["cell_scores"].shape == (3, Tp, pb.n, 5 + 4 * L) and got["summary"].shape == (3, pb.n + 1, 4 + 2 * L) and got["n_valid"] > 0
    assert np.array_equal(got["observed"], mm.hostabi.observed_table(pb), equal_nan=True)
    _check_against_twin(mm, got, R)
    usable = np.isfinite(got["observed"]) & (got["observed"] >= 0)
    assert usable.any() and np.isfinite(got["crps"][usable]).all() and np.isnan(got["crps"][~usable]).all()
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["median"]).all()
    assert np.isnan(got["variance"]).all() if got["n_valid"] * R == 1 else np.isfinite(got["variance"]).all()
    assert np.array_equal(got["summary_count"][:, :pb.n], usable.sum(axis=1))
    # observed = None: every output it shares with sepaihrd_ensemble_predictive_nb is that call's
    nb = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True, dispersion=MIXED)
    for key in NB_KEYS:
        assert np.array_equal(got[key], nb[key], equal_nan=True), key
    assert got["n_valid"] == nb["n_valid"]


@pytest.mark.parametrize("name,S,R", [("shipped", 5, 3), ("ref", 37, 7)])
def test_all_series_at_infinity_is_the_poisson_call(mm, shipped, ref_fixture, name, S, R):
    pb, mode = _problem(mm, name, shipped, ref_fixture)
    hip = _objective(mm, pb, mode)
    theta = mm.draws.jitter_draws(pb, 11, S)
    plain = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True)
    for dispersion in ((INF, INF, INF), hip.CONTEXT_DISPERSION):  # the context's default is +inf throughout
        got = _score(hip, theta, R, dispersion)
        for key in ("pred", "pit", "means", "draws", "status"):
            assert np.array_equal(got[key], plain[key], equal_nan=True), key
        assert got["n_valid"] == plain["n_valid"] and np.isposinf(got["k_used"]).all()
        _check_against_twin(mm, got, R)


def test_both_sort_routes(mm, ref_fixture):
    """R = 128: S = 128 gives 16384 draws per segment, the longest the LDS sort takes (128 KiB of draws and the cross-wave step next
    to them: the raised dynamic-LDS limit); S = 129 gives 16512, sorted by the segmented radix sort and scored over its scratch."""
    R = 128
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 129)
    lds = _score(hip, theta[:128], R)
    _check_against_twin(mm, lds, R)
    glob = _score(hip, theta, R)
    _check_against_twin(mm, glob, R)
    assert lds["n_valid"] == 128 and glob["n_valid"] == 129
    assert np.array_equal(glob["draws"][:128], lds["draws"])
    nb = hip.ensemble_predictive(theta, R, SEED, PROBS, dispersion=MIXED)
    assert np.array_equal(glob["pred"], nb["pred"]) and np.array_equal(glob["pit"], nb["pit"], equal_nan=True)


def test_failed_samples_are_left_out(mm, oracle_py, shipped):
    """The attempt budget as tests/test_gpu_predictive_nb.py's test_failed_samples_are_padded_and_skipped sets it: m = n_valid R, and
    the scores are those of a run over the valid samples alone."""
    S, R = 50, 2
    theta = oracle_py.Oracle(shipped).jitter_draws(shipped.base_theta, 11, S, mode=1)
    probe = _objective(mm, shipped, 1)
    r = probe.eval_batch(theta)
    budget = int(np.sort(r["n_accept"] + r["n_reject"])[S // 2])
    hip = _objective(mm, shipped.with_(max_attempts=budget), 1)
    got = _score(hip, theta, R)
    failed = got["status"] != 0
    assert 0 < got["n_valid"] < S and np.isnan(got["draws"][failed]).all()
    twin = _check_against_twin(mm, got, R)
    # the twin over the valid samples alone: their draws sit at other stream coordinates, so feed it the draws' own positions
    keep = np.flatnonzero(~failed)
    m = got["n_valid"] * R
    pooled = got["draws"][keep].reshape(m, 3, -1, shipped.n)
    for ser, t, a in ((0, 3, 1), (1, 100, 0), (2, 250, 3)):
        one = mm.hostabi.score_cell(pooled[:, ser, t, a], got["observed"][ser, t, a], LEVELS)
        assert np.array_equal(one["scores"], got["cell_scores"][ser, t, a], equal_nan=True)
    assert np.array_equal(twin["mean"], pooled.sum(axis=0) / m)


def test_a_nan_dispersion_entry_fails_its_sample_alone(mm, ref_fixture):
    plain = ref_fixture.with_(arith=mm.ARITH_STRICT)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, 2.0, INF))
    S, R = 5, 3
    theta = np.column_stack([mm.draws.jitter_draws(plain, 11, S), np.full(S, 4.0)])
    hip = mm.HipObjective(pb)
    theta[2, -1] = np.nan
    got = _score(hip, theta, R, hip.CONTEXT_DISPERSION)
    assert got["status"].tolist() == [0, 0, 1, 0, 0] and got["n_valid"] == 4 and np.isnan(got["k_used"][2, 0])
    _check_against_twin(mm, got, R)
    pooled = got["draws"][[0, 1, 3, 4]].reshape(12, 3, -1, pb.n)
    assert np.array_equal(got["mean"], pooled.sum(axis=0) / 12.0)
    # every sample failed: m = 0, every field NaN, counts 0
    theta[:, -1] = np.nan
    none = _score(hip, theta, R, hip.CONTEXT_DISPERSION)
    assert none["n_valid"] == 0 and np.isnan(none["cell_scores"]).all() and np.isnan(none["pit"]).all()
    assert (none["summary_count"] == 0).all() and np.isnan(none["summary"][..., 1:]).all()


def test_observed_override(mm, ref_fixture):
    S, R = 37, 7
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, S)
    base = _score(hip, theta, R)
    obs = mm.hostabi.observed_table(ref_fixture)
    Tp, n, L = obs.shape[1], obs.shape[2], len(LEVELS)
    other = np.where(np.isfinite(obs), obs + 1.5, 2.25)  # non-integer values
    other[1] = np.nan                                     # a series that is all NaN
    other[0, 3, 1] = np.nan
    other[2, 5, 2] = -1.0
    got = _score(hip, theta, R, observed=other)
    _check_against_twin(mm, got, R)
    assert np.array_equal(got["observed"], other, equal_nan=True)
    own = [0, 1, 2] + [5 + 4 * lv + f for lv in range(L) for f in (0, 1)]
    assert np.array_equal(got["cell_scores"][..., own], base["cell_scores"][..., own])
    for key in ("pred", "draws", "means", "status", "k_used"):
        assert np.array_equal(got[key], base[key], equal_nan=True), key
    usable = np.isfinite(other) & (other >= 0)
    assert np.isnan(got["crps"][~usable]).all() and np.isnan(got["pit"][~usable]).all() and np.isfinite(got["wis"][usable]).all()
    assert (got["summary_count"][1] == 0).all() and np.isnan(got["summary"][1, :, 1:]).all()
    assert got["summary_count"][0, 1] == Tp - 1 and got["summary_count"][2, n] == Tp * n - 1
    # a held-out window: NaN outside days 20 to 29
    window = np.full_like(obs, np.nan)
    window[:, 20:30] = other[:, 20:30]
    held = _score(hip, theta, R, observed=window)
    _check_against_twin(mm, held, R)
    assert np.array_equal(held["cell_scores"][:, 20:30], got["cell_scores"][:, 20:30], equal_nan=True)
    assert held["summary_count"][0, n] == 10 * n and held["summary_count"][1, n] == 0


@pytest.mark.parametrize("levels", [[], [0.1, 0.2, 0.3, 0.5, 0.8, 0.9, 0.95, 0.99]])
def test_no_level_and_eight_levels(mm, ref_fixture, levels):
    S, R = 37, 7
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, S)
    got = _score(hip, theta, R, levels=levels)
    assert got["cell_scores"].shape[-1] == 5 + 4 * len(levels) and got["summary"].shape[-1] == 4 + 2 * len(levels)
    _check_against_twin(mm, got, R, levels=levels)
    if not levels:  # the WIS of no interval is the absolute error of the median
        usable = np.isfinite(got["wis"])
        assert np.array_equal(got["wis"][usable], np.abs(got["observed"] - got["median"])[usable])


def test_the_context_is_left_unchanged(mm, shipped):
    S = 9
    pb = with_dispersion(shipped.with_(arith=mm.ARITH_STRICT), ("dispersion_H",), fixed=(INF, 6.0, INF))
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    theta = np.column_stack([mm.draws.jitter_draws(shipped, 11, S), np.linspace(0.5, 50.0, S)])
    q0 = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    p0 = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_means=True, want_draws=True, dispersion=hip.CONTEXT_DISPERSION)
    got = _score(hip, theta, 2, hip.CONTEXT_DISPERSION)
    for key in NB_KEYS:
        assert np.array_equal(got[key], p0[key], equal_nan=True), key
    _check_against_twin(mm, got, 2)
    assert np.isnan(hip.get_dispersion()[0]) and hip.get_dispersion()[1:].tolist() == [6.0, INF]
    q1 = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    p1 = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_means=True, want_draws=True, dispersion=hip.CONTEXT_DISPERSION)
    for key in ("ppc", "sero", "rt", "status"):
        assert np.array_equal(q0[key], q1[key], equal_nan=True)
    for key in NB_KEYS:
        assert np.array_equal(p0[key], p1[key], equal_nan=True), key
    # the last call's phases are reported
    assert got["phase_ms"].shape == (3,) and (got["phase_ms"] > 0).all()


def test_cpp_adapter_scores_through_the_device_call(mm, ref_fixture):
    """HipPosteriorPredictive::score on a dispersed objective (a calibrated dispersion_H and fixed values for the others) equals the
    context driven directly; on an undispersed one the draws are the Poisson call's."""
    plain = ref_fixture.with_(arith=mm.ARITH_STRICT, constraint_mode=mm.CONSTRAINT_CLAMP)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, INF, 3.0))
    S, R = 7, 5
    theta = np.column_stack([mm.draws.jitter_draws(plain, 11, S), np.linspace(0.2, 150.0, S)])
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    direct = _score(hip, theta, R, hip.CONTEXT_DISPERSION)
    host = mm.HostObjective(pb)
    got = host.posterior_predictive_scores(theta, 0, 0, R, SEED, PROBS, LEVELS, want_means=True, want_draws=True)
    assert got["samples_used"] == direct["n_valid"] and got["exact"] is True
    for key in TWIN_KEYS + ("means", "status", "k_used"):
        assert np.array_equal(got[key], direct[key], equal_nan=True), key
    # an observed table of the caller's own
    other = mm.hostabi.observed_table(pb) + 0.5
    got2 = host.posterior_predictive_scores(theta, 0, 0, R, SEED, PROBS, LEVELS, observed=other)
    direct2 = _score(hip, theta, R, hip.CONTEXT_DISPERSION, observed=other)
    for key in ("cell_scores", "summary", "pit", "pred"):
        assert np.array_equal(got2[key], direct2[key], equal_nan=True), key
    # an undispersed objective: Poisson draws, k_used +inf
    host0 = mm.HostObjective(plain)
    p0 = host0.posterior_predictive_scores(theta[:, :-1], 0, 0, R, SEED, PROBS, LEVELS, want_draws=True)
    hip0 = mm.HipObjective(plain)
    hip0.set_initial_state_mode(1)
    d0 = hip0.ensemble_predictive(theta[:, :-1], R, SEED, PROBS, want_draws=True)
    assert np.isposinf(p0["k_used"]).all()
    assert np.array_equal(p0["draws"], d0["draws"], equal_nan=True) and np.array_equal(p0["pred"], d0["pred"], equal_nan=True)
    assert np.array_equal(p0["pit"], d0["pit"], equal_nan=True)


def test_refused_arguments_on_the_device(mm, ref_fixture):
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 3)
    for bad in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"levels\[2\]"):
            _score(hip, theta, 2, levels=[0.5, 0.9, bad])
    with pytest.raises(ValueError, match="n_levels"):
        _score(hip, theta, 2, levels=np.linspace(0.1, 0.9, 9))
    # the C entry point itself refuses them with the same message
    lv = np.array([0.5, 1.0])
    th, pr = np.ascontiguousarray(theta), np.array(PROBS)
    Tp, n = len(ref_fixture.times), ref_fixture.n
    buf = [np.empty(k) for k in (6 * len(PROBS) * Tp * n, 3 * Tp * n, 3 * Tp * n * 13, 3 * (n + 1) * 8)]
    rc = hip.lib.sepaihrd_ensemble_predictive_scores(hip.ctx, th.ctypes.data, 3, 2, SEED, None, None, pr.ctypes.data, pr.size, lv.ctypes.data, 2,
                                                     buf[0].ctypes.data, buf[1].ctypes.data, buf[2].ctypes.data, buf[3].ctypes.data, None, None,
                                                     None, None, None, None)
    assert rc == -1 and "levels[1]" in hip.lib.sepaihrd_last_error(hip.ctx).decode()
    for shape in ((3, Tp, n + 1), (2, Tp, n)):
        with pytest.raises(ValueError, match="observed must be"):
            _score(hip, theta, 2, observed=np.zeros(shape))
    # the refusals of sepaihrd_ensemble_predictive_nb come through unchanged
    for bad, word in ((0.0, "is not positive"), (1e-4, "1e-3"), (float("nan"), "NaN")):
        with pytest.raises(ValueError) as e:
            _score(hip, theta, 2, (5.0, bad, INF))
        with pytest.raises(ValueError) as e2:
            mm.hostabi.particle_nb_validate((5.0, bad, INF))
        assert word in str(e.value) and str(e.value) == str(e2.value), (str(e.value), str(e2.value))
    with pytest.raises(ValueError, match="three entries"):
        _score(hip, theta, 2, (5.0, 5.0))
    for R, probs, word in ((0, PROBS, "R must be >= 1"), (-1, PROBS, "R must be >= 1"), (2, [0.5, 1.5], "probabilities")):
        with pytest.raises(RuntimeError) as e:
            _score(hip, theta, R, probs=probs)
        assert word in str(e.value), str(e.value)
    assert hip.lib.sepaihrd_eval_batch_begin(hip.ctx, th.ctypes.data, 3) == 0
    with pytest.raises(RuntimeError, match="sepaihrd_eval_batch_begin is pending"):
        _score(hip, theta, 2)
    ll = np.empty(3)
    assert hip.lib.sepaihrd_eval_batch_end(hip.ctx, ll.ctypes.data, None, None, None, None) == 0
    assert _score(hip, theta, 2)["n_valid"] >= 0
