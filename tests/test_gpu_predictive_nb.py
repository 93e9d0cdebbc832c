"""Posterior predictive draws under the negative-binomial observation model on the device (sepaihrd_ensemble_predictive_nb,
sepaihrd_gamma_device, sepaihrd_nb_draw_device) against the host twin, bit for bit: the twin is fed the
device's own means, status and k_used and the problem's observations.  With every series at +inf the call is
sepaihrd_ensemble_predictive in another lane mapping: the same bits."""
import numpy as np
import pytest

from nb_objective_cases import with_dispersion

pytestmark = pytest.mark.gpu

INF = float("inf")
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
SEED = 0x1234_5678_9ABC_DEF0  # both words of the key in use
MIXED = (0.5, 10.0, INF)      # the boost branch, Cheng's branch and a Poisson series in one launch
KEYS = ("draws", "pred", "pit")


def _problem(mm, name, shipped, ref_fixture):
    if name == "ref":      # n = 4, 30 times, no run-up
        return ref_fixture, 0
    if name == "shipped":  # n = 4, 326 times, run-up offset 20
        return shipped, 1
    wide = mm.problem.widen_age_classes(shipped, 4)  # n = 16: sixteen blocks along the grid's y dimension
    return mm.workloads.with_synthetic_observations(wide, lambda p: mm.HipObjective(p)), 1


def _objective(mm, pb, mode, arith=None):
    hip = mm.HipObjective(pb.with_(arith=mm.ARITH_STRICT if arith is None else arith))
    hip.set_initial_state_mode(mode)
    return hip


def _draw(hip, theta, R, dispersion, seed=SEED, probs=PROBS):
    return hip.ensemble_predictive(theta, R, seed, probs, want_means=True, want_draws=True, dispersion=dispersion)


def _check_against_twin(mm, pb, got, R, seed=SEED, probs=PROBS):
    twin = mm.hostabi.predictive_from_means(got["means"], got["status"], mm.hostabi.observed_table(pb), R, seed, probs, k_used=got["k_used"])
    assert got["n_valid"] == twin["n_valid"] == int(np.sum(got["status"] == 0))
    for key in KEYS:
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    return twin


def _same(a, b, keys=KEYS + ("means", "status")):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["n_valid"] == b["n_valid"]


@pytest.mark.parametrize("name,S,R,fma", [("ref", 1, 64, False), ("ref", 37, 7, False), ("shipped", 5, 3, False), ("shipped", 5, 3, True),
                                          ("wide", 5, 64, False)])
def test_device_equals_twin_with_mixed_dispersions(mm, shipped, ref_fixture, name, S, R, fma):
    pb, mode = _problem(mm, name, shipped, ref_fixture)
    hip = _objective(mm, pb, mode, mm.ARITH_FMA if fma else mm.ARITH_STRICT)
    theta = mm.draws.jitter_draws(pb, 11, S)
    got = _draw(hip, theta, R, MIXED)
    Tp = int(np.sum(np.asarray(pb.times) >= 0))
    assert got["draws"].shape == (S, R, 3, Tp, pb.n) and got["n_valid"] > 0
    assert np.array_equal(got["k_used"], np.tile(MIXED, (S, 1)))
    _check_against_twin(mm, pb, got, R)
    valid = got["status"] == 0
    d = got["draws"][valid]
    assert np.isfinite(d).all() and (d >= 0).all() and np.array_equal(d, np.floor(d))
    # the series left at +inf has the Poisson call's draws and quantiles (daily and cumulative), the dispersed ones have not
    plain = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True)
    assert np.array_equal(got["means"], plain["means"], equal_nan=True) and np.array_equal(got["status"], plain["status"])
    assert np.array_equal(got["draws"][:, :, 2], plain["draws"][:, :, 2], equal_nan=True)
    assert np.array_equal(got["pred"][[2, 5]], plain["pred"][[2, 5]], equal_nan=True)
    assert np.array_equal(got["pit"][2], plain["pit"][2], equal_nan=True)
    assert not np.array_equal(got["draws"][:, :, 0], plain["draws"][:, :, 0], equal_nan=True)
    assert not np.array_equal(got["draws"][:, :, 1], plain["draws"][:, :, 1], equal_nan=True)


@pytest.mark.parametrize("name,S,R", [("ref", 37, 7), ("shipped", 5, 3)])
def test_calibrated_dispersion_is_resolved_per_sample(mm, shipped, ref_fixture, name, S, R):
    """theta calibrates dispersion_H with a distinct value per sample (some outside the bounds: the constraint rule acts), the
    other two series have fixed values.  NULL takes what eval_batch's likelihood would: k_used is apply_constraints of theta."""
    plain, mode = _problem(mm, name, shipped, ref_fixture)
    plain = plain.with_(arith=mm.ARITH_STRICT)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, INF, 3.0))
    k_H = np.exp(np.linspace(np.log(0.06), np.log(190.0), S))
    k_H[-1] = 1234.5   # beyond the upper bound of 200
    if S > 2:
        k_H[1] = -0.3  # below the lower bound of 0.05
    theta = np.column_stack([mm.draws.jitter_draws(plain, 11, S), k_H])
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(mode)
    assert np.isnan(hip.get_dispersion()[0]) and hip.get_dispersion()[1:].tolist() == [INF, 3.0]
    got = _draw(hip, theta, R, hip.CONTEXT_DISPERSION)
    want_k = hip.apply_constraints(theta, pb.constraint_mode)[:, -1]
    assert np.array_equal(got["k_used"][:, 0], want_k) and len(set(want_k.tolist())) == S
    assert (want_k >= 0.05).all() and (want_k <= 200.0).all() and want_k[-1] != k_H[-1]
    assert np.array_equal(got["k_used"][:, 1:], np.tile([INF, 3.0], (S, 1)))
    _check_against_twin(mm, pb, got, R)
    # three values of the call's own override the context, whatever theta says; k_used says so
    over = _draw(hip, theta, R, (INF, 7.0, INF))
    assert np.array_equal(over["k_used"], np.tile([INF, 7.0, INF], (S, 1)))
    _check_against_twin(mm, pb, over, R)
    assert np.array_equal(over["means"], got["means"], equal_nan=True)
    assert not np.array_equal(over["draws"][:, :, 1], got["draws"][:, :, 1], equal_nan=True)


@pytest.mark.parametrize("name,S,R", [("shipped", 5, 3), ("shipped", 37, 7), ("wide", 5, 64)])
def test_all_series_at_infinity_is_the_poisson_call(mm, shipped, ref_fixture, name, S, R):
    """the wider mapping against the present one: every output has the bits of sepaihrd_ensemble_predictive"""
    pb, mode = _problem(mm, name, shipped, ref_fixture)
    hip = _objective(mm, pb, mode)
    theta = mm.draws.jitter_draws(pb, 11, S)
    plain = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True)
    for dispersion in ((INF, INF, INF), hip.CONTEXT_DISPERSION):  # the context's default is +inf throughout
        got = _draw(hip, theta, R, dispersion)
        _same(got, plain)
        assert np.isposinf(got["k_used"]).all() and got["k_used"].shape == (S, 3)


def test_both_sort_paths(mm, ref_fixture):
    """R = 128 as tests/test_gpu_predictive.py sizes it: S = 128 gives 16384 draws per segment, the longest the LDS sort takes;
    S = 129 gives 16512, sorted by the segmented radix sort."""
    R = 128
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 129)
    lds = _draw(hip, theta[:128], R, MIXED)
    _check_against_twin(mm, ref_fixture, lds, R)
    glob = _draw(hip, theta, R, MIXED)
    _check_against_twin(mm, ref_fixture, glob, R)
    assert lds["n_valid"] == 128 and glob["n_valid"] == 129
    assert np.array_equal(glob["draws"][:128], lds["draws"])


def test_draws_do_not_depend_on_the_call_around_them(mm, shipped):
    S = 12
    hip = _objective(mm, shipped, 1)
    theta = mm.draws.jitter_draws(shipped, 11, S)
    r4 = _draw(hip, theta, 4, MIXED)["draws"]
    assert np.array_equal(_draw(hip, theta, 2, MIXED)["draws"], r4[:, :2])
    assert np.array_equal(_draw(hip, theta[:5], 4, MIXED)["draws"], r4[:5])
    other = _draw(hip, theta, 4, MIXED, seed=SEED + 1)["draws"]
    assert np.mean(other != r4) > 0.05  # most cells of the shipped problem have small means: equal draws are common


def test_failed_samples_are_padded_and_skipped(mm, oracle_py, shipped):
    """The attempt budget as tests/test_gpu_predictive.py's test_failed_samples_are_padded_and_skipped sets it."""
    S, R = 50, 2
    theta = oracle_py.Oracle(shipped).jitter_draws(shipped.base_theta, 11, S, mode=1)
    probe = _objective(mm, shipped, 1)
    r = probe.eval_batch(theta)
    budget = int(np.sort(r["n_accept"] + r["n_reject"])[S // 2])
    hip = _objective(mm, shipped.with_(max_attempts=budget), 1)
    plain = hip.ensemble_quantiles(theta, PROBS)
    got = _draw(hip, theta, R, MIXED)
    assert 0 < got["n_valid"] < S and got["n_valid"] == plain["n_valid"] and np.array_equal(got["status"], plain["status"])
    failed = got["status"] != 0
    assert np.isnan(got["draws"][failed]).all() and np.isnan(got["means"][failed]).all() and np.isfinite(got["draws"][~failed]).all()
    _check_against_twin(mm, shipped, got, R)
    full = _draw(probe, theta, R, MIXED)
    assert np.array_equal(full["draws"][~failed], got["draws"][~failed])


def test_a_nan_dispersion_entry_fails_its_sample_alone(mm, ref_fixture):
    plain = ref_fixture.with_(arith=mm.ARITH_STRICT)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, 2.0, INF))
    S, R = 5, 3
    theta = np.column_stack([mm.draws.jitter_draws(plain, 11, S), np.full(S, 4.0)])
    hip = mm.HipObjective(pb)
    good = _draw(hip, theta, R, hip.CONTEXT_DISPERSION)
    theta[2, -1] = np.nan
    got = _draw(hip, theta, R, hip.CONTEXT_DISPERSION)
    assert got["status"].tolist() == [0, 0, 1, 0, 0] and got["n_valid"] == 4 and np.isnan(got["k_used"][2, 0])
    assert np.isnan(got["draws"][2]).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(got["draws"][keep], good["draws"][keep]) and np.isfinite(got["pred"]).all()
    _check_against_twin(mm, pb, got, R)


def test_the_context_is_left_unchanged(mm, shipped):
    S = 9
    pb = with_dispersion(shipped.with_(arith=mm.ARITH_STRICT), ("dispersion_H",), fixed=(INF, 6.0, INF))
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    theta = np.column_stack([mm.draws.jitter_draws(shipped, 11, S), np.linspace(0.5, 50.0, S)])
    q0 = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    e0 = hip.eval_batch(theta)
    p0 = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_means=True, want_draws=True)
    got = _draw(hip, theta, 2, hip.CONTEXT_DISPERSION)
    over = _draw(hip, theta, 2, (1.0, 1.0, 1.0))
    assert np.array_equal(over["k_used"], np.ones((S, 3))) and not np.array_equal(got["k_used"], over["k_used"])
    assert np.isnan(hip.get_dispersion()[0]) and hip.get_dispersion()[1:].tolist() == [6.0, INF]
    q1 = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    e1 = hip.eval_batch(theta)
    p1 = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_means=True, want_draws=True)
    for key in ("ppc", "sero", "rt", "status"):
        assert np.array_equal(q0[key], q1[key], equal_nan=True)
    for key in ("loglik", "ll_parts", "status"):
        assert np.array_equal(e0[key], e1[key])
    _same(p0, p1)
    # the Poisson call does not read the context's dispersion: the bits of an undispersed context
    ref = _objective(mm, shipped, 1).ensemble_predictive(theta[:, :-1], 2, SEED, PROBS, want_means=True, want_draws=True)
    _same(p0, ref)
    # the last call's phases are reported
    assert got["phase_ms"].shape == (3,) and (got["phase_ms"] > 0).all()


def test_probes_equal_the_host_sampler(mm, shipped):
    hip = mm.HipObjective(shipped)
    shapes = np.repeat(np.array([1e-3, 0.05, 0.5, 0.999, 1.0, 1.0001, 2.5, 10.0, 1e3, 1e6]), 512)
    g = hip.gamma_device(shapes, SEED)
    assert np.array_equal(g, mm.hostabi.gamma_probe(shapes, SEED)) and np.isfinite(g).all() and (g >= 0).all()
    assert not np.array_equal(g, hip.gamma_device(shapes, SEED + 1))
    ks = np.array([1e-3, 0.5, 1.0, 10.0, 100.0, 1e6, INF])
    mus = np.array([1e-10, 0.5, 3.0, 9.5, 30.0, 100.0, 1e3, 1e6, 0.0, -1.0, np.nan, np.inf])
    mu, k = np.repeat(np.tile(mus, len(ks)), 64), np.repeat(np.repeat(ks, len(mus)), 64)
    y = hip.nb_draw_device(mu, k, SEED)
    assert np.array_equal(y, mm.hostabi.nb_draw_probe(mu, k, SEED), equal_nan=True)
    assert np.array_equal(y[np.isposinf(k)], hip.poisson(mu, SEED)[np.isposinf(k)], equal_nan=True)
    for bad in (0.0, 1e-4, float("nan"), -1.0, 2e6):
        with pytest.raises(RuntimeError, match="finite in"):
            hip.nb_draw_device([3.0], [bad], SEED)
        with pytest.raises(RuntimeError, match="finite in"):
            hip.gamma_device([bad], SEED)
    with pytest.raises(RuntimeError, match="finite in"):
        hip.gamma_device([INF], SEED)


def test_refused_arguments_on_the_device(mm, ref_fixture):
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 3)
    for bad, word in ((0.0, "is not positive"), (1e-4, "1e-3"), (float("nan"), "NaN")):
        with pytest.raises(ValueError) as e:
            _draw(hip, theta, 2, (5.0, bad, INF))
        with pytest.raises(ValueError) as e2:
            mm.hostabi.particle_nb_validate((5.0, bad, INF))
        assert word in str(e.value) and str(e.value) == str(e2.value), (str(e.value), str(e2.value))
    with pytest.raises(ValueError, match="three entries"):
        _draw(hip, theta, 2, (5.0, 5.0))
    for R, probs, word in ((0, PROBS, "R must be >= 1"), (-1, PROBS, "R must be >= 1"), (2, [0.5, 1.5], "probabilities")):
        with pytest.raises(RuntimeError) as e:
            _draw(hip, theta, R, MIXED, probs=probs)
        assert word in str(e.value), str(e.value)
    th = np.ascontiguousarray(theta)
    assert hip.lib.sepaihrd_eval_batch_begin(hip.ctx, th.ctypes.data, 3) == 0
    with pytest.raises(RuntimeError, match="sepaihrd_eval_batch_begin is pending"):
        _draw(hip, theta, 2, MIXED)
    ll = np.empty(3)
    assert hip.lib.sepaihrd_eval_batch_end(hip.ctx, ll.ctypes.data, None, None, None, None) == 0
    assert _draw(hip, theta, 2, MIXED)["n_valid"] >= 0


def test_cpp_adapter_draws_through_the_dispersed_call(mm, ref_fixture):
    """HipPosteriorPredictive::draw on a dispersed objective (a calibrated dispersion_H and fixed values for the others) equals the
    context driven directly; on an undispersed one it stays the Poisson call."""
    plain = ref_fixture.with_(arith=mm.ARITH_STRICT, constraint_mode=mm.CONSTRAINT_CLAMP)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, INF, 3.0))
    S, R = 7, 5
    theta = np.column_stack([mm.draws.jitter_draws(plain, 11, S), np.linspace(0.2, 150.0, S)])
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    direct = _draw(hip, theta, R, hip.CONTEXT_DISPERSION)
    host = mm.HostObjective(pb)
    got = host.posterior_predictive(theta, 0, 0, R, SEED, PROBS, want_means=True, want_draws=True)
    assert got["dispersed"] and np.array_equal(got["k_used"], direct["k_used"]) and got["samples_used"] == direct["n_valid"]
    for key in KEYS + ("means", "status"):
        assert np.array_equal(got[key], direct[key], equal_nan=True), key
    host0 = mm.HostObjective(plain)
    p0 = host0.posterior_predictive(theta[:, :-1], 0, 0, R, SEED, PROBS, want_draws=True)
    hip0 = mm.HipObjective(plain)
    hip0.set_initial_state_mode(1)
    d0 = hip0.ensemble_predictive(theta[:, :-1], R, SEED, PROBS, want_draws=True)
    assert not p0["dispersed"] and np.isposinf(p0["k_used"]).all()
    assert np.array_equal(p0["draws"], d0["draws"], equal_nan=True) and np.array_equal(p0["pred"], d0["pred"], equal_nan=True)
    # a fixed dispersion set on the handle reaches the adapter's objective
    host0.set_dispersion((4.0, INF, 0.8))
    hip0.set_dispersion((4.0, INF, 0.8))
    p1 = host0.posterior_predictive(theta[:, :-1], 0, 0, R, SEED, PROBS, want_draws=True)
    d1 = _draw(hip0, theta[:, :-1], R, hip0.CONTEXT_DISPERSION)
    assert p1["dispersed"] and np.array_equal(p1["k_used"], np.tile([4.0, INF, 0.8], (S, 1)))
    assert np.array_equal(p1["draws"], d1["draws"], equal_nan=True) and np.array_equal(p1["pred"], d1["pred"], equal_nan=True)
