"""Scores of the posterior predictive draws on window and age-group totals on the device (sepaihrd_ensemble_predictive_targets;
DESIGN.md section 6r) against the host twin, bit for bit -- the twin is fed the device's own means, status and k_used and the
table the observed targets are summed from -- and against the scored call on the same inputs.  The shapes are those of
tests/test_gpu_predictive_scores.py: one draw in a pad of 64, exactly one wavefront, a padded segment across a 256-lane
workgroup, the run-up offset, sixteen ages, the longest LDS sort and the radix route."""
import numpy as np
import pytest

from nb_objective_cases import with_dispersion

pytestmark = pytest.mark.gpu

INF = float("inf")
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
LEVELS = [0.5, 0.9, 0.95]
SEED = 0x1234_5678_9ABC_DEF0  # both words of the key in use
MIXED = (0.5, 10.0, INF)      # the boost branch, Cheng's branch and a Poisson series in one launch
GROUPS = (0, 0, 1, -1)        # on the 30-day fixture with w = 7, o = 1: 4 windows, row 0 and row 29 in none
TWIN_KEYS = ("target_quantiles", "pit", "target_obs", "target_scores", "summary", "target_draws", "draws")
SHARED_KEYS = ("means", "draws", "k_used", "status")


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


def _targets(hip, theta, R, groups=GROUPS, window=7, origin=1, dispersion=MIXED, observed=None, levels=LEVELS, seed=SEED, probs=PROBS,
             want=True):
    return hip.ensemble_predictive_targets(theta, R, seed, probs, levels, groups, window, origin, observed=observed, dispersion=dispersion,
                                           want_means=True, want_draws=want, want_target_draws=want)


def _check_against_twin(mm, got, pb, R, observed=None, levels=LEVELS, seed=SEED, probs=PROBS):
    obs = mm.hostabi.observed_table(pb) if observed is None else observed
    twin = mm.hostabi.predictive_targets_from_means(got["means"], got["status"], obs, R, seed, probs, levels, got["age_group"], got["window"],
                                                    got["origin"], k_used=got["k_used"])
    assert got["n_valid"] == twin["n_valid"] == int(np.sum(got["status"] == 0))
    assert got["exact"] is True and twin["exact"] is True
    assert (got["W"], got["G"]) == (twin["W"], twin["G"])
    for key in TWIN_KEYS:
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    return twin


def _sums_of(draws, groups, window, origin, W):
    """[S][R][3][W][G] window totals of the daily draws [S][R][3][T_pos][n] in numpy"""
    groups = np.asarray(groups)
    G = groups.max() + 1
    out = np.zeros(draws.shape[:3] + (W, G))
    for v in range(W):
        rows = draws[:, :, :, origin + v * window:origin + (v + 1) * window, :]
        for g in range(G):
            out[..., v, g] = rows[..., groups == g].sum(axis=(3, 4))
    return out


@pytest.mark.parametrize("S,R", [(1, 1), (1, 64), (37, 7)])
def test_device_equals_twin_on_the_reference_fixture(mm, ref_fixture, S, R):
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, S)
    got = _targets(hip, theta, R)
    L = len(LEVELS)
    assert (got["W"], got["G"]) == (4, 2) and got["window_first_row"].tolist() == [1, 8, 15, 22] and got["n_valid"] > 0
    assert got["target_scores"].shape == (6, 4, 2, 5 + 4 * L) and got["summary"].shape == (6, 3, 4 + 2 * L)
    assert got["target_quantiles"].shape == (6, len(PROBS), 4, 2) and got["target_draws"].shape == (S, R, 3, 4, 2)
    _check_against_twin(mm, got, ref_fixture, R)
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["median"]).all()
    # the optional outputs left out: the same targets (the draw kernel then launches the grouped ages alone)
    lean = hip.ensemble_predictive_targets(theta, R, SEED, PROBS, LEVELS, GROUPS, 7, 1, dispersion=MIXED)
    for key in ("target_quantiles", "pit", "target_obs", "target_scores", "summary", "k_used", "status"):
        assert np.array_equal(got[key], lean[key], equal_nan=True), key


@pytest.mark.parametrize("name,S,R,fma,groups", [("shipped", 5, 3, False, (0, 0, 0, 0)), ("shipped", 5, 3, True, (0, 0, 0, 0)),
                                                 ("wide", 5, 64, False, (1, 0, 2, 2, 2, 1, 1, 2, 2, 1, 2, 2, 2, 1, 2, 2))])
def test_device_equals_twin_on_other_problems(mm, shipped, ref_fixture, name, S, R, fma, groups):
    pb, mode = _problem(mm, name, shipped, ref_fixture)
    hip = _objective(mm, pb, mode, mm.ARITH_FMA if fma else mm.ARITH_STRICT)
    theta = mm.draws.jitter_draws(pb, 11, S)
    got = _targets(hip, theta, R, groups=groups, origin=0)
    Tp = int(np.sum(np.asarray(pb.times) >= 0))
    assert got["W"] == Tp // 7 and got["G"] == max(groups) + 1
    if name == "wide":
        assert sorted(np.bincount(np.asarray(groups)).tolist()) == [1, 5, 10]
    _check_against_twin(mm, got, pb, R)


def test_against_the_scored_call(mm, ref_fixture):
    S, R = 37, 7
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, S)
    sc = hip.ensemble_predictive_scores(theta, R, SEED, PROBS, LEVELS, dispersion=MIXED, want_means=True, want_draws=True)
    got = _targets(hip, theta, R)
    for key in SHARED_KEYS:
        assert np.array_equal(got[key], sc[key], equal_nan=True), key
    assert got["n_valid"] == sc["n_valid"]
    assert np.array_equal(got["target_draws"], _sums_of(sc["draws"], GROUPS, 7, 1, 4))
    # the identity grouping: every target is a daily cell
    ident = _targets(hip, theta, R, groups=(0, 1, 2, 3), window=1, origin=0)
    assert np.array_equal(ident["target_quantiles"], sc["pred"])
    assert np.array_equal(ident["target_scores"][:3], sc["cell_scores"], equal_nan=True)
    assert np.array_equal(ident["summary"][:3], sc["summary"], equal_nan=True)
    assert np.array_equal(ident["pit"][:3], sc["pit"], equal_nan=True)
    assert np.array_equal(ident["target_obs"][:3], sc["observed"], equal_nan=True)
    assert np.array_equal(ident["target_draws"], sc["draws"])
    # every series at +inf: the Poisson call's pred and pit
    plain = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True, want_draws=True)
    inf = _targets(hip, theta, R, groups=(0, 1, 2, 3), window=1, origin=0, dispersion=(INF, INF, INF))
    assert np.array_equal(inf["target_quantiles"], plain["pred"]) and np.array_equal(inf["pit"][:3], plain["pit"], equal_nan=True)
    assert np.array_equal(inf["draws"], plain["draws"]) and np.array_equal(inf["means"], plain["means"])


def test_both_sort_routes(mm, ref_fixture):
    """R = 128: S = 128 gives 16384 draws per segment, the longest the LDS sort takes (the raised dynamic-LDS limit); S = 129 gives
    16512, sorted by the segmented radix sort and scored over its scratch.  One group and w = 7: 6 x 4 segments."""
    R = 128
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 129)
    lds = _targets(hip, theta[:128], R, groups=(0, 0, 0, 0))
    _check_against_twin(mm, lds, ref_fixture, R)
    glob = _targets(hip, theta, R, groups=(0, 0, 0, 0))
    _check_against_twin(mm, glob, ref_fixture, R)
    assert lds["n_valid"] == 128 and glob["n_valid"] == 129 and (lds["W"], lds["G"]) == (4, 1)
    assert np.array_equal(glob["target_draws"][:128], lds["target_draws"])


def test_failed_samples_are_left_out(mm, oracle_py, shipped):
    """The attempt budget as tests/test_gpu_predictive_scores.py sets it: m = n_valid R, the failed samples' draws NaN, and a
    target's value independent of S, of R and of which other samples failed."""
    S, R = 50, 2
    theta = oracle_py.Oracle(shipped).jitter_draws(shipped.base_theta, 11, S, mode=1)
    probe = _objective(mm, shipped, 1)
    r = probe.eval_batch(theta)
    budget = int(np.sort(r["n_accept"] + r["n_reject"])[S // 2])
    hip = _objective(mm, shipped.with_(max_attempts=budget), 1)
    got = _targets(hip, theta, R, groups=(0, 0, 1, 1), origin=0)
    failed = got["status"] != 0
    assert 0 < got["n_valid"] < S and np.isnan(got["target_draws"][failed]).all() and np.isnan(got["draws"][failed]).all()
    _check_against_twin(mm, got, shipped, R)
    keep = np.flatnonzero(~failed)
    m = got["n_valid"] * R
    pooled = got["target_draws"][keep].reshape(m, 3, got["W"], 2)
    for k, v, g in ((0, 3, 1), (1, 20, 0), (2, 40, 1)):
        one = mm.hostabi.score_cell(pooled[:, k, v, g], got["target_obs"][k, v, g], LEVELS)
        assert np.array_equal(one["scores"], got["target_scores"][k, v, g], equal_nan=True)
        cum = mm.hostabi.score_cell(pooled[:, k, :v + 1, g].sum(axis=1), got["target_obs"][k + 3, v, g], LEVELS)
        assert np.array_equal(cum["scores"], got["target_scores"][k + 3, v, g], equal_nan=True)
    # the first valid sample alone, with one replicate more, under the unbudgeted context: the same values at (s, r)
    s0 = int(keep[0])
    alone = _targets(probe, theta[:s0 + 1], R + 1, groups=(0, 0, 1, 1), origin=0)
    assert alone["status"][s0] == 0
    assert np.array_equal(alone["target_draws"][s0, :R], got["target_draws"][s0])


def test_a_nan_dispersion_entry_fails_its_sample_alone(mm, ref_fixture):
    plain = ref_fixture.with_(arith=mm.ARITH_STRICT)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, 2.0, INF))
    S, R = 5, 3
    theta = np.column_stack([mm.draws.jitter_draws(plain, 11, S), np.full(S, 4.0)])
    hip = mm.HipObjective(pb)
    theta[2, -1] = np.nan
    got = _targets(hip, theta, R, dispersion=hip.CONTEXT_DISPERSION)
    assert got["status"].tolist() == [0, 0, 1, 0, 0] and got["n_valid"] == 4 and np.isnan(got["k_used"][2, 0])
    _check_against_twin(mm, got, pb, R)
    pooled = got["target_draws"][[0, 1, 3, 4]].reshape(12, 3, 4, 2)
    assert np.array_equal(got["mean"][:3], pooled.sum(axis=0) / 12.0)
    # every sample failed: m = 0, every field NaN, counts 0
    theta[:, -1] = np.nan
    none = _targets(hip, theta, R, dispersion=hip.CONTEXT_DISPERSION)
    assert none["n_valid"] == 0 and np.isnan(none["target_scores"]).all() and np.isnan(none["pit"]).all()
    assert np.isnan(none["target_quantiles"]).all() and np.isnan(none["target_draws"]).all()
    assert (none["summary_count"] == 0).all() and np.isnan(none["summary"][..., 1:]).all()


def test_observed_override(mm, ref_fixture):
    S, R = 37, 7
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, S)
    base = _targets(hip, theta, R)
    obs = mm.hostabi.observed_table(ref_fixture)
    L = len(LEVELS)
    other = np.where(np.isfinite(obs), obs + 1.5, 2.25)  # non-integer values
    other[1] = np.nan                                     # a series that is all NaN
    other[0, 10, 1] = np.nan                              # inside window 1 of group 0
    other[2, 16, 3] = np.nan                              # an age outside every group: no target sees it
    got = _targets(hip, theta, R, observed=other)
    _check_against_twin(mm, got, ref_fixture, R, observed=other)
    own = [0, 1, 2] + [5 + 4 * lv + f for lv in range(L) for f in (0, 1)]
    assert np.array_equal(got["target_scores"][..., own], base["target_scores"][..., own])
    for key in ("target_quantiles", "target_draws", "draws", "means", "status", "k_used"):
        assert np.array_equal(got[key], base[key], equal_nan=True), key
    tobs = got["target_obs"]
    assert np.isnan(tobs[[1, 4]]).all() and np.isfinite(tobs[[2, 5]]).all()
    assert np.isnan(tobs[0, 1, 0]) and np.isnan(tobs[3, 1:, 0]).all() and np.isfinite(tobs[3, 0, 0]) and np.isfinite(tobs[[0, 3]][:, :, 1]).all()
    assert np.isfinite(tobs[0, [0, 2, 3], 0]).all()
    usable = np.isfinite(tobs)
    assert np.isnan(got["crps"][~usable]).all() and np.isnan(got["pit"][~usable]).all() and np.isfinite(got["wis"][usable]).all()
    assert got["summary_count"][:, 2].tolist() == [7, 0, 8, 5, 0, 8]
    # a held-out tail: NaN from row 15 on leaves windows 0 and 1
    tail = other.copy()
    tail[1] = np.where(np.isfinite(obs[1]), obs[1] + 0.25, 1.0)
    tail[:, 15:] = np.nan
    held = _targets(hip, theta, R, observed=tail)
    _check_against_twin(mm, held, ref_fixture, R, observed=tail)
    assert np.isnan(held["target_obs"][:, 2:]).all() and np.isfinite(held["target_obs"][1, :2]).all()
    assert held["summary_count"][1].tolist() == [2, 2, 4] and held["summary_count"][4].tolist() == [2, 2, 4]
    assert np.array_equal(held["target_scores"][2, :2], got["target_scores"][2, :2])


@pytest.mark.parametrize("levels", [[], [0.1, 0.2, 0.3, 0.5, 0.8, 0.9, 0.95, 0.99]])
def test_no_level_and_eight_levels(mm, ref_fixture, levels):
    S, R = 37, 7
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, S)
    got = _targets(hip, theta, R, levels=levels)
    assert got["target_scores"].shape[-1] == 5 + 4 * len(levels) and got["summary"].shape[-1] == 4 + 2 * len(levels)
    _check_against_twin(mm, got, ref_fixture, R, levels=levels)
    if not levels:  # the WIS of no interval is the absolute error of the median
        usable = np.isfinite(got["wis"])
        assert np.array_equal(got["wis"][usable], np.abs(got["target_obs"] - got["median"])[usable])


def test_the_context_is_left_unchanged(mm, shipped):
    S = 9
    pb = with_dispersion(shipped.with_(arith=mm.ARITH_STRICT), ("dispersion_H",), fixed=(INF, 6.0, INF))
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    theta = np.column_stack([mm.draws.jitter_draws(shipped, 11, S), np.linspace(0.5, 50.0, S)])
    q0 = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    p0 = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_means=True, want_draws=True, dispersion=hip.CONTEXT_DISPERSION)
    got = _targets(hip, theta, 2, groups=(0, 1, 1, -1), origin=3, dispersion=hip.CONTEXT_DISPERSION)
    for key in SHARED_KEYS:
        assert np.array_equal(got[key], p0[key], equal_nan=True), key
    _check_against_twin(mm, got, pb, 2)
    assert np.isnan(hip.get_dispersion()[0]) and hip.get_dispersion()[1:].tolist() == [6.0, INF]
    q1 = hip.ensemble_quantiles(theta, [0.0, 0.5, 1.0], want_sero=True, want_rt=True)
    p1 = hip.ensemble_predictive(theta, 2, SEED, PROBS, want_means=True, want_draws=True, dispersion=hip.CONTEXT_DISPERSION)
    for key in ("ppc", "sero", "rt", "status"):
        assert np.array_equal(q0[key], q1[key], equal_nan=True)
    for key in ("pred", "pit") + SHARED_KEYS:
        assert np.array_equal(p0[key], p1[key], equal_nan=True), key
    assert got["phase_ms"].shape == (3,) and (got["phase_ms"] > 0).all()


def test_cpp_adapter_scores_targets_through_the_device_call(mm, ref_fixture):
    """HipPosteriorPredictive::scoreTargets on a dispersed objective equals the context driven directly; on an undispersed one the
    draws are Poisson and k_used is +inf."""
    plain = ref_fixture.with_(arith=mm.ARITH_STRICT, constraint_mode=mm.CONSTRAINT_CLAMP)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, INF, 3.0))
    S, R = 7, 5
    theta = np.column_stack([mm.draws.jitter_draws(plain, 11, S), np.linspace(0.2, 150.0, S)])
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    direct = _targets(hip, theta, R, dispersion=hip.CONTEXT_DISPERSION)
    host = mm.HostObjective(pb)
    got = host.posterior_predictive_targets(theta, 0, 0, R, SEED, PROBS, LEVELS, GROUPS, 7, 1, want_target_draws=True)
    assert got["samples_used"] == direct["n_valid"] and got["exact"] is True and (got["W"], got["G"]) == (4, 2)
    for key in ("target_quantiles", "pit", "target_obs", "target_scores", "summary", "target_draws", "status", "k_used"):
        assert np.array_equal(got[key], direct[key], equal_nan=True), key
    other = mm.hostabi.observed_table(pb) + 0.5
    got2 = host.posterior_predictive_targets(theta, 0, 0, R, SEED, PROBS, LEVELS, GROUPS, 7, 1, observed=other)
    direct2 = _targets(hip, theta, R, dispersion=hip.CONTEXT_DISPERSION, observed=other)
    for key in ("target_quantiles", "pit", "target_obs", "target_scores", "summary"):
        assert np.array_equal(got2[key], direct2[key], equal_nan=True), key
    host0 = mm.HostObjective(plain)
    p0 = host0.posterior_predictive_targets(theta[:, :-1], 0, 0, R, SEED, PROBS, LEVELS, GROUPS, 7, 1)
    hip0 = mm.HipObjective(plain)
    hip0.set_initial_state_mode(1)
    d0 = _targets(hip0, theta[:, :-1], R, dispersion=(INF, INF, INF))
    assert np.isposinf(p0["k_used"]).all()
    for key in ("target_quantiles", "pit", "target_scores", "summary"):
        assert np.array_equal(p0[key], d0[key], equal_nan=True), key
    with pytest.raises(ValueError, match="gap"):
        host.posterior_predictive_targets(theta, 0, 0, R, SEED, PROBS, LEVELS, (0, 2, 2, -1), 7, 1)


def test_refused_arguments_on_the_device(mm, ref_fixture):
    hip = _objective(mm, ref_fixture, 0)
    theta = mm.draws.jitter_draws(ref_fixture, 11, 3)
    for groups, window, origin, word in (((0, 0, 4, -1), 7, 1, r"age_group\[2\] = 4"), ((0, -2, 1, -1), 7, 1, r"age_group\[1\] = -2"),
                                         ((0, 2, 2, -1), 7, 1, "no age has group id 1"), ((-1, -1, -1, -1), 7, 1, "no age in any group"),
                                         (GROUPS, 0, 1, "window must be >= 1"), (GROUPS, 7, -1, "origin must be >= 0"),
                                         (GROUPS, 31, 0, r"W < 1"), (GROUPS, 7, 24, r"W < 1"), (GROUPS, 1, 30, r"W < 1")):
        with pytest.raises(ValueError, match=word):
            _targets(hip, theta, 2, groups=groups, window=window, origin=origin)
    with pytest.raises(ValueError, match="age_group must hold"):
        _targets(hip, theta, 2, groups=(0, 0, 1))
    # the C entry point itself refuses them with the same message, and a NULL age_group
    th, pr, lv = np.ascontiguousarray(theta), np.array(PROBS), np.array(LEVELS)
    buf = [np.empty(k) for k in (6 * len(PROBS) * 8, 6 * 8, 6 * 8 * 17, 6 * 3 * 10)]

    def call(ag, window, origin):
        return hip.lib.sepaihrd_ensemble_predictive_targets(
            hip.ctx, th.ctypes.data, 3, 2, SEED, None, None, None if ag is None else ag.ctypes.data, window, origin, pr.ctypes.data, pr.size,
            lv.ctypes.data, lv.size, buf[0].ctypes.data, buf[1].ctypes.data, buf[2].ctypes.data, buf[3].ctypes.data, None, None, None, None, None,
            None, None, None)
    assert call(None, 7, 1) == -1 and "age_group must not be NULL" in hip.lib.sepaihrd_last_error(hip.ctx).decode()
    assert call(np.array([0, 2, 2, -1], dtype=np.int32), 7, 1) == -1 and "gap" in hip.lib.sepaihrd_last_error(hip.ctx).decode()
    assert call(np.array(GROUPS, dtype=np.int32), 7, 1) == 0
    # the scored call's refusals come through unchanged
    for bad in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"levels\[2\]"):
            _targets(hip, theta, 2, levels=[0.5, 0.9, bad])
    for shape in ((3, 30, 5), (2, 30, 4)):
        with pytest.raises(ValueError, match="observed must be"):
            _targets(hip, theta, 2, observed=np.zeros(shape))
    for bad, word in ((0.0, "is not positive"), (1e-4, "1e-3"), (float("nan"), "NaN")):
        with pytest.raises(ValueError) as e:
            _targets(hip, theta, 2, dispersion=(5.0, bad, INF))
        assert word in str(e.value), str(e.value)
    for R, probs, word in ((0, PROBS, "R must be >= 1"), (2, [0.5, 1.5], "probabilities")):
        with pytest.raises(RuntimeError) as e:
            _targets(hip, theta, R, probs=probs)
        assert word in str(e.value), str(e.value)
    assert hip.lib.sepaihrd_eval_batch_begin(hip.ctx, th.ctypes.data, 3) == 0
    with pytest.raises(RuntimeError, match="sepaihrd_eval_batch_begin is pending"):
        _targets(hip, theta, 2)
    ll = np.empty(3)
    assert hip.lib.sepaihrd_eval_batch_end(hip.ctx, ll.ctypes.data, None, None, None, None) == 0
    assert _targets(hip, theta, 2)["n_valid"] >= 0
