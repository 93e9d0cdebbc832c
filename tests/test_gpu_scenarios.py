"""NPI scenario analysis on the device (sepaihrd_scenario_ensemble): kappa counterfactuals over every posterior sample.

Reference behaviour: PostCalibrationAnalyser.cpp:94-141 (scenarios scale the constrained kappa_values[idx]),
:163-168 (the metrics read the template's unscaled NPI strategy), :378-401 (one run per scenario).
"""
import numpy as np
import pytest

PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]


def _draws(oracle_py, pb, S, seed0=11):
    return oracle_py.Oracle(pb).jitter_draws(pb.base_theta, seed0, S, mode=1)


def _hip(mm, pb):
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    return hip


def _mult(pb, rows):
    nk = len(pb.kappa_values)
    out = np.ones((len(rows), nk))
    for k, (i, f) in enumerate(rows):
        if i is not None:
            out[k, i] = f
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["strict", "fma"])
@pytest.mark.parametrize("solver", [0, 1, 2])
def test_identity_table_reproduces_ensemble_quantiles(mm, oracle_py, shipped, solver, arith):
    pb = shipped.with_(solver=solver, arith=mm.ARITH_STRICT if arith == "strict" else mm.ARITH_FMA)
    theta = _draws(oracle_py, pb, 37)
    ens = _hip(mm, pb).ensemble_quantiles(theta, PROBS, want_sero=True, want_rt=True, want_metrics=True)
    sc = _hip(mm, pb).scenario_ensemble(theta, np.ones((1, len(pb.kappa_values))), PROBS, want_sero=True, want_rt=True)
    assert np.array_equal(sc["status"][0], ens["status"]) and sc["n_valid"][0] == ens["n_valid"]
    for key in ("ppc", "sero", "rt"):
        assert np.array_equal(sc[key][0], ens[key]), key
    assert np.array_equal(sc["metrics"][0], ens["metrics"], equal_nan=True)


def _oracle_theta(hip, pb, theta, mult_row):
    """theta whose constrained kappa values are the scenario's scaled ones; None where the scaled value leaves the bounds."""
    c = hip.apply_constraints(theta, pb.constraint_mode)
    t = c.copy()
    codes, idxs = pb.field_map()
    for p, (code, i) in enumerate(zip(codes, idxs)):
        if pb.param_names[p].startswith("kappa_"):
            t[:, p] = c[:, p] * mult_row[i]
    keep = np.all(hip.apply_constraints(t, pb.constraint_mode) == t, axis=1)
    return t, keep


def _oracle_metrics(oracle_py, pb, theta, scaled):
    """MetricsCalculator::calculateEssentialMetrics restated in numpy (oracle/rt_numpy.py) on the oracle's trajectories of
    the scaled-kappa theta, with the UNSCALED parameters of theta: R0, Rt and the attack-rate accumulation read the
    template's kappa (PostCalibrationAnalyser.cpp:163-168), the run itself the scenario's."""
    import rt_numpy
    orc = oracle_py.Oracle(pb)
    sim = orc.simulate_samples(scaled)
    assert (sim["status"] == 0).all()
    return np.array([rt_numpy.essential_metrics(sim["traj"][s], orc.model_parameters(theta[s]), pb) for s in range(len(theta))])


def _oracle_rt_quantiles(oracle_py, pb, theta, scaled):
    import rt_numpy
    orc = oracle_py.Oracle(pb)
    sim = orc.simulate_samples(scaled)
    rts = np.array([rt_numpy.rt_trajectory(sim["traj"][s], orc.model_parameters(theta[s]), pb) for s in range(len(theta))])
    return np.array([[rt_numpy.sorted_quantile(rts[:, t], p) for t in range(rts.shape[1])] for p in PROBS])


@pytest.mark.gpu
@pytest.mark.parametrize("n_age", [4, 16])
def test_scenarios_match_oracle_with_scaled_kappa(mm, oracle_py, shipped, n_age):
    """Every scenario against the oracle: trajectories (PPC quantiles) of the run with kappa fixed at the constrained
    kappa_values x mult, and the per-sample metric table and the paired differences against the numpy metrics of those
    trajectories with the unscaled kappa."""
    pb = shipped if n_age == 4 else mm.widen_age_classes(shipped, 4)
    # a non-zero constant beta: the attack-rate accumulation multiplies kappa(t) by it (MetricsCalculator.cpp:103-113), so
    # with the shipped beta = 0 it could not tell the scaled kappa from the unscaled one
    pb = pb.with_(arith=mm.ARITH_STRICT, beta=0.3)
    S = 96
    theta = _draws(oracle_py, pb, S)
    table = _mult(pb, [(None, 1.0), (1, 0.9), (1, 1.1)])
    hip = _hip(mm, pb)
    # samples whose scaled kappa stays inside the bounds in every scenario have an oracle twin (the oracle constrains again)
    scaled, keeps = zip(*(_oracle_theta(hip, pb, theta, table[k]) for k in range(3)))
    keep = keeps[0] & keeps[1] & keeps[2]
    assert keep.sum() >= 8
    th = theta[keep]
    sc = hip.scenario_ensemble(th, table, PROBS, want_rt=True)
    assert (sc["status"] == 0).all()
    ref = np.array([_oracle_metrics(oracle_py, pb, th, scaled[k][keep]) for k in range(3)])
    for k in range(3):
        # Rt(t) of the scenario's trajectory with the unscaled beta(t) kappa(t) (test_ensemble.py's bar for Rt quantiles)
        np.testing.assert_allclose(sc["rt"][k], _oracle_rt_quantiles(oracle_py, pb, th, scaled[k][keep]), rtol=1e-9)
        ppc = oracle_py.Oracle(pb).ensemble_quantiles(scaled[k][keep], PROBS)["ppc"]
        np.testing.assert_allclose(sc["ppc"][k], ppc, rtol=1e-9, atol=1e-9)
        # metric bar of test_ensemble.py::test_hip_essential_metrics_table; columns 5, 6 are output times (exact)
        assert np.array_equal(sc["metrics"][k][:, 5:7], ref[k][:, 5:7])
        np.testing.assert_allclose(sc["metrics"][k], ref[k], rtol=1e-9, atol=1e-12)
        # paired differences: quantiles of the oracle's per-sample differences (each value good to 1e-9 of its scale)
        d = ref[k] - ref[0]
        scale = np.maximum(np.max(np.abs(ref[k]), axis=0), np.max(np.abs(ref[0]), axis=0))
        for col in range(d.shape[1]):
            np.testing.assert_allclose(sc["diff"][k, col], np.quantile(d[:, col], PROBS, method="linear"), rtol=0,
                                       atol=2e-9 * scale[col] + 1e-12)
    # the comparison tells the two kappas apart: with the SCALED kappa in the metrics the attack-rate accumulation and the
    # Rt extremes move far beyond the bar (R0 does not: it reads kappa at t = 0, kappa_values[0], which no row scales)
    wrong = _oracle_metrics(oracle_py, pb, scaled[1][keep], scaled[1][keep])
    assert np.all(np.abs(wrong[:, 2] - sc["metrics"][1][:, 2]) > 1e-6 * np.abs(wrong[:, 2]))
    wrong_rt = _oracle_rt_quantiles(oracle_py, pb, scaled[1][keep], scaled[1][keep])
    assert np.max(np.abs(wrong_rt - sc["rt"][1]) / np.abs(wrong_rt)) > 1e-3
    # a stricter lockdown means fewer deaths, a weaker one more
    deaths = np.median(sc["metrics"][:, :, 7], axis=1)
    assert deaths[1] < deaths[0] < deaths[2]


@pytest.mark.gpu
def test_block_independence(mm, oracle_py, shipped):
    pb = shipped.with_(arith=mm.ARITH_FMA)
    theta = _draws(oracle_py, pb, 50)
    table = _mult(pb, [(None, 1.0), (1, 0.9), (3, 1.2)])
    sc = _hip(mm, pb).scenario_ensemble(theta, table, PROBS, want_sero=True)
    for k in range(3):
        one = _hip(mm, pb).scenario_ensemble(theta, table[k:k + 1], PROBS, want_sero=True)
        for key in ("ppc", "sero", "status"):
            assert np.array_equal(sc[key][k], one[key][0]), (k, key)
        assert np.array_equal(sc["metrics"][k], one["metrics"][0], equal_nan=True)
        assert np.array_equal(sc["summary"][k], one["summary"][0], equal_nan=True)


def _check_summaries(sc, K):
    met, st = sc["metrics"], sc["status"]
    for k in range(K):
        ok = st[k] == 0
        both = ok & (st[0] == 0)
        assert sc["n_valid"][k] == ok.sum()
        for col in range(met.shape[2]):
            v = met[k][ok, col]
            mean = 0.0
            for x in v:
                mean += x
            mean /= len(v)
            var = 0.0
            for x in v:
                var += (x - mean) * (x - mean)
            var /= len(v)
            assert sc["summary"][k, col, 0] == mean and sc["summary"][k, col, 1] == np.sqrt(var)
            # numpy's linear interpolation is a different operation sequence: equal to rounding on the column's scale
            np.testing.assert_allclose(sc["summary"][k, col, 2:], np.quantile(v, PROBS, method="linear"), rtol=1e-13,
                                       atol=1e-14 * np.max(np.abs(v)))
            d = met[k][both, col] - met[0][both, col]
            np.testing.assert_allclose(sc["diff"][k, col], np.quantile(d, PROBS, method="linear"), rtol=1e-12,
                                       atol=1e-14 * max(np.max(np.abs(d)), 1e-300))


@pytest.mark.gpu
def test_paired_differences_and_summary(mm, oracle_py, shipped):
    pb = shipped.with_(arith=mm.ARITH_FMA)
    theta = _draws(oracle_py, pb, 300)
    sc = _hip(mm, pb).scenario_ensemble(theta, _mult(pb, [(None, 1.0), (1, 0.9), (1, 1.1)]), PROBS)
    _check_summaries(sc, 3)
    assert (sc["diff"][0] == 0).all()
    assert sc["diff"][1, 7, 2] < 0 < sc["diff"][2, 7, 2]  # median deaths averted / added


@pytest.mark.gpu
def test_global_sort_path(mm, oracle_py, shipped):
    """More samples than the LDS sort holds: segments sorted in global memory."""
    pb = shipped.with_(arith=mm.ARITH_FMA)
    S = 16384 + 700
    theta = _draws(oracle_py, pb, S)
    sc = _hip(mm, pb).scenario_ensemble(theta, _mult(pb, [(None, 1.0), (1, 0.9)]), PROBS)
    _check_summaries(sc, 2)


@pytest.mark.gpu
def test_refusals(mm, shipped):
    hip = _hip(mm, shipped)
    theta = np.tile(np.array(shipped.base_theta), (3, 1))
    nk = len(shipped.kappa_values)
    for bad in (-np.ones((1, nk)), np.full((1, nk), np.nan), np.full((1, nk), np.inf), np.ones((1, nk + 1)), np.ones((1, nk - 1))):
        with pytest.raises(RuntimeError):
            hip.scenario_ensemble(theta, bad, PROBS)
    with pytest.raises(RuntimeError):
        hip.scenario_ensemble(theta, np.ones((1, nk)), [0.5, 1.5])
    # K x S beyond one launch: K S trajectories (T 11 n doubles each) over 4 TB, more than any device holds, refused with
    # INVALID_ARG before anything is allocated; every buffer passed has the size the call's arguments give it
    lib, ctx = hip.lib, hip.ctx
    probs = np.asarray(PROBS)
    S_big = 4096
    theta_big = np.ascontiguousarray(np.tile(np.array(shipped.base_theta), (S_big, 1)))
    K_big = int(np.ceil(4e12 / (S_big * shipped.n_times * 11 * shipped.n * 8)))
    big_k = np.ones((K_big, nk))
    rc = lib.sepaihrd_scenario_ensemble(ctx, theta_big.ctypes.data, S_big, big_k.ctypes.data, K_big, nk, probs.ctypes.data, 5,
                                        None, None, None, None, None, None, None, None)
    assert rc == -1 and b"device memory" in lib.sepaihrd_last_error(ctx)
    # a pending eval_batch_begin
    assert lib.sepaihrd_eval_batch_begin(ctx, theta.ctypes.data, 3) == 0
    with pytest.raises(RuntimeError):
        hip.scenario_ensemble(theta, np.ones((1, nk)), PROBS)
    ll, st = np.empty(3), np.empty(3, dtype=np.int32)
    assert lib.sepaihrd_eval_batch_end(ctx, ll.ctypes.data, st.ctypes.data, None, None, None) == 0
    hip.scenario_ensemble(theta, np.ones((1, nk)), PROBS)  # accepted again once the batch is fetched
    # fp32 states: UNSUPPORTED, as sepaihrd_ensemble_quantiles
    hip.set_precision(1)
    rc = lib.sepaihrd_scenario_ensemble(ctx, theta.ctypes.data, 3, np.ones((1, nk)).ctypes.data, 1, nk, probs.ctypes.data, 5,
                                        None, None, None, None, None, None, None, None)
    assert rc == -4


@pytest.mark.gpu
def test_drop_in_scenario_comparison(mm, oracle_py, shipped, tmp_path):
    """C++ HipPosteriorEnsemble::performScenarioAnalysis as the reference's report runs it: the last analysed sample as
    baseline, the default lockdown scenarios, scenario_comparison.csv.  Each row's trajectory is the oracle's run with
    kappa fixed at the constrained kappa_values x the scenario's multipliers."""
    pb = shipped.with_(arith=mm.ARITH_STRICT)
    samples = _draws(oracle_py, pb, 40, seed0=5)
    burn_in, thinning = 10, 7
    table = np.array([m for _, m in mm.config_io.default_lockdown_scenarios(len(pb.kappa_values))])
    hip = _hip(mm, pb)
    # the last analysed sample (index 38) is one whose three scaled kappas stay inside the bounds: all three rows have an
    # oracle twin
    scaled, keeps = zip(*(_oracle_theta(hip, pb, samples, table[k]) for k in range(3)))
    q = int(np.nonzero(keeps[0] & keeps[1] & keeps[2])[0][0])
    last_idx = list(range(burn_in, len(samples), thinning))[-1]
    samples[[q, last_idx]] = samples[[last_idx, q]]
    last = samples[last_idx]
    host = mm.HostObjective(pb)
    path = tmp_path / "scenarios" / "scenario_comparison.csv"
    path.parent.mkdir()
    got = host.scenario_comparison(samples, burn_in, thinning, path=str(path))
    assert got["names"] == ["baseline", "stricter_lockdown", "weaker_lockdown"]
    orc = oracle_py.Oracle(pb)
    kappa0 = orc.model_parameters(last)["kappa_values"]
    np.testing.assert_array_equal(got["kappa"], kappa0[None, :] * table)
    # the three rows against the oracle's three runs: trajectories with kappa fixed at the scaled values, metrics of those
    # trajectories with the unscaled kappa
    ref = np.array([_oracle_metrics(oracle_py, pb, last[None, :], _oracle_theta(hip, pb, last[None, :], table[k])[0])[0]
                    for k in range(3)])
    assert np.array_equal(got["metrics"][:, 5:7], ref[:, 5:7])
    np.testing.assert_allclose(got["metrics"], ref, rtol=1e-9, atol=1e-12)
    # the file's values are those rows with six significant digits
    rows = [line.split(",") for line in path.read_text().splitlines()[1:]]
    csv_vals = np.array([[float(v) for v in r[1:10]] for r in rows])
    np.testing.assert_allclose(csv_vals, ref[:, [0, 1, 2, 3, 4, 5, 6, 7, 11]], rtol=5e-6, atol=0)
    order = mm.config_io.kappa_column_order(len(kappa0))
    np.testing.assert_allclose(np.array([[float(v) for v in r[10:]] for r in rows]), (kappa0[None, :] * table)[:, order], rtol=5e-6)
    # the file: AnalysisWriter's format, the same bytes as the Python writer's
    ref_path = tmp_path / "ref.csv"
    mm.config_io.write_scenario_comparison(str(ref_path), list(zip(got["names"], got["metrics"], got["kappa"])))
    assert path.read_text() == ref_path.read_text()
    lines = path.read_text().splitlines()
    assert len(lines) == 4 and lines[1].startswith("baseline,")
    # ENE-COVID file of the same samples: the metric summary's seroprevalence_day64
    ene = tmp_path / "ene_covid_validation.csv"
    host.ene_covid_validation(samples, str(ene), burn_in, thinning)
    ens = hip.ensemble_quantiles(samples[burn_in::thinning], PROBS, want_metrics=True)
    ref_ene = tmp_path / "ref_ene.csv"
    mm.config_io.write_ene_covid_validation(str(ref_ene), mm.config_io.sero64_summary(ens["metrics"]))
    assert ene.read_text() == ref_ene.read_text()
