"""SIR posterior ensemble and intervention scenarios on the device (sepaihrd_sir_scenario_ensemble,
HipSIRObjective.scenario_ensemble) against workloads.sir_scenario_reference over the CPU oracle.

Fixture: sir_config0, S = 1000 samples TRUE * exp(N(0, 0.1)) from a fixed seed, probs 0.025 / 0.05 / 0.5 / 0.95 / 0.975, three
scenarios: the baseline, the reference demo's contact reduction 0.7 at day 20, and a compound schedule (transmission 0.3 at
day 30, contact 0.5 at day 45, contact 1.6 at day 90).

Bars (strict arithmetic, abs = rel = 1e-6) are the project's own for ensemble outputs (tests/test_ensemble.py): quantiles rtol
1e-9 / atol 1e-9, metrics, summaries and difference quantiles rtol 1e-9 / atol 1e-12, step counts and peak times equal.  Order
statistics are 1-Lipschitz in the sup norm, so a quantile cannot be further off than the worst sample.
tests/test_sir_ensemble_cpu.py asserts from the oracle alone that no sample's peak is an argmax tie at these bars.

Every comparison prints its largest error as a fraction of its bar before it asserts (run with -s).  No observed figure is
recorded here or in DESIGN.md section 6f yet."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_STATE_BAR = 1e-6  # BASELINE.json north_star (tests/test_gpu_parity.py)
TRUE = np.array([0.03, 1.0, 0.2, 0.2, 0.15])
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
SCENARIOS = [[], [(20, "contact", 0.7)], [(30, "transmission", 0.3), (45, "contact", 0.5), (90, "contact", 1.6)]]
DRAW_SEED = 20250243  # tests/test_sir_ensemble_cpu.py checks the peaks of exactly these draws
TIME_COLS = [2, 4]
WIDE_SEED = {16: 319, 33: 333}  # draws of the two wide problems, free of argmax ties as well


def draws(S=1000):
    rng = np.random.default_rng(DRAW_SEED)
    return TRUE * np.exp(rng.normal(0.0, 0.1, size=(S, 5)))


def synthetic_problem(mm, oracle_py, n, seed=7):
    """n age classes, a fixed-seed contact matrix with R0 around 2, Poisson observations of the true incidence
    (tests/test_gpu_sir.py)"""
    rng = np.random.default_rng(seed + n)
    N = rng.uniform(2e5, 1.5e6, n)
    Cm = rng.uniform(0.2, 1.0, (n, n)) * 12.0 / n
    gamma = rng.uniform(0.15, 0.25, n)
    I0 = np.round(rng.uniform(5, 25, n))
    init = np.concatenate([N - I0, I0, np.zeros(n)])
    times = np.arange(0.0, 121.0)
    names = ["q", "scale_C_total"] + [f"gamma_{i}" for i in range(n)]
    pb = mm.SIRProblem(N=N, C=Cm, gamma=gamma, q=0.03, scale_C_total=1.0, initial_state=init, times=times,
                       obs=np.zeros((len(times), n)), param_names=names)
    traj = oracle_py.sir_simulate(N, Cm, gamma, 0.03, 1.0, init, times)["traj"]
    return pb.with_(obs=rng.poisson(mm.workloads.sir_incidence(pb, traj)).astype(np.float64))


def close(got, ref, rtol, atol):
    """max of |got - ref| / (atol + rtol |ref|) over the entries (NaN must meet NaN, inf must meet the same inf)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / (atol + rtol * np.abs(ref[fin]))))


def check_strict(got, ref, label):
    assert np.array_equal(got["status"], ref["status"]), label
    ok = ref["status"] == 0
    assert np.array_equal(got["n_accept"][ok], ref["n_accept"][ok]) and np.array_equal(got["n_reject"][ok], ref["n_reject"][ok]), label
    assert np.array_equal(got["n_valid"], ref["n_valid"]), label
    fig = {"quantiles": close(got["quantiles"], ref["quantiles"], 1e-9, 1e-9),
           "metrics": close(got["metrics"], ref["metrics"], 1e-9, 1e-12),
           "metric_summary": close(got["metric_summary"], ref["metric_summary"], 1e-9, 1e-12),
           "diff_quantiles": close(got["diff_quantiles"], ref["diff_quantiles"], 1e-9, 1e-12)}
    print(f"{label}: error / bar  " + "  ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert np.array_equal(got["metrics"][..., TIME_COLS][ok], ref["metrics"][..., TIME_COLS][ok]), label  # peak times: equal
    for k, v in fig.items():
        assert v <= 1.0, (label, k, v)


@pytest.fixture(scope="module")
def pb5(mm, oracle_py):
    return mm.workloads.sir_config0(oracle_py.sir_simulate)


@pytest.fixture(scope="module")
def ref1000(mm, oracle_py, pb5):
    return mm.workloads.sir_scenario_reference(oracle_py.sir_simulate, pb5, draws(), SCENARIOS, PROBS)


@pytest.fixture(scope="module")
def got1000(mm, pb5):
    hip = mm.HipSIRObjective(pb5)
    got = hip.scenario_ensemble(draws(), SCENARIOS, PROBS)
    hip.close()
    return got


def test_strict_dopri5_matches_the_reference_over_the_oracle(got1000, ref1000):
    assert np.all(ref1000["status"] == 0) and ref1000["n_accept"].min() >= 200
    check_strict(got1000, ref1000, "config0, 1000 samples x 3 scenarios")
    # the scenarios do something: the reference demo's contact reduction lowers every sample's attack rate
    assert np.all(got1000["metrics"][1, :, 5] < got1000["metrics"][0, :, 5])
    assert np.all(got1000["diff_quantiles"][0] == 0.0)


def test_ensemble_quantiles_is_the_single_empty_scenario(mm, pb5, got1000):
    hip = mm.HipSIRObjective(pb5)
    one = hip.ensemble_quantiles(draws(), PROBS)
    hip.close()
    assert np.array_equal(one["quantiles"], got1000["quantiles"][0]) and np.array_equal(one["metrics"], got1000["metrics"][0])
    assert np.array_equal(one["metric_summary"], got1000["metric_summary"][0])
    assert one["n_valid"] == 1000 and np.all(one["status"] == 0)


@pytest.mark.parametrize("arith", ["strict", "fma"])
@pytest.mark.parametrize("solver", ["dopri5", "cash_karp", "fehlberg78"])
def test_empty_scenario_is_eval_batch_bit_for_bit(mm, pb5, solver, arith):
    """Series 1 (a copy of I) and 2 (S(t0) - S(t), one subtraction) of K = 1 without events against eval_batch's trajectories:
    the extremes over 33 samples (probabilities 0 and 1 pick single order statistics), every value of three single-sample
    calls, and every sample's per-age peak prevalence."""
    code = {"dopri5": mm.SOLVER_DOPRI5, "cash_karp": mm.SOLVER_CASH_KARP54, "fehlberg78": mm.SOLVER_FEHLBERG78}[solver]
    hip = mm.HipSIRObjective(pb5.with_(solver=code, arith=mm.ARITH_FMA if arith == "fma" else mm.ARITH_STRICT))
    theta = draws(33)
    ev = hip.eval_batch(theta, want_traj=True)
    assert np.all(ev["status"] == 0)
    S_, I_ = ev["traj"][:, :, 0:3], ev["traj"][:, :, 3:6]
    cum = pb5.initial_state[None, None, 0:3] - S_
    got = hip.scenario_ensemble(theta, [[]], [0.0, 1.0])
    assert np.array_equal(got["n_accept"][0], ev["n_accept"]) and np.array_equal(got["n_reject"][0], ev["n_reject"])
    q = got["quantiles"][0]
    assert np.array_equal(q[1, 0, :, :3], I_.min(axis=0)) and np.array_equal(q[1, 1, :, :3], I_.max(axis=0))
    assert np.array_equal(q[2, 0, :, :3], cum.min(axis=0)) and np.array_equal(q[2, 1, :, :3], cum.max(axis=0))
    assert np.array_equal(got["metrics"][0][:, 7::2], I_.max(axis=1))
    for s in (0, 16, 32):
        one = hip.scenario_ensemble(theta[s:s + 1], [[]], [0.5], want=("quantiles",))["quantiles"][0]
        assert np.array_equal(one[1, 0, :, :3], I_[s]) and np.array_equal(one[2, 0, :, :3], cum[s])
    hip.close()


@pytest.mark.parametrize("solver", ["cash_karp", "fehlberg78"])
def test_cash_karp_and_fehlberg_against_segments_composed_from_device_runs(mm, pb5, solver):
    """The oracle has no SIR run for these steppers: each scenario of 8 samples is composed from plain device runs, one
    context per sample and segment with that segment's grid, initial state and parameters."""
    code = {"cash_karp": mm.SOLVER_CASH_KARP54, "fehlberg78": mm.SOLVER_FEHLBERG78}[solver]
    pbs = pb5.with_(solver=code)

    def device_segment(N, Cm, gamma, q, scale, init, times, abs_err, rel_err):
        seg = mm.SIRProblem(N=N, C=Cm, gamma=gamma, q=q, scale_C_total=scale, initial_state=init, times=times,
                            obs=np.zeros((len(times), len(N))), param_names=["q"], solver=code, abs_err=abs_err, rel_err=rel_err)
        hip = mm.HipSIRObjective(seg)
        r = hip.eval_batch(np.array([[q]]), want_traj=True)
        hip.close()
        if r["status"][0] != 0:
            raise RuntimeError("segment failed")
        return {"traj": r["traj"][0], "n_accept": int(r["n_accept"][0]), "n_reject": int(r["n_reject"][0])}

    theta = draws(8)
    ref = mm.workloads.sir_scenario_reference(device_segment, pbs, theta, SCENARIOS, PROBS)
    hip = mm.HipSIRObjective(pbs)
    got = hip.scenario_ensemble(theta, SCENARIOS, PROBS)
    hip.close()
    assert np.all(ref["status"] == 0)
    check_strict(got, ref, solver)


def test_fma_within_north_star_tolerance_of_strict(mm, pb5, got1000):
    hip = mm.HipSIRObjective(pb5.with_(arith=mm.ARITH_FMA))
    got = hip.scenario_ensemble(draws(), SCENARIOS, PROBS)
    hip.close()
    assert np.array_equal(got["status"], got1000["status"])
    worst = {}
    for k in ("quantiles", "metrics", "metric_summary", "diff_quantiles"):
        a, b = got[k], got1000[k]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        worst[k] = float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))
    print("fma against strict, max |a - b| / max(|b|, 1): " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < REL_STATE_BAR, (k, v)


@pytest.mark.parametrize("n", [16, 33])
def test_wide_problems_with_a_wavefront_across_scenarios(mm, oracle_py, n):
    """n = 16 (a register row of sixteen) and n = 33 (64 lanes per chain, rows in LDS); S = 257: the wavefronts of 4 chains
    (n = 16) straddle the scenarios and the last one is partial."""
    pb = synthetic_problem(mm, oracle_py, n)
    rng = np.random.default_rng(WIDE_SEED[n])
    theta = pb.current_parameters() * np.exp(rng.normal(0.0, 0.1, size=(257, pb.n_params)))
    ref = mm.workloads.sir_scenario_reference(oracle_py.sir_simulate, pb, theta, SCENARIOS, PROBS)
    hip = mm.HipSIRObjective(pb)
    got = hip.scenario_ensemble(theta, SCENARIOS, PROBS)
    hip.close()
    assert np.all(ref["status"] == 0)
    check_strict(got, ref, f"n = {n}, 257 samples")


@pytest.mark.parametrize("S", [1, 17, 4096, 16385])
def test_sample_counts_on_repeated_samples(mm, pb5, got1000, ref1000, S):
    """16 385 crosses from the LDS sort to the segmented sort.  The same multiset of samples in another order gives the same
    quantile bits; every sample's metric row is the one it has among the 1000; the summaries follow the reference."""
    base = draws()
    idx = np.arange(S) % 1000
    perm = np.random.default_rng(S).permutation(S)
    hip = mm.HipSIRObjective(pb5)
    a = hip.scenario_ensemble(base[idx], SCENARIOS, PROBS)
    b = hip.scenario_ensemble(base[idx[perm]], SCENARIOS, PROBS)
    hip.close()
    assert np.all(a["status"] == 0) and np.array_equal(a["n_valid"], [S] * 3)
    assert np.array_equal(a["metrics"], got1000["metrics"][:, idx]) and np.array_equal(b["metrics"], got1000["metrics"][:, idx[perm]])
    assert np.array_equal(a["n_accept"], got1000["n_accept"][:, idx])
    assert np.array_equal(a["quantiles"], b["quantiles"])
    assert np.array_equal(a["metric_summary"][:, :, 2:], b["metric_summary"][:, :, 2:]) and np.array_equal(a["diff_quantiles"], b["diff_quantiles"])
    if S == 1:
        assert np.array_equal(a["quantiles"][:, :, 0], a["quantiles"][:, :, -1])
    # against the reference: the metric quantiles, and the series quantiles of every 25th output time
    m = ref1000["metrics"][:, idx]
    fig = [close(a["metric_summary"][:, :, 2:], np.moveaxis(np.quantile(m, PROBS, axis=1, method="linear"), 0, -1), 1e-9, 1e-12),
           close(a["diff_quantiles"], np.moveaxis(np.quantile(m - m[0], PROBS, axis=1, method="linear"), 0, -1), 1e-9, 1e-12),
           close(a["quantiles"][:, :, :, ::25], np.moveaxis(np.quantile(ref1000["series"][:, :, :, ::25][:, idx], PROBS, axis=1, method="linear"), 0, 2),
                 1e-9, 1e-9)]
    print(f"S = {S}: error / bar  summary quantiles {fig[0]:.3g}  difference quantiles {fig[1]:.3g}  series quantiles {fig[2]:.3g}")
    assert max(fig) <= 1.0, fig


def test_failed_samples_are_skipped_not_raised(mm, oracle_py, pb5, ref1000):
    attempts = ref1000["n_accept"] + ref1000["n_reject"]
    budget = int(np.median(attempts[0]))
    # the kernel's budget rule: a chain fails when it is still running after max_attempts attempts
    valid = attempts <= budget
    assert 0 < valid[0].sum() < 1000
    pbf = pb5.with_(max_attempts=budget)
    ref = mm.workloads.sir_scenario_reference(oracle_py.sir_simulate, pbf, draws(), SCENARIOS, PROBS)
    assert np.array_equal(ref["status"] == 0, valid)
    hip = mm.HipSIRObjective(pbf)
    got = hip.scenario_ensemble(draws(), SCENARIOS, PROBS)
    hip.close()
    assert np.array_equal(got["status"] == 0, valid) and np.all(got["status"][~valid] == 3)
    assert np.all(np.isnan(got["metrics"][~valid])) and not np.any(np.isnan(got["metrics"][valid]))
    assert np.array_equal(got["n_valid"], valid.sum(axis=1))
    check_strict(got, ref, f"max_attempts = {budget}, valid {valid.sum(axis=1)}")

    hip = mm.HipSIRObjective(pb5.with_(max_attempts=5))
    got = hip.scenario_ensemble(draws(64), SCENARIOS, PROBS)
    hip.close()
    assert np.all(got["status"] == 3) and np.all(got["n_valid"] == 0)
    for k in ("quantiles", "metrics", "metric_summary", "diff_quantiles"):
        assert np.all(np.isnan(got[k])), k


def test_every_combination_of_null_outputs(mm, pb5):
    names = ("quantiles", "metrics", "metric_summary", "diff_quantiles", "status", "n_accept", "n_reject", "n_valid")
    theta = draws(37)
    hip = mm.HipSIRObjective(pb5)
    full = hip.scenario_ensemble(theta, SCENARIOS[:2], PROBS)
    for mask in range(1 << len(names)):
        want = tuple(nm for i, nm in enumerate(names) if mask >> i & 1)
        got = hip.scenario_ensemble(theta, SCENARIOS[:2], PROBS, want=want)
        assert set(got) == set(want)
        for nm in want:
            assert np.array_equal(got[nm], full[nm]), (want, nm)
    assert hip.ensemble_timing()["calls"] == 1 + (1 << len(names))
    hip.close()


def test_a_bad_event_table_is_refused_before_the_device_is_touched(mm, pb5):
    hip = mm.HipSIRObjective(pb5)
    hip.scenario_ensemble(draws(5), SCENARIOS, PROBS)
    before = hip.ensemble_timing()["calls"]
    bad = [[[(201, "contact", 0.7)]], [[(-1, "contact", 0.7)]], [[(30, "contact", 0.7), (20, "contact", 0.7)]],
           [[(1, "contact", 0.9)] * 9], [[(5, 7, 0.5)]], [[(5, "contact", -0.1)]], [[(5, "transmission", 1.5)]],
           [[(5, "contact", float("nan"))]], [[], [(5, "transmission", float("inf"))]]]
    for sc in bad:
        with pytest.raises(ValueError, match="scenario"):  # SEPAIHRD_E_INVALID_ARG with the message of sepaihrd_sir_last_error
            hip.scenario_ensemble(draws(5), sc, PROBS)
    assert hip.ensemble_timing()["calls"] == before
    with pytest.raises(ValueError, match="probabilities"):
        hip.scenario_ensemble(draws(5), SCENARIOS, [0.5, 1.5])
    assert hip.ensemble_timing()["calls"] == before
    # events at the ends of the grid: index 0 is a plain run with the changed parameters, index T - 1 changes nothing
    ends = hip.scenario_ensemble(draws(5), [[], [(200, "contact", 0.1)], [(0, "contact", 0.7), (0, "transmission", 0.25)]], PROBS)
    assert np.array_equal(ends["quantiles"][1], ends["quantiles"][0]) and np.array_equal(ends["metrics"][1], ends["metrics"][0])
    hip.close()
    changed = draws(5) * np.array([0.75, 0.7, 1.0, 1.0, 1.0])  # q (1 - 0.25), scale 0.7: the same single products
    hip = mm.HipSIRObjective(pb5)
    plain = hip.scenario_ensemble(changed, [[]], PROBS)
    hip.close()
    assert np.array_equal(ends["quantiles"][2], plain["quantiles"][0])
    assert np.array_equal(ends["metrics"][2][:, 1:], plain["metrics"][0][:, 1:])  # R0 is the sample's own, before any event


def test_host_scenario_comparison_writes_the_two_files_with_the_direct_call_s_numbers(mm, pb5, tmp_path):
    """HipSIRScenarioAnalysis through HostSIRObjective.scenario_comparison: burn-in and thinning, scenarios from the reference's
    intervention names, both CSVs; every number is the direct call's, formatted with six significant digits."""
    samples = draws(300)
    named = {"baseline": [], "demo": [(20.0, "contact_reduction", 0.7)],
             "compound": [(45.0, "lockdown", 0.5), (30.0, "mask_mandate", 0.3), (90.0, "social_distancing", 1.6)]}
    h = mm.HostSIRObjective(pb5)
    cmp_path, bands_path = tmp_path / "out" / "sir_scenario_comparison.csv", tmp_path / "out" / "sir_posterior_bands.csv"
    got = h.scenario_comparison(samples, named, PROBS, burn_in=100, thinning=2, comparison_path=cmp_path, bands_path=bands_path)
    hip = mm.HipSIRObjective(pb5)
    direct = hip.scenario_ensemble(samples[100::2], SCENARIOS, PROBS)
    hip.close()
    for k in ("quantiles", "metrics", "metric_summary", "diff_quantiles", "status", "n_valid"):
        assert np.array_equal(got[k], direct[k]), k
    labels = ["q2.5", "q5", "q50", "q95", "q97.5"]
    lines = cmp_path.read_text().splitlines()
    assert lines[0] == "scenario,metric,mean,std_dev," + ",".join(labels) + "," + ",".join("diff_" + x for x in labels)
    names = mm.hipabi.sir_metric_names(3)
    assert len(lines) == 1 + 3 * len(names)
    for k, sc in enumerate(named):
        for w, nm in enumerate(names):
            f = lines[1 + k * len(names) + w].split(",")
            assert f[:2] == [sc, nm]
            expect = list(direct["metric_summary"][k, w]) + list(direct["diff_quantiles"][k, w])
            assert f[2:] == ["%g" % v for v in expect], (sc, nm)
    bands = bands_path.read_text().splitlines()
    assert bands[0] == "scenario,series,time,age," + ",".join(labels) and len(bands) == 1 + 3 * 3 * 201 * 4
    row = bands[1 + ((1 * 3 + 1) * 201 + 60) * 4 + 3].split(",")   # scenario "demo", prevalence, day 60, age total
    assert row[:4] == ["demo", "prevalence", "60", "total"]
    assert row[4:] == ["%g" % v for v in direct["quantiles"][1, 1, :, 60, 3]]
    with pytest.raises(RuntimeError, match="grid times only"):
        h.scenario_comparison(samples, {"baseline": [], "off": [(20.5, "lockdown", 0.7)]}, PROBS)
    with pytest.raises(RuntimeError, match="No posterior samples left"):
        h.scenario_comparison(samples, named, PROBS, burn_in=300)


def test_more_scenarios_than_a_grid_dimension_holds(mm, pb5):
    """K = 65 537 scenarios on a three-point grid: the scenario is folded into the x dimension of the fix-up and metric
    launches, so K is bounded by the chain count and the memory alone.  65 536 empty scenarios repeat scenario 0 bit for
    bit; the last one (events at index 0) is a plain run with the changed parameters."""
    pbs = pb5.with_(times=pb5.times[:3], obs=pb5.obs[:3])
    K = 65537
    theta = draws(3)
    hip = mm.HipSIRObjective(pbs)
    got = hip.scenario_ensemble(theta, [[]] * (K - 1) + [[(0, "contact", 0.7), (0, "transmission", 0.25)]], [0.5])
    plain = hip.scenario_ensemble(theta * np.array([0.75, 0.7, 1.0, 1.0, 1.0]), [[]], [0.5])
    hip.close()
    assert np.all(got["status"] == 0) and np.array_equal(got["n_valid"], [3] * K)
    for k in ("quantiles", "metrics", "metric_summary"):
        assert np.all(got[k][:K - 1] == got[k][0]), k
    assert np.all(got["diff_quantiles"][:K - 1] == 0.0)
    assert np.array_equal(got["quantiles"][K - 1], plain["quantiles"][0])
    assert np.array_equal(got["metrics"][K - 1][:, 1:], plain["metrics"][0][:, 1:])
    assert np.all(got["metrics"][K - 1][:, 5] < got["metrics"][0][:, 5])
