"""GPU tests of the C++ host mirror: IObjectiveFunction::calculate / calculateBatch through
HipSEPAIHRDObjectiveFunction, SimulationCache semantics, and the multi-chain Adaptive-Metropolis
driver against the oracle's restatement of MetropolisHastingsSampler (bit-exact accept/reject
sequences for a fixed seed)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_calculate_matches_c_abi_and_uses_cache(mm, ref_fixture):
    pb = ref_fixture
    host = mm.HostObjective(pb)
    direct = mm.HipObjective(pb)
    rs = np.random.RandomState(0)
    lo, hi, _ = pb.bounds_arrays()
    thetas = lo + (hi - lo) * rs.uniform(0, 1, (6, pb.n_params))
    want = direct.eval_batch(thetas)["loglik"]
    got = np.array([host.calculate(t) for t in thetas])
    assert np.array_equal(got, want)
    st0 = host.cache_stats()
    assert st0["calls"] == 6 and st0["hits"] == 0 and st0["size"] == 6
    again = np.array([host.calculate(t) for t in thetas])      # CacheEqualityTest (:349)
    assert np.array_equal(again, want)
    assert host.cache_stats()["hits"] == 6
    # parameters equal to 1e-8 share a cache entry (hash of the quantised theta, no theta compare)
    v = host.calculate(thetas[0] + 2e-9)
    assert v == want[0] and host.cache_stats()["hits"] == 7
    out, status = host.calculate_batch(thetas)                  # batch path bypasses the cache
    assert np.array_equal(out, want) and np.all(status == 0)


def test_calculate_returns_lowest_for_invalid_theta(mm, shipped):
    pb = shipped
    pb.bounds = dict(pb.bounds)
    pb.bounds["seed_exposed"] = (5.0, 1e9)
    host = mm.HostObjective(pb)
    th = pb.base_theta.copy()
    th[pb.param_names.index("seed_exposed")] = 9e8
    assert host.calculate(th) == mm.LOWEST


def test_integration_failure_propagates_like_simulation_exception(mm, ref_fixture):
    pb = ref_fixture.with_(abs_err=0.0, rel_err=1e-300, max_attempts=0)
    # the host mirror uses the library default attempt budget (1e6): keep the case cheap with a 4-point grid
    pb = pb.with_(times=pb.times[:4], obs_H=pb.obs_H[:4], obs_ICU=pb.obs_ICU[:4], obs_D=pb.obs_D[:4])
    host = mm.HostObjective(pb)
    with pytest.raises(RuntimeError, match="integration failed"):
        host.calculate(pb.base_theta)
    out, status = host.calculate_batch(pb.base_theta[None, :])
    assert status[0] == 3 and out[0] == mm.LOWEST


@pytest.mark.parametrize("fixture_name,iters,burn", [("ref_fixture", 400, 150), ("shipped", 160, 60)])
def test_multichain_mh_matches_oracle_sampler(mm, oracle_py, request, fixture_name, iters, burn):
    """Same seed -> identical accept/reject sequence, accepted counts, samples and scale as the CPU
    restatement of MetropolisHastingsSampler, chain by chain (chain c uses mt19937(seed + c))."""
    pb = request.getfixturevalue(fixture_name)
    pb.constraint_mode = mm.CONSTRAINT_REFLECT
    C = 5
    from mmid_amd import draws
    if fixture_name == "shipped":
        x0 = draws.jitter_draws(pb, 100, C)
    else:
        rs = np.random.RandomState(1)
        lo, hi, _ = pb.bounds_arrays()
        x0 = lo + (hi - lo) * rs.uniform(0.3, 0.7, (C, pb.n_params))
    host = mm.HostObjective(pb)
    got = host.metropolis_hastings(x0, seed=11, iterations=iters, burn_in=burn, adaptation_period=40, thinning=7)
    orc = oracle_py.Oracle(pb)
    for c in range(C):
        ref = orc.metropolis_hastings(x0[c], seed=11 + c, iterations=iters, burn_in=burn, adaptation_period=40,
                                      thinning=7)
        assert np.array_equal(got["accept_trace"][c], ref["accept_trace"]), c
        assert got["accepted"][c] == ref["accepted"]
        np.testing.assert_allclose(got["samples"][c], ref["samples"], rtol=0, atol=0)
        np.testing.assert_allclose(got["sample_values"][c], ref["sample_values"], rtol=1e-10)
        np.testing.assert_allclose(got["final_scale"][c], ref["final_scale"], rtol=1e-14)
        np.testing.assert_allclose(got["best_value"][c], ref["best_value"], rtol=1e-10)


def test_multichain_equals_scalar_interface(mm, ref_fixture):
    """optimizeChains (one batched launch per iteration) == optimize() per chain through calculate()."""
    pb = ref_fixture
    rs = np.random.RandomState(3)
    lo, hi, _ = pb.bounds_arrays()
    x0 = lo + (hi - lo) * rs.uniform(0.3, 0.7, (3, pb.n_params))
    a = mm.HostObjective(pb).metropolis_hastings(x0, seed=5, iterations=120, burn_in=40, adaptation_period=20)
    b = mm.HostObjective(pb).metropolis_hastings(x0, seed=5, iterations=120, burn_in=40, adaptation_period=20,
                                                 scalar_interface=True)
    assert np.array_equal(a["accept_trace"], b["accept_trace"])
    assert np.array_equal(a["samples"], b["samples"])


def test_batched_hill_climbing_follows_the_serial_search(mm, oracle_py, shipped):
    """BatchedHillClimbingOptimizer (cloud, backtracking and expansion each as ONE launch) walks the
    path of the one-call-at-a-time HillClimbingOptimizer restatement in the oracle
    (HillClimbingOptimizer.cpp:132-353), same seed and virtual threads."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=0)
    iters, mult, threads, seed = 25, 4, 4, 99
    ref = oracle_py.Oracle(pb).hill_climbing(pb.base_theta, seed, iters, mult, threads)
    host = mm.HostObjective(pb)
    got = host.hill_climbing(pb.base_theta, seed, iters, mult, threads)
    np.testing.assert_allclose(got["trace"], ref["trace"], rtol=1e-10)
    np.testing.assert_allclose(got["best"], ref["best"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got["final_cov"], ref["final_cov"], rtol=1e-9, atol=1e-18)
    assert got["best_value"] >= got["trace"][0] and np.all(np.diff(got["trace"]) >= 0)
    # three launches per iteration at most (cloud, backtracking, expansion) + the initial value
    assert got["launches"] <= 3 * iters + 1 and got["evaluations"] >= ref["evaluations"]
    # the scalar interface (one launch per value, through calculate() and its cache) gives the same search
    scalar = mm.HostObjective(pb).hill_climbing(pb.base_theta, seed, iters, mult, threads, use_scalar_interface=True)
    assert np.array_equal(scalar["trace"], got["trace"]) and np.array_equal(scalar["best"], got["best"])


@pytest.mark.parametrize("settings", [
    dict(),                                                                     # the reference's defaults
    dict(variant=1),                                                            # quantum-behaved
    dict(variant=3),                                                            # Levy flight
    dict(variant=2, use_adaptive_parameters=1),                                 # adaptive + elitist learning
    dict(variant=4, use_adaptive_parameters=1, use_opposition_learning=1),      # hybrid
    dict(variant=4, topology=2, max_stagnation=2, restart_threshold=1e300),     # von Neumann grid + restarts
    dict(topology=1), dict(topology=3),                                         # ring, random dynamic
], ids=["standard", "quantum", "levy", "adaptive", "hybrid-obl", "hybrid-grid-restart", "ring", "random"])
def test_batched_particle_swarm_follows_the_serial_swarm(mm, oracle_py, shipped, settings):
    """BatchedParticleSwarmOptimization (one launch per swarm phase) against the one-particle-at-a-time restatement
    of ParticleSwarmOptimizer.cpp:105-948 in the oracle, same seed.  With the GLOBAL_BEST topology the oracle runs
    the reference's serial order; the other topologies read neighbours' personal bests inside the loop, so there
    the oracle is told to defer the personal-best updates as the batched evaluation does."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=0)
    iters, swarm, seed = 14, 12, 21
    deferred = int(settings.get("topology", 0) != 0)
    ref = oracle_py.Oracle(pb).particle_swarm(pb.base_theta, seed, iterations=iters, swarm_size=swarm,
                                              deferred_personal_bests=deferred, **settings)
    got = mm.HostObjective(pb).particle_swarm(pb.base_theta, seed, iterations=iters, swarm_size=swarm, **settings)
    np.testing.assert_allclose(got["trace"], ref["trace"], rtol=1e-10)
    np.testing.assert_allclose(got["best"], ref["best"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got["final_cov"], ref["final_cov"], rtol=1e-9, atol=1e-18)
    assert got["evaluations"] == ref["evaluations"]
    assert np.all(np.diff(got["trace"]) >= 0) and got["best_value"] == got["trace"][-1]
    # one launch per swarm phase (+ the elitist trials, one value each): far fewer launches than values
    assert got["launches"] <= 2 + iters + 3 * (iters // 5 + 1) + iters // 2
    assert got["launches"] < got["evaluations"] / 4


def test_particle_swarm_shipped_settings_and_errors(mm, shipped):
    """data/configuration/pso_settings.txt ships swarm_size 1, iterations 1: the run is two evaluations and the
    covariance divides by swarm_size - 1 = 0 (ParticleSwarmOptimizer.cpp:233) -- kept, not papered over."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=0)
    host = mm.HostObjective(pb)
    got = host.particle_swarm(pb.base_theta, 1, iterations=1, swarm_size=1, omega_start=0.9, omega_end=0.4,
                              c1_initial=1.5, c1_final=1.5, c2_initial=1.5, c2_final=1.5, report_interval=1)
    assert got["evaluations"] == 2 and got["launches"] == 2
    assert not np.all(np.isfinite(got["final_cov"]))
    np.testing.assert_allclose(got["trace"][0], max(host.calculate(pb.base_theta), got["best_value"]), rtol=1e-12)
    for bad in (dict(iterations=0), dict(swarm_size=0), dict(variant=5), dict(topology=4), dict(omega_start=-1),
                dict(max_stagnation=0)):
        with pytest.raises(RuntimeError):
            host.particle_swarm(pb.base_theta, 1, **bad)


def test_two_phase_calibration_follows_the_reference_flow(mm, oracle_py, shipped):
    """HipModelCalibrator (ModelCalibrator.cpp:47-159): HC in clamp mode -> conditioned covariance ->
    MH in reflect mode -> objective value of every stored sample; chain 0 of a 3-chain run walks the
    path of the oracle's one-chain restatement."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=0)
    kw = dict(hc_seed=5, mh_seed=6, hc_iterations=12, mh_iterations=300, burn_in=100, cloud_size_multiplier=2,
              threads=4, adaptation_period=50, thinning=2)
    ref = oracle_py.Oracle(pb).calibrate(pb.base_theta, **kw)
    got = mm.HostObjective(pb).calibrate(chains=3, **kw)
    np.testing.assert_allclose(got["initial_value"], ref["initial_value"], rtol=1e-10)
    np.testing.assert_allclose(got["phase1_best_value"], ref["phase1_best_value"], rtol=1e-10)
    np.testing.assert_allclose(got["phase2_cov"], ref["phase2_cov"], rtol=1e-8, atol=1e-20)
    assert np.array_equal(got["accept_trace"][0], ref["accept_trace"])
    assert 0 < ref["accept_trace"].sum() < len(ref["accept_trace"])
    assert got["n_samples"] == ref["n_samples"]
    np.testing.assert_allclose(got["samples"][0], ref["samples"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got["sample_values"][0], ref["sample_values"], rtol=1e-10)
    np.testing.assert_allclose(got["mcmc_objective_values"][0], ref["mcmc_objective_values"], rtol=1e-10)
    # the other chains start from the same optimum with their own streams
    assert not np.array_equal(got["accept_trace"][1], got["accept_trace"][0])
    assert got["best_value"] >= ref["best_value"] * (1 - 1e-10)


def test_swarm_then_sampler_calibration(mm, oracle_py, shipped):
    """SEPAIHRDModelCalibration::runPSOMCMC (SEPAIHRDModelCalibration.cpp:179-208): the swarm is phase 1 of the same
    ModelCalibrator flow -- its best vector starts the chains, its personal-best covariance is conditioned
    (ModelCalibrator.cpp:93-131) and handed to the sampler."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=0)
    pso = dict(iterations=10, swarm_size=16, seed=8)
    orc = oracle_py.Oracle(pb)
    ref1 = orc.particle_swarm(pb.base_theta, 8, iterations=10, swarm_size=16)
    got = mm.HostObjective(pb).calibrate_pso(pso, mh_seed=9, mh_iterations=200, burn_in=50, adaptation_period=50,
                                             thinning=2, chains=2)
    np.testing.assert_allclose(got["phase1_best_value"], ref1["best_value"], rtol=1e-10)
    np.testing.assert_allclose(got["phase2_cov"], orc.condition_covariance(ref1["final_cov"]), rtol=1e-8, atol=1e-20)
    # the chains start at the overall best so far: the swarm's, or the initial guess when the swarm found nothing better
    start = ref1["best"] if ref1["best_value"] > got["initial_value"] else pb.base_theta
    np.testing.assert_allclose(got["samples"][0, 0], start, rtol=1e-12, atol=1e-14)
    # phase 2 is the code path test_two_phase_calibration_follows_the_reference_flow pins against the oracle
    assert 0 < got["accept_trace"][0].sum() < 199 and not np.array_equal(got["accept_trace"][0], got["accept_trace"][1])
    assert got["n_samples"] == 100 and np.all(np.isfinite(got["mcmc_objective_values"]))
    assert got["best_value"] >= max(ref1["best_value"], got["initial_value"]) * (1 - 1e-10)


def _multiplier_fixture(mm, ref_fixture):
    """reference test fixture + calibrated E0 / I0 multipliers (the finite-difference objective reads them)."""
    pb = ref_fixture
    names = list(pb.param_names) + ["E0_multiplier", "I0_multiplier"]
    sig = dict(pb.sigmas); sig.update(E0_multiplier=0.05, I0_multiplier=0.05)
    bnd = dict(pb.bounds); bnd.update(E0_multiplier=(0.5, 1.2), I0_multiplier=(0.1, 3.0))
    theta = np.concatenate([np.asarray(pb.base_theta), [1.2, 0.8]])  # E0 multiplier AT its upper bound
    return pb.with_(param_names=names, sigmas=sig, bounds=bnd, base_theta=theta, arith=mm.ARITH_STRICT, constraint_mode=0)


def test_finite_difference_gradient_objective(mm, oracle_py, ref_fixture):
    """HipSEPAIHRDGradientObjectiveFunction (P perturbed runs in one launch) == the restatement of
    SEPAIHRDGradientObjectiveFunction.cpp:15-171, incl. a multiplier perturbed past its upper bound
    (the reference reads it unconstrained)."""
    pb = _multiplier_fixture(mm, ref_fixture)
    theta = np.asarray(pb.base_theta)
    ref_v, ref_g = oracle_py.Oracle(pb).evaluate_with_gradient(theta)
    got_v, got_g = mm.HostObjective(pb).evaluate_with_gradient(theta)
    np.testing.assert_allclose(got_v, ref_v, rtol=1e-11)
    assert np.all(np.isfinite(ref_g)) and np.count_nonzero(ref_g) >= 4
    # the difference quotient divides the 1e-12-relative log / pow differences by eps ~ 1e-4 |theta|
    scale = np.abs(ref_v) * 1e-10 / (1e-4 * np.maximum(np.abs(theta), 1e-4))
    assert np.all(np.abs(got_g - ref_g) <= np.maximum(1e-6 * np.abs(ref_g), scale)), (got_g, ref_g)
    # differentiating the smooth parameters by hand agrees with the quotient's sign and size
    k = pb.param_names.index("beta")
    h = 1e-4 * max(abs(theta[k]), 1e-4)
    tp = theta.copy(); tp[k] += h
    o = oracle_py.Oracle(pb)
    assert np.isclose((o.calculate(tp) - o.calculate(theta)) / h, ref_g[k], rtol=1e-6)


def test_no_u_turn_sampler_follows_the_reference_flow(mm, oracle_py, ref_fixture):
    """HipNUTSSampler against the restatement of NUTSSampler.cpp:41-428 over the finite-difference gradient
    objective, same seed: same tree depths, step sizes, samples and values.  The repeated parameter vectors the
    reference evaluates again (three gradient calls per leaf) are served from the last evaluations: the
    reference's call count with about a third of the launches."""
    pb = _multiplier_fixture(mm, ref_fixture)
    theta = np.concatenate([np.asarray(ref_fixture.base_theta), [1.0, 0.8]])
    pb = pb.with_(base_theta=theta, constraint_mode=1)
    kw = dict(iterations=10, adaptation_window=4, max_tree_depth=3)
    ref = oracle_py.Oracle(pb).nuts(theta, 3, **kw)
    got = mm.HostObjective(pb).nuts(theta, 3, **kw)
    assert np.array_equal(got["depth_trace"], ref["depth_trace"]) and ref["depth_trace"].max() >= 2
    np.testing.assert_allclose(got["epsilon_trace"], ref["epsilon_trace"], rtol=1e-6)
    np.testing.assert_allclose(got["samples"], ref["samples"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got["sample_values"], ref["sample_values"], rtol=1e-6)
    assert got["gradient_calls"] == ref["gradient_calls"]
    assert got["gradient_launches"] <= 0.45 * got["gradient_calls"]
    assert got["best_value"] == got["sample_values"].max()


def test_finite_difference_gradient_row_mismatch_follows_the_reference(mm, oracle_py, shipped):
    """With run-up output rows the reference's perturbed likelihood fails its dimension check:
    every entry is (lowest() - f) / eps (here -inf), no simulation is needed for it."""
    pb = shipped.with_(arith=mm.ARITH_STRICT)
    theta = np.asarray(pb.base_theta)
    ref_v, ref_g = oracle_py.Oracle(pb).evaluate_with_gradient(theta)
    got_v, got_g = mm.HostObjective(pb).evaluate_with_gradient(theta)
    np.testing.assert_allclose(got_v, ref_v, rtol=1e-11)
    assert np.array_equal(got_g, ref_g) and np.all(np.isneginf(ref_g))


def test_device_resident_sampler_state_matches_host_loop(mm, oracle_py, shipped):
    """optimizeChainsOnDevice (covariance, Cholesky factor, running mean and history in HBM; rank-one
    updates, two-pass refresh and factorisation as kernels) gives the numbers of the host loop bit for
    bit, and chain 0's accept trace is the oracle's."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    C, iters, burn, ap = 6, 260, 60, 40   # refresh at t = 80, 120, ... with >= P + 10 = 72 states in the history
    x0 = oracle_py.Oracle(pb).jitter_draws(pb.base_theta, 3, C, mode=1)
    kw = dict(seed=17, iterations=iters, burn_in=burn, adaptation_period=ap, thinning=5)
    host = mm.HostObjective(pb).metropolis_hastings(x0, **kw)
    dev = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, **kw)
    assert np.array_equal(dev["accept_trace"], host["accept_trace"])
    assert 0 < host["accept_trace"].sum() < host["accept_trace"].size
    for k in ("accepted", "best_value", "best", "final_scale", "samples", "sample_values"):
        assert np.array_equal(dev[k], host[k]), k
    ref = oracle_py.Oracle(pb).metropolis_hastings(x0[0], 17, iters, burn, adaptation_period=ap, thinning=5)
    assert np.array_equal(dev["accept_trace"][0], ref["accept_trace"])


@pytest.mark.parametrize("iters", [1, 2, 3, 5])
def test_device_resident_sampler_short_runs(mm, shipped, iters):
    """The ends of the device-resident loop (first proposal without a test, last test without a proposal, the
    bookkeeping that trails by one evaluation): runs of 1, 2, 3 and 5 iterations equal the host loop."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    from mmid_amd import draws
    x0 = draws.jitter_draws(pb, 5, 4)
    kw = dict(seed=29, iterations=iters, burn_in=0, adaptation_period=2, thinning=1)
    host = mm.HostObjective(pb).metropolis_hastings(x0, **kw)
    dev = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, **kw)
    for k in ("accept_trace", "accepted", "best_value", "best", "final_scale", "samples", "sample_values"):
        assert np.array_equal(dev[k], host[k]), k


def test_chain_groups_on_separate_streams_give_the_single_group_result(mm, oracle_py, shipped):
    """optimizeChainGroupsOnDevice: 7 chains in 3 ragged groups (one context, stream and host thread each)
    == one group; chain c draws from mt19937(seed + c) whatever the grouping."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    x0 = oracle_py.Oracle(pb).jitter_draws(pb.base_theta, 9, 7, mode=1)
    kw = dict(seed=23, iterations=150, burn_in=40, adaptation_period=30, thinning=5)
    one = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, **kw)
    objs = [mm.HostObjective(pb) for _ in range(3)]
    grp = mm.hostabi.metropolis_hastings_groups(objs, x0, **kw)
    for k in ("accept_trace", "accepted", "best_value", "best"):
        assert np.array_equal(grp[k], one[k]), k


def test_device_resident_sampler_with_158_parameters(mm, oracle_py, shipped):
    """BASELINE config 5's shape (16 age groups, 158 calibrated parameters): the factorisation keeps a packed
    lower triangle in LDS; device-resident state == host loop."""
    pb = mm.widen_age_classes(shipped, 4)
    pb.arith = mm.ARITH_STRICT
    pb.constraint_mode = 1
    pb.times = pb.times[:60]
    pb = pb.with_(obs_H=pb.obs_H[:40], obs_ICU=pb.obs_ICU[:40], obs_D=pb.obs_D[:40])
    from mmid_amd import draws
    x0 = draws.jitter_draws(pb, 3, 3)
    kw = dict(seed=29, iterations=230, burn_in=20, adaptation_period=30, thinning=10)  # refreshes from t = 180 (>= P + 10 rows)
    host = mm.HostObjective(pb).metropolis_hastings(x0, **kw)
    dev = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, **kw)
    for k in ("accept_trace", "accepted", "best_value", "best", "samples", "sample_values", "final_scale"):
        assert np.array_equal(dev[k], host[k]), k


@pytest.mark.parametrize("problem", ["headline", "shipped"])
def test_device_sampler_accept_traces_in_production_arithmetic(mm, oracle_py, synth400, shipped, problem):
    """The arithmetic bench.py's headline number is measured in (fma: contraction, folded constants, hardware
    log2 / exp2 in the step-size factor) against the bit-exact contract of the north star: device-resident
    Adaptive-Metropolis, fixed seed, 6 chains x 400 iterations with covariance refreshes -- accept/reject
    sequences and accepted counts EQUAL the oracle's strict-arithmetic MetropolisHastingsSampler restatement
    (MetropolisHastingsSampler.cpp:283-351), hence the stored samples are the same bits; the log-likelihoods
    agree to 1e-7 relative.  (A likelihood that differs in the 9th digit can flip an accept test whose uniform
    falls inside that gap: for these seeds none does.)"""
    pb = (synth400 if problem == "headline" else shipped).with_(arith=mm.ARITH_FMA, constraint_mode=1, solver=0)
    C, iters, burn, ap = 6, 400, 100, 50
    x0 = oracle_py.Oracle(pb).jitter_draws(pb.base_theta, 41, C, mode=1)
    kw = dict(iterations=iters, burn_in=burn, adaptation_period=ap, thinning=5)
    dev = mm.HostObjective(pb).metropolis_hastings(x0, seed=31, device_state=True, **kw)
    assert 0 < dev["accept_trace"].sum() < dev["accept_trace"].size
    orc = oracle_py.Oracle(pb.with_(arith=mm.ARITH_STRICT))
    for c in range(C):
        ref = orc.metropolis_hastings(x0[c], 31 + c, iters, burn, adaptation_period=ap, thinning=5)
        assert np.array_equal(dev["accept_trace"][c], ref["accept_trace"]), c
        assert dev["accepted"][c] == ref["accepted"]
        assert np.array_equal(dev["samples"][c], ref["samples"])
        np.testing.assert_allclose(dev["sample_values"][c], ref["sample_values"], rtol=1e-7)
        np.testing.assert_allclose(dev["final_scale"][c], ref["final_scale"], rtol=1e-14)


def test_covariance_refresh_from_running_moments_against_the_two_pass_form(mm, oracle_py, shipped):
    """recomputeFullCovariance (MetropolisHastingsSampler.cpp:168-199) from running co-moments (the default: O(P^2) per
    refresh, no history) against the reference's two literal passes over the whole history, both on the device and both
    bit-identical to the host loop and to the oracle in the same mode; between the modes the final covariances agree to
    1e-11 of their largest entry, the refreshed running mean is the same sum in the same order (the samples -- proposals
    formed from the factor -- differ by rounding only) and the accept traces are equal."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    C, iters, burn, ap = 5, 330, 80, 50
    x0 = oracle_py.Oracle(pb).jitter_draws(pb.base_theta, 3, C, mode=1)
    kw = dict(seed=43, iterations=iters, burn_in=burn, adaptation_period=ap, thinning=7)
    out = {}
    for two_pass in (False, True):
        host = mm.HostObjective(pb).metropolis_hastings(x0, two_pass_covariance=two_pass, **kw)
        dev = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, two_pass_covariance=two_pass, **kw)
        for k in ("accept_trace", "accepted", "best_value", "best", "final_scale", "samples", "sample_values", "final_cov"):
            assert np.array_equal(dev[k], host[k]), (two_pass, k)
        ref = oracle_py.Oracle(pb).metropolis_hastings(x0[1], 43 + 1, iters, burn, adaptation_period=ap, thinning=7,
                                                       two_pass_covariance=two_pass)
        assert np.array_equal(dev["accept_trace"][1], ref["accept_trace"])
        assert np.array_equal(dev["final_cov"][1], ref["final_cov"])
        assert np.array_equal(dev["samples"][1], ref["samples"])
        out[two_pass] = dev
    a, b = out[False], out[True]
    assert np.array_equal(a["accept_trace"], b["accept_trace"])
    scale = np.abs(b["final_cov"]).max(axis=(1, 2), keepdims=True)
    # ~1e-13 per refresh; the states themselves then differ by rounding (proposals are formed from the factors)
    assert (np.abs(a["final_cov"] - b["final_cov"]) / scale).max() < 1e-11
    np.testing.assert_allclose(a["samples"], b["samples"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("window", [2, 7, 33])
def test_ring_of_newest_states_smaller_than_the_adaptation_period(mm, shipped, window):
    """The device keeps the newest `adaptation_window` states only; queued rank-one and co-moment updates are caught up
    before the ring overwrites a state they read.  Whatever the window -- 2 (every commit forces a catch-up), 7, 33
    against a period of 40 -- the run is the default one bit for bit, final covariance (rank-one updates after the last
    refresh) included."""
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    from mmid_amd import draws
    x0 = draws.jitter_draws(pb, 5, 4)
    kw = dict(seed=29, iterations=215, burn_in=30, adaptation_period=40, thinning=3)
    want = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, **kw)
    got = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, adaptation_window=window, **kw)
    for k in ("accept_trace", "accepted", "best_value", "best", "final_scale", "samples", "sample_values", "final_cov"):
        assert np.array_equal(got[k], want[k]), k


def test_sampler_entry_points_in_any_call_pattern(mm, shipped):
    """sepaihrd_mh_adapt reads the NEWEST state whatever came before it: commit, commit, adapt, commit, adapt, adapt
    (updates queued with the state they read, applied when the covariance is read) against a numpy restatement of
    updateCovarianceRank1 (MetropolisHastingsSampler.cpp:154-166) applied at once; then the running moments, the
    stored samples, the summary records (means, variances, best value, accepted count) and the bounds of
    read_history / read_samples."""
    import ctypes as C
    from mmid_amd import draws, hipabi
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=mm.CONSTRAINT_REFLECT)
    Cn, P = 9, pb.n_params
    lib = hipabi.load_library()
    rng = np.random.default_rng(5)
    x0 = draws.jitter_draws(pb, 3, Cn)
    cov0 = np.diag((0.02 * np.maximum(np.abs(pb.base_theta), 1e-3)) ** 2) + 1e-6 * np.eye(P)
    hip = mm.HipObjective(pb)
    mh = hipabi.mh_create(lib, hip.ctx, Cn, 12, x0, cov0, thinning=2, adaptation_window=3)
    assert mh
    lp0 = np.empty(Cn)
    assert lib.sepaihrd_mh_evaluate_current(mh, lp0.ctypes.data, None) == 0
    states = [x0.copy()]
    cov = np.repeat(cov0[None], Cn, axis=0)
    mean = x0.copy()
    accepted = np.zeros(Cn)

    def step(accept_mask):
        z = rng.standard_normal((Cn, P))
        scale = np.full(Cn, 0.4)
        ll = np.empty(Cn)
        assert lib.sepaihrd_mh_propose(mh, z.ctypes.data, scale.ctypes.data, ll.ctypes.data, None) == 0
        prop = np.empty((Cn, P))
        assert lib.sepaihrd_mh_read_proposal(mh, prop.ctypes.data) == 0
        acc = np.ascontiguousarray(accept_mask, dtype=np.uint8)
        assert lib.sepaihrd_mh_commit(mh, acc.ctypes.data) == 0
        states.append(np.where(acc[:, None] & 1, prop, states[-1]))
        accepted[:] += acc & 1

    def adapt(gamma):
        assert lib.sepaihrd_mh_adapt(mh, gamma, 0, 0) == 0
        d = states[-1] - mean
        cov[:] = (1.0 - gamma) * cov + gamma * (d[:, :, None] * d[:, None, :])
        mean[:] += gamma * d

    pattern = np.arange(Cn) % 2
    step(pattern); step(1 - pattern); adapt(0.3); step(pattern); adapt(0.2); adapt(0.1)
    step(np.ones(Cn)); step(pattern); step(1 - pattern)   # the ring (3 states) wraps over the states the updates read
    got = np.empty((Cn, P, P))
    assert lib.sepaihrd_mh_read_covariance(mh, got.ctypes.data) == 0
    assert np.array_equal(got, cov)
    # running moments of all 7 states against numpy (different summation order: agreement, not identity)
    hist = np.stack(states, axis=1)                      # [C][7][P]
    wmean, m2 = np.empty((Cn, P)), np.empty((Cn, P, P))
    assert lib.sepaihrd_mh_read_moments(mh, wmean.ctypes.data, m2.ctypes.data) == 0
    np.testing.assert_allclose(wmean, hist.mean(axis=1), rtol=1e-13)
    dev = hist - hist.mean(axis=1, keepdims=True)
    want_m2 = np.einsum("csi,csj->cij", dev, dev)
    il = np.tril_indices(P)
    assert np.abs(m2[:, il[0], il[1]] - want_m2[:, il[0], il[1]]).max() <= 1e-12 * np.abs(want_m2).max()
    # samples: states 0, 2, 4, 6
    assert lib.sepaihrd_mh_history_length(mh) == 7 and lib.sepaihrd_mh_sample_count(mh) == 4
    kept = np.empty((Cn, 4, P))
    assert lib.sepaihrd_mh_read_samples(mh, 0, 4, kept.ctypes.data) == 0
    assert np.array_equal(kept, hist[:, ::2])
    assert lib.sepaihrd_mh_read_samples(mh, 2, 3, kept.ctypes.data) != 0      # beyond what is stored
    rows = np.array([4, 6], dtype=np.int32)
    two = np.empty((Cn, 2, P))
    assert lib.sepaihrd_mh_read_history(mh, rows.ctypes.data, 2, two.ctypes.data) == 0
    assert np.array_equal(two, hist[:, [4, 6]])
    rows[0] = 3                                                                # left the ring of 3
    assert lib.sepaihrd_mh_read_history(mh, rows.ctypes.data, 2, two.ctypes.data) != 0
    # summary records over samples 1.. (states 2, 4, 6)
    lib.sepaihrd_mh_set_values.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.sepaihrd_mh_set_values(mh, lp0.ctypes.data) == 0
    rec = np.empty((Cn, 2 * P + 2))
    assert lib.sepaihrd_mh_summary_records(mh, 1, rec.ctypes.data, None) == 0
    np.testing.assert_allclose(rec[:, :P], hist[:, 2::2].mean(axis=1), rtol=1e-14)
    np.testing.assert_allclose(rec[:, P:2 * P], hist[:, 2::2].var(axis=1, ddof=1), rtol=1e-9, atol=1e-30)
    assert np.array_equal(rec[:, 2 * P], lp0) and np.array_equal(rec[:, 2 * P + 1], accepted)
    lib.sepaihrd_mh_destroy(mh)


def test_sampler_state_fits_at_the_reference_run_length(mm, shipped):
    """data/configuration/mcmc_settings.txt: 100 000 iterations, thinning 100.  The sampler state of BASELINE configs[2]'s
    65 536 chains fits the device (ring + samples + covariance, factor and second moment: ~47 GB) where the whole history
    (65 536 x 100 000 x 62 doubles = 3.25 TB) could not; the two-pass mode says so instead of failing in an allocation."""
    from mmid_amd import hipabi
    pb = shipped.with_(constraint_mode=1)
    lib = hipabi.load_library()
    hip = mm.HipObjective(pb)
    P = pb.n_params
    x0 = np.repeat(np.asarray(pb.base_theta)[None], 65536, axis=0)
    cov0 = 1e-4 * np.eye(P)
    assert not hipabi.mh_create(lib, hip.ctx, 65536, 100000, x0, cov0, thinning=100, covariance_mode=hipabi.MH_COV_TWO_PASS)
    assert b"GB" in lib.sepaihrd_last_error(hip.ctx)
    mh = hipabi.mh_create(lib, hip.ctx, 65536, 100000, x0, cov0, thinning=100)
    assert mh, lib.sepaihrd_last_error(hip.ctx)
    lib.sepaihrd_mh_destroy(mh)


def test_headline_batch_accept_traces_in_production_arithmetic(mm, oracle_py, synth400):
    """The acceptance contract of the arithmetic `bench.py`'s value is measured in, at the headline batch: the
    device-resident sampler in fma arithmetic, 4096 chains x 300 iterations with covariance refreshes, against the
    STRICT oracle's MetropolisHastingsSampler restatement chain by chain (MetropolisHastingsSampler.cpp:318-330).
    Expected mismatches: 0.  A likelihood that differs in the 9th digit flips an accept test whose uniform falls inside
    that gap (probability ~1e-9 x |log-likelihood| per test): the assertion allows none, and says how many if any."""
    from concurrent.futures import ThreadPoolExecutor
    pb = synth400.with_(arith=mm.ARITH_FMA, constraint_mode=1, solver=0)
    C, iters, burn, ap = 4096, 300, 100, 50
    from mmid_amd import draws
    x0 = draws.jitter_draws(pb, 1, C)
    kw = dict(iterations=iters, burn_in=burn, adaptation_period=ap, thinning=50)
    dev = mm.HostObjective(pb).metropolis_hastings(x0, seed=1000, device_state=True, **kw)
    orc = oracle_py.Oracle(pb.with_(arith=mm.ARITH_STRICT))

    def one(c):
        ref = orc.metropolis_hastings(x0[c], 1000 + c, iters, burn, adaptation_period=ap, thinning=50)
        return ref["accept_trace"], ref["accepted"]

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        refs = list(ex.map(one, range(C)))
    trace = np.stack([r[0] for r in refs])
    mismatches = int((trace != dev["accept_trace"]).sum())
    chains_off = int((trace != dev["accept_trace"]).any(axis=1).sum())
    assert mismatches == 0, f"{mismatches} accept decisions differ in {chains_off} of {C} chains"
    assert np.array_equal(dev["accepted"], np.array([r[1] for r in refs]))
    assert 0.02 < dev["accept_trace"].mean() < 0.9


def test_chain_summaries_gathered_over_two_groups_on_one_device(mm, shipped):
    """SURVEY 8(e) from the C++ host: optimizeChainGroupsOnDevice over two objectives, the per-chain summary records formed
    on the device ([P means | P variances | best value | accepted proposals] over the samples after burn-in) equal numpy
    on the returned samples, and gatherChainSummaries leaves the table of ALL chains on both groups' devices.  Two
    contexts on ONE device: the gather stages through the host (RCCL wants one rank per device) and says so; forcing
    RCCL is refused."""
    from mmid_amd import draws, hipabi
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    C, P = 11, pb.n_params
    x0 = draws.jitter_draws(pb, 7, C)
    objs = [mm.HostObjective(pb), mm.HostObjective(pb)]
    kw = dict(seed=5, iterations=121, burn_in=40, adaptation_period=30, thinning=10)
    out = mm.hostabi.metropolis_hastings_group_summaries(objs, x0, **kw)
    assert out["backend_used"] == hipabi.GATHER_HOST
    kept = out["samples"][:, 5:]                      # samples of iterations 50, 60, ... 120: after the burn-in of 40
    rec = out["records"]
    np.testing.assert_allclose(rec[:, :P], kept.mean(axis=1), rtol=1e-13)
    np.testing.assert_allclose(rec[:, P:2 * P], kept.var(axis=1, ddof=1), rtol=1e-9, atol=1e-30)
    assert np.array_equal(rec[:, 2 * P], out["best_value"]) and np.array_equal(rec[:, 2 * P + 1], out["accepted"])
    assert np.array_equal(out["gathered"][0], rec) and np.array_equal(out["gathered"][1], rec)
    one = mm.HostObjective(pb).metropolis_hastings(x0, device_state=True, **kw)     # same chains in one group
    assert np.array_equal(one["samples"], out["samples"])
    with pytest.raises(RuntimeError, match="one rank per device"):
        mm.hostabi.metropolis_hastings_group_summaries(objs, x0, backend=hipabi.GATHER_RCCL, **kw)


def test_rccl_allgather_entry_point_single_rank(mm, shipped):
    """The RCCL form of the exchange executed on the one device a box has: ncclCommInitAll over one device, ncclAllGather
    inside a group call, compaction -- a single rank, so the gathered table is the local one.  (More than one rank needs
    more than one device: test_rccl_allgather_over_two_devices below, skipped on one-GPU boxes.)"""
    import ctypes as C
    from mmid_amd import hipabi
    lib = hipabi.load_library()
    hip = mm.HipObjective(shipped)
    rows, width = 37, 2 * shipped.n_params + 2
    table = np.random.RandomState(1).normal(size=(rows, width))
    assert lib.sepaihrd_write_records(hip.ctx, 0, table.ctypes.data, table.size) == 0
    assert lib.sepaihrd_records_buffer(hip.ctx, 0, table.size)
    ctxs = (C.c_void_p * 1)(hip.ctx)
    nrows = np.array([rows], dtype=np.int32)
    used = C.c_int(-1)
    rc = lib.sepaihrd_allgather_records(ctxs, 1, nrows.ctypes.data, width, hipabi.GATHER_RCCL, C.byref(used))
    assert rc == 0, lib.sepaihrd_last_error(hip.ctx)
    assert used.value == hipabi.GATHER_RCCL
    back = np.empty_like(table)
    assert lib.sepaihrd_read_records(hip.ctx, 1, back.ctypes.data, back.size) == 0
    assert np.array_equal(back, table)


def test_rccl_allgather_over_two_devices(mm, shipped):
    """One context per device, ragged shares (5 + 3 rows): every device ends up with all 8 records in device order,
    through RCCL."""
    import ctypes as C
    import torch
    from mmid_amd import hipabi
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    lib = hipabi.load_library()
    hips = [mm.HipObjective(shipped, device=0), mm.HipObjective(shipped, device=1)]
    width = 2 * shipped.n_params + 2
    parts = [np.random.RandomState(k).normal(size=(r, width)) for k, r in enumerate((5, 3))]
    for h, t in zip(hips, parts):
        assert lib.sepaihrd_write_records(h.ctx, 0, t.ctypes.data, t.size) == 0
    ctxs = (C.c_void_p * 2)(*[h.ctx for h in hips])
    nrows = np.array([5, 3], dtype=np.int32)
    used = C.c_int(-1)
    assert lib.sepaihrd_allgather_records(ctxs, 2, nrows.ctypes.data, width, hipabi.GATHER_AUTO, C.byref(used)) == 0
    assert used.value == hipabi.GATHER_RCCL
    want = np.concatenate(parts)
    for h in hips:
        back = np.empty_like(want)
        assert lib.sepaihrd_read_records(h.ctx, 1, back.ctypes.data, back.size) == 0
        assert np.array_equal(back, want)


@pytest.mark.parametrize("problem", ["shipped", "wide"])
def test_streams_drawn_on_the_device_are_the_hosts(mm, oracle_py, shipped, problem):
    """optimizeChainsOnDevice with the chains' std::mt19937 streams on the device (mt19937 state and twist, generate_canonical,
    the polar method evaluated 64 attempts at a time, glibc's log written out: csrc/sepaihrd_rng.inc) against the same run
    with libstdc++ drawing on the host: every output is the same bits -- accept traces, samples, values, scales, final
    covariance.  1500 iterations per chain cross ~380 twists of the 624-word state; the 16-age problem (158 parameters:
    79 pairs, more than 64 attempts can deliver) takes several rounds of attempts per draw.  Chain 0 against the oracle."""
    pb = shipped
    iters, burn, ap = 1500, 300, 100
    if problem == "wide":
        pb = mm.widen_age_classes(shipped, 4)
        pb.times = pb.times[:40]
        pb = pb.with_(obs_H=pb.obs_H[:20], obs_ICU=pb.obs_ICU[:20], obs_D=pb.obs_D[:20])
        iters, burn, ap = 400, 50, 60
    pb = pb.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    from mmid_amd import draws
    x0 = draws.jitter_draws(pb, 3, 6)
    kw = dict(seed=4242, iterations=iters, burn_in=burn, adaptation_period=ap, thinning=25, device_state=True)
    dev = mm.HostObjective(pb).metropolis_hastings(x0, device_streams=True, **kw)
    host = mm.HostObjective(pb).metropolis_hastings(x0, device_streams=False, **kw)
    assert 0.02 < dev["accept_trace"].mean() < 0.9
    for k in ("accept_trace", "accepted", "best_value", "best", "final_scale", "samples", "sample_values", "final_cov"):
        assert np.array_equal(dev[k], host[k]), k
    if problem == "shipped":
        ref = oracle_py.Oracle(pb).metropolis_hastings(x0[0], 4242, iters, burn, adaptation_period=ap, thinning=25)
        assert np.array_equal(dev["accept_trace"][0], ref["accept_trace"]) and np.array_equal(dev["samples"][0], ref["samples"])


@pytest.mark.parametrize("widen", [1e5, 300.0, 40.0])
def test_scale_adaptation_on_the_device_through_its_rare_branches(mm, oracle_py, shipped, widen):
    """adaptGlobalScale (MetropolisHastingsSampler.cpp:104-152) on the device, pushed through the branches an ordinary run
    never takes: proposal sigmas widened so that nearly every proposal is rejected -- the aggressive shrink (rate < 0.02 with
    500 outcomes), the emergency shrink (rate < 0.001 with 1000) and the clamp at log-scale -6.9; with the milder widening
    the scale falls to the floor and the recovery rule (:146-148) can fire.  Every output equals the host-driven loop's bits,
    chain 0 equals the oracle's."""
    import math
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    pb.sigmas = {k: v * widen for k, v in pb.sigmas.items()}
    from mmid_amd import draws
    x0 = draws.jitter_draws(shipped, 9, 4)
    iters = 1700
    # burn-in = the whole run: the covariance stays the widened initial one, only the scale can answer
    kw = dict(seed=77, iterations=iters, burn_in=iters, adaptation_period=100, thinning=50, device_state=True)
    dev = mm.HostObjective(pb).metropolis_hastings(x0, device_streams=True, **kw)
    host = mm.HostObjective(pb).metropolis_hastings(x0, device_streams=False, **kw)
    for k in ("accept_trace", "accepted", "best_value", "best", "final_scale", "samples", "sample_values", "final_cov"):
        assert np.array_equal(dev[k], host[k]), k
    ref = oracle_py.Oracle(pb).metropolis_hastings(x0[0], 77, iters, iters, adaptation_period=100, thinning=50)
    assert np.array_equal(dev["accept_trace"][0], ref["accept_trace"])
    assert dev["final_scale"][0] == ref["final_scale"]
    if widen > 1e4:
        assert dev["accept_trace"][:, -1000:].mean() < 0.001        # the emergency branch's condition held at the end
        assert np.all(dev["final_scale"] == math.exp(-6.9))         # ... and the clamp
    else:
        print("final scales", dev["final_scale"], "acceptance over the last 1000", dev["accept_trace"][:, -1000:].mean(axis=1))


def test_scale_on_device_in_either_order_with_set_values(mm, shipped):
    """sepaihrd_mh_keep_scale_on_device before or after sepaihrd_mh_set_values: the value of sample 0 is the chain's current
    value either way; after the first iteration the call is refused (the accept window starts with the run)."""
    import ctypes as C
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=1)
    from mmid_amd import draws
    x0 = draws.jitter_draws(pb, 2, 3)
    hip = mm.HipObjective(pb)
    lib = hip.lib
    P = pb.n_params
    cov0 = np.diag(pb.sigma_array() ** 2 + 1e-6)
    vals = np.array([1.5, -2.5, 3.25])
    got = []
    for order in ("before", "after"):
        mh = mm.hipabi.mh_create(lib, hip.ctx, 3, 50, x0, cov0, thinning=5)
        assert mh
        if order == "before":
            assert lib.sepaihrd_mh_keep_scale_on_device(mh, 1, C.c_double(0.234), 0) == 0
        assert lib.sepaihrd_mh_set_values(mh, vals.ctypes.data) == 0
        if order == "after":
            assert lib.sepaihrd_mh_keep_scale_on_device(mh, 1, C.c_double(0.234), 0) == 0
        out = np.full((3, 1), np.nan)
        assert lib.sepaihrd_mh_read_sample_values(mh, 0, 1, out.ctypes.data) == 0
        got.append(out[:, 0].copy())
        lib.sepaihrd_mh_destroy(mh)
    assert np.array_equal(got[0], vals) and np.array_equal(got[1], vals)


def test_reference_constructor_argument_lists(mm, shipped, monkeypatch):
    """The drop-in at SEPAIHRDModelCalibration.cpp:84-118 is a change of two class names: the parameter manager and the
    objective are built with the reference's argument lists (shared_ptr<AgeSEPAIHRDModel> first,
    SEPAIHRDObjectiveFunction.hpp:49-58).  Same values as the struct-taking constructors in both constraint modes --
    with a HipSEPAIHRDParameterManager, and with an IParameterManager of another type whose mode is switched
    without telling the objective (what ModelCalibrator.cpp:62-64,88-90 does to the reference's own manager);
    updateModelParameters() writes into the model it was given."""
    rs = np.random.RandomState(4)
    lo, hi, _ = shipped.bounds_arrays()
    theta = lo + (hi - lo) * rs.uniform(-0.2, 1.2, (5, shipped.n_params))   # beyond the bounds: the mode matters
    theta[0] = shipped.base_theta
    theta[0, 3] = hi[3] + 0.3 * (hi[3] - lo[3])
    # these constructors have no room for the arithmetic: fma (what bench.py's `value` is measured in) unless the
    # environment says SEPAIHRD_ARITH=strict
    by_arith = {}
    for env, arith in ((None, mm.ARITH_FMA), ("strict", mm.ARITH_STRICT), ("fma", mm.ARITH_FMA)):
        monkeypatch.delenv("SEPAIHRD_ARITH", raising=False)
        if env:
            monkeypatch.setenv("SEPAIHRD_ARITH", env)
        assert mm.hostabi.default_arith() == arith
        pb = shipped.with_(arith=arith)
        got = mm.hostabi.reference_constructors(pb, theta)
        for mode in (0, 1):
            want, status = mm.HostObjective(pb.with_(constraint_mode=mode)).calculate_batch(theta)
            assert np.all(status <= 1)
            assert np.array_equal(got["values"][0, mode], want), (env, mode)
            assert np.array_equal(got["values"][1, mode], want), (env, mode)
        assert not np.array_equal(got["values"][0, 0], got["values"][0, 1])
        by_arith[env] = got["values"].copy()
    assert not np.array_equal(by_arith[None], by_arith["strict"]) and np.array_equal(by_arith[None], by_arith["fma"])
    np.testing.assert_allclose(by_arith[None], by_arith["strict"], rtol=1e-7)
    pb = shipped.with_(arith=mm.ARITH_STRICT)
    clamped = mm.HostObjective(pb, with_objective=False).apply_constraints(theta[0], 0)[0]
    assert np.array_equal(got["model_back"], clamped)


def test_device_accept_test_against_the_host_driven_step(mm, shipped):
    """sepaihrd_mh_step_tested (accept test, commit and next proposal on the device) against the reference's rule applied
    on the host to the same values, and against the host-driven entry point fed with that outcome: flags, the values
    compared, the committed history rows and the next proposals are the same bits.  Covers chains that take no uniform
    (log_ratio >= 0) and chains whose uniform decides either way."""
    import ctypes as C
    from mmid_amd import draws, hipabi
    pb = shipped.with_(arith=mm.ARITH_STRICT, constraint_mode=mm.CONSTRAINT_REFLECT)
    Cn, P = 48, pb.n_params
    lib = hipabi.load_library()
    vp = C.c_void_p
    lib.sepaihrd_mh_set_values.argtypes = [vp, vp]
    lib.sepaihrd_mh_test_buffer.restype = C.POINTER(C.c_double)
    lib.sepaihrd_mh_test_buffer.argtypes = [vp]
    lib.sepaihrd_mh_staging_buffer.restype = C.POINTER(C.c_double)
    lib.sepaihrd_mh_staging_buffer.argtypes = [vp]
    lib.sepaihrd_mh_stage_normals.argtypes = [vp, vp]
    lib.sepaihrd_mh_step.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_int]
    lib.sepaihrd_mh_step_tested.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    lib.sepaihrd_mh_fetch_test.argtypes = [vp, vp, vp]
    rng = np.random.default_rng(11)
    x0 = draws.jitter_draws(pb, 3, Cn)
    cov0 = np.diag((0.02 * np.maximum(np.abs(pb.base_theta), 1e-3)) ** 2) + 1e-6 * np.eye(P)
    z1 = rng.standard_normal((Cn, P))
    z2u = rng.standard_normal((Cn, P))
    z2p = rng.standard_normal((Cn, P))
    scale1 = np.full(Cn, 0.7)
    scale_rej, scale_acc = np.full(Cn, 0.5), np.full(Cn, 1.25)
    log_u = np.where(np.arange(Cn) % 3 == 0, -1e300, np.where(np.arange(Cn) % 3 == 1, 0.0, -0.5))

    def sampler():
        hip = mm.HipObjective(pb)
        mh = hipabi.mh_create(lib, hip.ctx, Cn, 8, x0, cov0)
        assert mh
        lp0, st0 = np.empty(Cn), np.empty(Cn, dtype=np.int32)
        assert lib.sepaihrd_mh_evaluate_current(mh, lp0.ctypes.data, st0.ctypes.data) == 0
        lp0 = np.where((st0 >= 2) | ~np.isfinite(lp0), -1e18, lp0)
        buf = np.ctypeslib.as_array(lib.sepaihrd_mh_staging_buffer(mh), shape=(Cn * P,))
        buf[:] = z1.ravel()
        assert lib.sepaihrd_mh_stage_normals(mh, buf.ctypes.data) == 0
        assert lib.sepaihrd_mh_step(mh, None, scale1.ctypes.data, None, None, 0, 0.1, 0) == 0
        ll1, st1 = np.empty(Cn), np.empty(Cn, dtype=np.int32)
        assert lib.sepaihrd_mh_fetch(mh, ll1.ctypes.data, st1.ctypes.data) == 0
        prop1 = np.empty((Cn, P))
        assert lib.sepaihrd_mh_read_proposal(mh, prop1.ctypes.data) == 0
        return hip, mh, lp0, ll1, st1, prop1

    # the reference's rule on the host
    hipA, mhA, lp0, ll1, st1, prop1 = sampler()
    v_ref = np.where((st1 >= 2) | ~np.isfinite(ll1), -1e18, ll1)
    ratio = v_ref - lp0
    no_u = ratio >= 0.0
    acc = no_u | (log_u < ratio)
    assert acc.any() and (~acc).any() and no_u.any() and (~no_u).any()
    flags_ref = acc.astype(np.uint8) | ((acc & (v_ref > lp0)).astype(np.uint8) << 1) | (no_u.astype(np.uint8) << 2)
    # A: the device's own test
    assert lib.sepaihrd_mh_set_values(mhA, lp0.ctypes.data) == 0
    tb = np.ctypeslib.as_array(lib.sepaihrd_mh_test_buffer(mhA), shape=(3 * Cn + Cn * P,))
    tb[:Cn], tb[Cn:2 * Cn], tb[2 * Cn:3 * Cn], tb[3 * Cn:] = log_u, scale_rej, scale_acc, z2p.ravel()
    buf = np.ctypeslib.as_array(lib.sepaihrd_mh_staging_buffer(mhA), shape=(Cn * P,))
    buf[:] = z2u.ravel()
    assert lib.sepaihrd_mh_stage_normals(mhA, buf.ctypes.data) == 0
    assert lib.sepaihrd_mh_step_tested(mhA, 0.1, 0, 0) == 0
    values, flags = np.empty(Cn), np.empty(Cn, dtype=np.uint8)
    assert lib.sepaihrd_mh_fetch_test(mhA, values.ctypes.data, flags.ctypes.data) == 0
    assert np.array_equal(values, v_ref) and np.array_equal(flags, flags_ref)
    propA = np.empty((Cn, P))
    assert lib.sepaihrd_mh_read_proposal(mhA, propA.ctypes.data) == 0
    rows = np.array([0, 1], dtype=np.int32)
    histA = np.empty((Cn, 2, P))
    assert lib.sepaihrd_mh_read_history(mhA, rows.ctypes.data, 2, histA.ctypes.data) == 0
    assert np.array_equal(histA[:, 1], np.where(acc[:, None], prop1, x0))
    # B: the host-driven step with that outcome
    hipB, mhB, lp0b, ll1b, st1b, prop1b = sampler()
    assert np.array_equal(ll1b, ll1) and np.array_equal(prop1b, prop1)
    buf = np.ctypeslib.as_array(lib.sepaihrd_mh_staging_buffer(mhB), shape=(Cn * P,))
    buf[:] = z2u.ravel()
    assert lib.sepaihrd_mh_stage_normals(mhB, buf.ctypes.data) == 0
    scale2 = np.where(acc, scale_acc, scale_rej)
    patch = np.nonzero(no_u)[0].astype(np.int32)
    accept_b = (flags_ref & 3).astype(np.uint8)
    assert lib.sepaihrd_mh_step(mhB, accept_b.ctypes.data, scale2.ctypes.data, patch.ctypes.data, z2p.ctypes.data, len(patch), 0.1, 0) == 0
    ll2 = np.empty(Cn)
    assert lib.sepaihrd_mh_fetch(mhB, ll2.ctypes.data, None) == 0
    propB = np.empty((Cn, P))
    assert lib.sepaihrd_mh_read_proposal(mhB, propB.ctypes.data) == 0
    assert np.array_equal(propA, propB)
    ll2a = np.empty(Cn)
    assert lib.sepaihrd_mh_fetch(mhA, ll2a.ctypes.data, None) == 0
    assert np.array_equal(ll2a, ll2)
    lib.sepaihrd_mh_destroy(mhA)
    lib.sepaihrd_mh_destroy(mhB)


def test_kernel_info_says_whether_the_phase_pass_was_applied(mm, synth400):
    """which build was measured.  Both arithmetic builds of the shipped library went through
    csrc/phase_pass.py (the CPU suite asserts there is no fall-back marker); the fp32-state kernel does not use it."""
    for arith in (mm.ARITH_FMA, mm.ARITH_STRICT):
        hip = mm.HipObjective(synth400.with_(arith=arith))
        for batch in (4096, 32768):
            assert hip.kernel_info(batch)["phase_pass_applied"] == 1, (arith, batch)
        hip.close()
    hip = mm.HipObjective(synth400.with_(arith=mm.ARITH_FMA, precision=mm.PRECISION_F32))
    assert hip.kernel_info(4096)["phase_pass_applied"] == 0
    hip.close()


def test_device_libm_selfcheck_and_the_fall_back_to_host_streams(mm, shipped, tmp_path, monkeypatch):
    """ADVICE r3 (medium) / VERDICT r3 weak 6: the device's log / exp are restatements of THIS image's libm.  The sampler checks
    that at run time (4096 fixed arguments, device against std::log / std::exp of the process) before it lets the device draw
    the chains' streams.  Here: the check passes on this box; when it is made to fail (SEPAIHRD_LIBM_SELFCHECK=fail: the test
    hook that stands for a host with another libm) the C entry points refuse, and the C++ sampler falls back to host-drawn
    streams, says so, sets the flag -- and produces the same chains, because host streams ARE the reference's."""
    import ctypes as C
    pb = shipped.with_(arith=mm.ARITH_FMA, constraint_mode=mm.CONSTRAINT_REFLECT)
    hip = mm.HipObjective(pb)
    assert hip.device_libm_check() == (0, 0)
    hip.close()
    x0 = mm.draws.jitter_draws(pb, 1, 24)
    kw = dict(adaptation_period=40, thinning=5, report_interval=100, checkpoint_chains=1)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    good = mm.HostObjective(pb).metropolis_hastings_reported(x0, 5, 300, 60, str(tmp_path / "a"), str(tmp_path / "a.log"), **kw)
    assert not good["fell_back"] and good["failures"] == [0, 0, 0]
    monkeypatch.setenv("SEPAIHRD_LIBM_SELFCHECK", "fail")
    hip = mm.HipObjective(pb)
    dl, de = hip.device_libm_check()
    assert dl >= 1 and de >= 1
    # the C ABI refuses to seed device streams on such a host
    lib = mm.hipabi.load_library()
    cfg = mm.hipabi.sepaihrd_mh_config(chains=4, iterations=10, thinning=1, adaptation_window=0, covariance_mode=0, reserved=0,
                                       reg_eps=1e-6, scaling_factor=2.38 ** 2 / pb.n_params)
    cov0 = np.ascontiguousarray(np.eye(pb.n_params) * 1e-4)
    x4 = np.ascontiguousarray(x0[:4])
    mh = lib.sepaihrd_mh_create(hip.ctx, C.byref(cfg), x4.ctypes.data, cov0.ctypes.data)
    assert mh
    assert lib.sepaihrd_mh_seed_streams(mh, 1) == -4            # SEPAIHRD_E_UNSUPPORTED
    assert b"libm" in lib.sepaihrd_last_error(hip.ctx)
    assert lib.sepaihrd_mh_keep_scale_on_device(mh, 1, C.c_double(0.234), 0) == -4
    lib.sepaihrd_mh_destroy(mh)
    hip.close()
    fell = mm.HostObjective(pb).metropolis_hastings_reported(x0, 5, 300, 60, str(tmp_path / "b"), str(tmp_path / "b.log"), **kw)
    assert fell["fell_back"]
    assert "libm" in (tmp_path / "b.log").read_text().splitlines()[0] and (tmp_path / "b.log").read_text().startswith("WARNING")
    assert np.array_equal(fell["samples"], good["samples"]) and np.array_equal(fell["sample_values"], good["sample_values"])
    # and the files of the two runs are the same bytes: reports and checkpoints do not depend on where the streams are drawn
    for name in ("posterior_trace_checkpoint.csv", "posterior_trace_final.csv", "posterior_trace.csv"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    strip = lambda text: [l for l in text.splitlines() if "libm" not in l]
    assert strip((tmp_path / "a.log").read_text()) == strip((tmp_path / "b.log").read_text())


def test_checkpoints_and_progress_lines_while_the_device_resident_sampler_runs(mm, shipped, tmp_path):
    """VERDICT r3 missing 3 / next 5 (MetropolisHastingsSampler.cpp:363-383,399-411,440-469): every report_interval iterations
    a progress line and posterior_trace_checkpoint.csv (the chain's last <= 5000 thinned samples), at the end
    posterior_trace_final.csv and posterior_trace.csv -- from a run whose iterations are queued ahead of the device and which
    does not stop for any of it.  A watcher thread reads the checkpoint file WHILE the run is going (nothing is killed): every
    version it sees is a prefix of the final trace, line for line; header and number format are the reference's; the first
    two chains report; the host-state loop writes the same bytes."""
    import json
    import threading
    import time
    pb = shipped.with_(arith=mm.ARITH_FMA, constraint_mode=mm.CONSTRAINT_REFLECT)
    Cn, iters, thin, every = 512, 2400, 4, 200
    x0 = mm.draws.jitter_draws(pb, 1, Cn)
    out = tmp_path / "dev"
    out.mkdir()
    seen, stop = [], threading.Event()

    def watch():
        last = None
        path = out / "posterior_trace_checkpoint.csv"
        while not stop.is_set():
            try:
                st = path.stat()
                key = (st.st_mtime_ns, st.st_size)
                if key != last:
                    seen.append((time.perf_counter(), path.read_text()))
                    last = key
            except FileNotFoundError:
                pass
            time.sleep(0.001)

    th = threading.Thread(target=watch, daemon=True)
    th.start()
    t0 = time.perf_counter()
    host = mm.HostObjective(pb)
    r = host.metropolis_hastings_reported(x0, 9, iters, 300, str(out), str(tmp_path / "dev.log"), adaptation_period=100, thinning=thin,
                                          report_interval=every, checkpoint_chains=2)
    t1 = time.perf_counter()
    stop.set()
    th.join()
    assert not r["fell_back"] and r["failures"] == [0, 0, 0]
    names = list(pb.param_names)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_output_headers.json")) as fh:
        fmt = json.load(fh)["posterior_trace"]
    final = (out / "posterior_trace_final.csv").read_text().splitlines()
    assert final[0].split(",") == fmt["header"][:2] + names
    n_s = 1 + (iters - 1) // thin
    assert len(final) == 1 + n_s
    for i in (0, 1, n_s - 1):    # iter as integer, every other field std::scientific << setprecision(6)
        cells = final[1 + i].split(",")
        assert cells[0] == str(i) and cells[1] == "%.6e" % r["sample_values"][0, i]
        assert cells[2:] == ["%.6e" % v for v in r["samples"][0, i]]
    assert (out / "posterior_trace.csv").read_text().splitlines() == final
    # chain 1 reports too, under its own names
    final1 = (out / "posterior_trace_final_chain1.csv").read_text().splitlines()
    assert final1[1 + 7].split(",")[2:] == ["%.6e" % v for v in r["samples"][1, 7]]
    # what the watcher saw while the run was going: several versions, each a prefix of the final trace
    during = [(t, text) for t, text in seen if t < t1]
    assert len(during) >= 3, (len(seen), t1 - t0)
    sizes = []
    for _, text in seen:
        lines = text.splitlines()
        assert lines[0] == final[0]
        first = int(lines[1].split(",")[0])
        assert lines[1:] == final[1 + first:1 + first + len(lines) - 1]
        sizes.append(first + len(lines) - 1)
    assert sizes == sorted(sizes) and sizes[-1] == (iters // every * every - 1) // thin + 1   # samples stored up to the last report
    # the progress lines: one per report and chain, the reference's layout, values of THAT iteration
    log = (tmp_path / "dev.log").read_text().splitlines()
    lines0 = [l for l in log if l.startswith("INFO Iter:")]
    lines1 = [l for l in log if l.startswith("INFO [chain 1] Iter:")]
    assert len(lines0) == len(lines1) == iters // every
    import re
    pat = re.compile(r"INFO Iter: +(\d+) \| LogPost: (-?[\d.]+) \| Best: (-?[\d.]+) \| AccRate: ([\d.]+)% \| Scale: ([\d.]+)$")
    for k, line in enumerate(lines0):
        m = pat.match(line)
        assert m and int(m.group(1)) == (k + 1) * every, line
        t = (k + 1) * every - 1                                  # the iteration reported; its state is sample t / thin if stored
        if t % thin == 0:
            assert m.group(2) == "%.2f" % r["sample_values"][0, t // thin]
        assert float(m.group(3)) >= float(m.group(2)) - 0.006
    # the host-state loop (host libstdc++ streams, same chains) writes the same bytes
    out2 = tmp_path / "host"
    out2.mkdir()
    r2 = host.metropolis_hastings_reported(x0[:3], 9, 420, 100, str(out2), str(tmp_path / "host.log"), adaptation_period=50, thinning=thin,
                                           report_interval=100, checkpoint_chains=2, device_state=False)
    out3 = tmp_path / "dev3"
    out3.mkdir()
    r3 = host.metropolis_hastings_reported(x0[:3], 9, 420, 100, str(out3), str(tmp_path / "dev3.log"), adaptation_period=50, thinning=thin,
                                           report_interval=100, checkpoint_chains=2, device_state=True)
    assert np.array_equal(r2["samples"], r3["samples"])
    for name in ("posterior_trace_checkpoint.csv", "posterior_trace_final.csv", "posterior_trace.csv", "posterior_trace_checkpoint_chain1.csv"):
        assert (out2 / name).read_bytes() == (out3 / name).read_bytes(), name
    assert (tmp_path / "host.log").read_text().replace(str(out2), "<dir>") == (tmp_path / "dev3.log").read_text().replace(str(out3), "<dir>")


def test_draws_queued_behind_the_evaluation_give_the_overlapped_result(mm, shipped, monkeypatch):
    """The draws of the next accept test run beside the evaluation on the copy stream, except for batches that fill the chip
    with two integrator waves per SIMD, where they queue behind it on the main stream (csrc/sepaihrd_mh_capi.cpp
    mh_draws_behind_the_evaluation); beside the evaluation they are followed by L z of both continuations (mh_lz_kernel), which
    the fused test + commit + proposal launch then takes instead of reading the factor itself.  Where the kernels are
    launched changes nothing they compute: the same run with either placement forced, and with the look-ahead product on or
    off, gives the same accept traces, samples and final state, including over covariance refreshes."""
    pb = shipped.with_(arith=mm.ARITH_FMA, constraint_mode=1)
    from mmid_amd import draws
    x0 = draws.jitter_draws(pb, 4, 21)
    kw = dict(seed=5, iterations=260, burn_in=60, adaptation_period=100, thinning=10, device_state=True, device_streams=True)
    out = {}
    for mode, lz in (("overlap", "ahead"), ("overlap", "fused"), ("serial", "ahead")):
        monkeypatch.setenv("SEPAIHRD_MH_DRAW", mode)
        monkeypatch.setenv("SEPAIHRD_MH_LZ", lz)
        out[(mode, lz)] = mm.HostObjective(pb).metropolis_hastings(x0, **kw)
    monkeypatch.delenv("SEPAIHRD_MH_DRAW")
    monkeypatch.delenv("SEPAIHRD_MH_LZ")
    ref = out[("overlap", "fused")]
    for key, r in out.items():
        for k in ("accept_trace", "accepted", "best_value", "best", "final_scale", "samples", "sample_values", "final_cov"):
            assert np.array_equal(r[k], ref[k]), (key, k)
    assert 0 < ref["accept_trace"].mean() < 1


def test_forms_that_serve_one_wave_per_simd_cannot_be_paired_on_a_simd(mm, synth400):
    """Up to 1024 one-wave workgroups a batch means at most one integrator wave per SIMD -- but only if two of them do not FIT a
    SIMD: behind any kernel that touched tens of MB the workgroup dispatcher pairs up what fits while other SIMDs stay empty
    (round 4: 16 384 chains 0.95 -> 1.46 ms; tools/probe_dispatch_placement.py, profiles/r04_dispatch_placement_probe.txt).
    The forms launched for such batches therefore allocate more than half a SIMD's 512 registers (the inline Dopri5 kernel needs
    them; the others declare an accumulation register they never touch), from 1025 workgroups on the two-wave sibling takes
    over, and the 16-lane form asks for half a CU's LDS (one workgroup per CU)."""
    for solver in (mm.SOLVER_DOPRI5, mm.SOLVER_CASH_KARP54):
        hip = mm.HipObjective(synth400.with_(arith=mm.ARITH_FMA, solver=solver))
        for batch in (6000, 8192, 12288, 16384):        # 375 .. 1024 one-wave workgroups
            info = hip.kernel_info(batch)
            assert info["lanes_per_chain"] == 4 and info["vgprs"] > 256, (solver, batch, info)
        info = hip.kernel_info(16384)
        if solver == mm.SOLVER_DOPRI5:
            assert info["likelihood_form"] == 0, info          # inline: nothing parked between half and one wave per SIMD
        for batch in (16400, 24576, 32768):              # some SIMD has to hold two waves: the two-wave form, which shares by design
            info = hip.kernel_info(batch)
            assert info["vgprs"] <= 256 and info["max_blocks_per_cu"] >= 8 and info["likelihood_form"] == 0, (solver, batch, info)
        info = hip.kernel_info(4096)                     # the 16-lane form: one 8-wave workgroup per CU
        assert info["lanes_per_chain"] == 16 and info["max_blocks_per_cu"] == 1 and info["lds_bytes"] >= 80 * 1024, info
        hip.close()
