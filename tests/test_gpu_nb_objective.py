"""The negative-binomial observation model of the deterministic objective on the device: the pass against
the host twin applied to the call's own trajectory and against the Python likelihood over the CPU oracle's trajectories, the
integrator forms and lane counts, mixed and absent dispersion against the Poisson run bit for bit, the statuses, the callers
that go through the context (device-resident sampler, finite-difference gradients), the lgamma probe, and the recovery of a
known dispersion.  Small shapes: the 30-day reference fixture, 5 chains (ragged in every layout), a distinct k per chain."""
import numpy as np
import pytest

from nb_objective_cases import DISPERSION_BOUNDS, INF, increments, lgamma_grid, observation_grid, python_reference, with_dispersion

pytestmark = pytest.mark.gpu

K_H = np.array([0.07, 0.9, 5.0, 37.0, 180.0])   # the calibrated dispersion of the five chains


def thetas(pb_plain, B=5, seed=5):
    rs = np.random.RandomState(seed)
    lo, hi, _ = pb_plain.bounds_arrays()
    theta = lo + (hi - lo) * rs.uniform(0, 1, (B, pb_plain.n_params))
    theta[0] = pb_plain.base_theta
    return theta


def twin_of(mm, pb_plain, got, k):
    """the host twin over the increments differenced from the call's own trajectory"""
    return mm.hostabi.nb_objective(increments(got["traj"], pb_plain.n), *observation_grid(pb_plain), k)


def dispersed_run(mm, pb_plain, theta_plain, k_H, fixed, form=None, want_traj=True):
    pb = with_dispersion(pb_plain, ("dispersion_H",), fixed=fixed)
    hip = mm.HipObjective(pb)
    if form is not None:
        hip.set_integrator_form(form)
    got = hip.eval_batch(np.column_stack([theta_plain, k_H]), want_traj=want_traj)
    k = np.column_stack([k_H, np.full(len(k_H), fixed[1]), np.full(len(k_H), fixed[2])])
    return hip, got, k


# ---- 1. the pass against the twin and against the oracle-based reference
@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_pass_matches_the_twin_and_the_oracle_reference(mm, oracle_py, ref_fixture, arith):
    """loglik and ll_parts against the twin over the call's own trajectory at rtol 1e-10 (the strict Poisson bar of
    tests/test_gpu_parity.py: the one operation not shared is log_pos against std::log); in strict also against the Python
    likelihood over the oracle's trajectories at rtol 1e-8."""
    pb = ref_fixture.with_(arith=mm.ARITH_STRICT if arith == "strict" else mm.ARITH_FMA)
    theta = thetas(pb)
    hip, got, k = dispersed_run(mm, pb, theta, K_H, (INF, INF, 3.0))
    assert np.isnan(hip.get_dispersion()[0]) and hip.get_dispersion()[1:].tolist() == [INF, 3.0]
    assert (got["status"] == 0).all()
    twin = twin_of(mm, pb, got, k)
    print(arith, "loglik", got["loglik"], "largest relative difference from the twin",
          np.max(np.abs(got["loglik"] - twin["loglik"]) / np.abs(twin["loglik"])))
    np.testing.assert_allclose(got["loglik"], twin["loglik"], rtol=1e-10)
    np.testing.assert_allclose(got["ll_parts"], twin["ll_parts"], rtol=1e-10)
    again = hip.eval_batch(np.column_stack([theta, K_H]))   # the launch without a trajectory: the same bits
    assert np.array_equal(again["loglik"], got["loglik"]) and np.array_equal(again["ll_parts"], got["ll_parts"])
    if arith == "strict":
        ref = oracle_py.Oracle(pb).eval_batch(theta, want_traj=True)
        assert np.array_equal(got["n_accept"], ref["n_accept"]) and np.array_equal(got["n_reject"], ref["n_reject"])
        ll, parts = python_reference(increments(ref["traj"], pb.n), observation_grid(pb), k)
        np.testing.assert_allclose(got["loglik"], ll, rtol=1e-8)
        np.testing.assert_allclose(got["ll_parts"], parts, rtol=1e-8)


# ---- 2. forms and lane counts
@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_sixteen_lane_form_and_lane_per_age_form_give_the_same_bits(mm, ref_fixture, arith):
    pb = ref_fixture.with_(arith=mm.ARITH_STRICT if arith == "strict" else mm.ARITH_FMA)
    theta = thetas(pb)
    _, quad, _ = dispersed_run(mm, pb, theta, K_H, (INF, 11.0, 3.0), form=mm.hipabi.FORM_QUAD, want_traj=False)
    _, lane, _ = dispersed_run(mm, pb, theta, K_H, (INF, 11.0, 3.0), form=mm.hipabi.FORM_LANE_PER_AGE, want_traj=False)
    for key in ("loglik", "ll_parts", "status", "n_accept", "n_reject"):
        assert np.array_equal(quad[key], lane[key]), key
    assert (quad["status"] == 0).all()


@pytest.mark.parametrize("n_age,solver", [(1, 0), (3, 2), (3, 1), (16, 0)])
def test_other_lane_counts_and_solvers(mm, ref_fixture, n_age, solver):
    """n = 1, 3 (pads a lane) and 16, Cash-Karp and Fehlberg 7(8) once each: the pass against the twin over the call's own
    trajectory (the new pass has one form for every batch size: no serial-walk branch to cover)"""
    pb = {1: lambda: mm.restrict_age_classes(ref_fixture, [0]), 3: lambda: mm.restrict_age_classes(ref_fixture, [0, 1, 2]),
          16: lambda: mm.widen_age_classes(ref_fixture, 4)}[n_age]()
    pb = pb.with_(solver=solver, arith=mm.ARITH_STRICT)
    theta = thetas(pb)
    _, got, k = dispersed_run(mm, pb, theta, K_H, (INF, 0.4, 60.0))
    assert (got["status"] == 0).all()
    twin = twin_of(mm, pb, got, k)
    np.testing.assert_allclose(got["loglik"], twin["loglik"], rtol=1e-10)
    np.testing.assert_allclose(got["ll_parts"], twin["ll_parts"], rtol=1e-10)


# ---- 3. mixed and absent dispersion against the Poisson run
@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_poisson_series_and_undispersed_context_keep_the_poisson_bits(mm, ref_fixture, arith):
    pb = ref_fixture.with_(arith=mm.ARITH_STRICT if arith == "strict" else mm.ARITH_FMA)
    theta = thetas(pb)
    plain_hip = mm.HipObjective(pb)
    plain = plain_hip.eval_batch(theta)
    plain_info = plain_hip.kernel_info(len(theta))
    assert "nb_ll" not in plain_info["kernel_name"]
    hip = mm.HipObjective(pb)
    hip.set_dispersion((4.0, INF, 0.8))
    mixed = hip.eval_batch(theta)
    assert np.array_equal(mixed["ll_parts"][:, 1], plain["ll_parts"][:, 1])
    assert not np.array_equal(mixed["ll_parts"][:, 0], plain["ll_parts"][:, 0])
    assert np.array_equal(mixed["n_accept"], plain["n_accept"]) and np.array_equal(mixed["n_reject"], plain["n_reject"])
    info = hip.kernel_info(len(theta))
    assert "sepaihrd_nb_ll_rows_kernel" in info["kernel_name"] and info["likelihood_form"] == 1 and info["scratch_bytes"] == 0
    hip.set_dispersion((INF, INF, INF))
    back = hip.eval_batch(theta)
    for key in ("loglik", "ll_parts", "status", "n_accept", "n_reject"):
        assert np.array_equal(back[key], plain[key]), key
    info = hip.kernel_info(len(theta))
    for key in ("kernel_name", "vgprs", "lds_bytes", "likelihood_form", "lanes_per_chain"):
        assert info[key] == plain_info[key], key
    with pytest.raises(ValueError, match=r"dispersion\[2\] \(k_D\) = 0 is not positive"):
        hip.set_dispersion((1.0, 1.0, 0.0))
    # the fp32-state arm has no parked increments: a dispersed context is refused, an undispersed one runs
    hip.set_precision(mm.PRECISION_F32)
    hip.eval_batch(theta)
    hip.set_dispersion((4.0, INF, INF))
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        hip.eval_batch(theta)


# ---- 4. statuses
def test_statuses_and_skipped_observations(mm, oracle_py, ref_fixture):
    theta = thetas(ref_fixture)
    pb = ref_fixture.with_(arith=mm.ARITH_STRICT)
    pb.bounds = dict(pb.bounds)
    pb.bounds["kappa_2"] = (-1.0, 1.5)
    theta[1, pb.param_names.index("kappa_2")] = -0.5      # a negative kappa: invalid theta
    theta[3, pb.param_names.index("kappa_2")] = -0.25
    ref = oracle_py.Oracle(pb).eval_batch(theta)
    _, got, _ = dispersed_run(mm, pb, theta, K_H, (INF, 9.0, 3.0), want_traj=False)
    assert got["status"].tolist() == ref["status"].tolist() == [0, 1, 0, 1, 0]
    assert (got["loglik"][[1, 3]] == mm.LOWEST).all() and np.isfinite(got["loglik"][[0, 2, 4]]).all()
    assert (got["ll_parts"][[1, 3]] == 0.0).all()
    # a dispersion entry that is NaN: the cells are NaN, the total fails the finiteness check
    kk = K_H.copy()
    kk[2] = np.nan
    _, got_nan, _ = dispersed_run(mm, pb, theta, kk, (INF, 9.0, 3.0), want_traj=False)
    assert got_nan["status"].tolist() == [0, 1, 1, 1, 0] and got_nan["loglik"][2] == mm.LOWEST
    assert got_nan["loglik"][0] == got["loglik"][0] and got_nan["loglik"][4] == got["loglik"][4]
    # the step budget
    tight = ref_fixture.with_(abs_err=0.0, rel_err=1e-300, max_attempts=3000, arith=mm.ARITH_STRICT)
    _, got3, _ = dispersed_run(mm, tight, np.tile(tight.base_theta, (3, 1)), K_H[:3], (INF, 9.0, 3.0), want_traj=False)
    assert got3["status"].tolist() == [3, 3, 3] and (got3["loglik"] == mm.LOWEST).all()
    # NaN and negative observations are skipped
    holes = ref_fixture.with_(arith=mm.ARITH_STRICT)
    holes.obs_H = holes.obs_H.copy()
    holes.obs_D = holes.obs_D.copy()
    holes.obs_H[3, 1], holes.obs_H[7, 2], holes.obs_D[11, 0] = np.nan, -1.0, np.nan
    th = thetas(holes)
    _, goth, k = dispersed_run(mm, holes, th, K_H, (INF, INF, 3.0))
    twin = twin_of(mm, holes, goth, k)
    assert (goth["status"] == 0).all()
    np.testing.assert_allclose(goth["ll_parts"], twin["ll_parts"], rtol=1e-10)


# ---- 5. the callers that go through the context
def test_sampler_and_gradient_go_through_the_pass(mm, ref_fixture):
    lib = mm.hipabi.load_library()
    pb = with_dispersion(ref_fixture.with_(arith=mm.ARITH_STRICT), ("dispersion_H",), fixed=(INF, INF, 3.0))
    P, Cn = pb.n_params, 4
    x0 = np.column_stack([thetas(ref_fixture, Cn), K_H[:Cn]])
    hip = mm.HipObjective(pb)
    direct = hip.eval_batch(x0)
    mh = mm.hipabi.mh_create(lib, hip.ctx, Cn, 4, x0, 1e-4 * np.eye(P))
    assert mh
    try:
        lp0, st0 = np.empty(Cn), np.empty(Cn, dtype=np.int32)
        assert lib.sepaihrd_mh_evaluate_current(mh, lp0.ctypes.data, st0.ctypes.data) == 0
        assert np.array_equal(lp0, direct["loglik"]) and np.array_equal(st0, direct["status"])
        z = np.random.RandomState(2).standard_normal((Cn, P))
        z[:, -1] = [40000.0, -40000.0, 3.0e6, -0.5]     # far outside the bounds of the dispersion: the reflect rule acts
        scale = np.ones(Cn)
        lp, st = np.empty(Cn), np.empty(Cn, dtype=np.int32)
        assert lib.sepaihrd_mh_propose(mh, z.ctypes.data, scale.ctypes.data, lp.ctypes.data, st.ctypes.data) == 0
        prop = np.empty((Cn, P))
        assert lib.sepaihrd_mh_read_proposal(mh, prop.ctypes.data) == 0
    finally:
        lib.sepaihrd_mh_destroy(mh)
    assert ((prop[:, -1] >= DISPERSION_BOUNDS[0]) & (prop[:, -1] <= DISPERSION_BOUNDS[1])).all()
    assert not np.allclose(prop[:3, -1], x0[:3, -1])
    at_prop = hip.eval_batch(prop)
    assert np.array_equal(lp, at_prop["loglik"]) and np.array_equal(st, at_prop["status"])
    # finite-difference gradients: the centre values are eval_batch's, the perturbed context has the same observation model
    g = hip.fd_gradient_batch(x0)
    assert np.array_equal(g["value"], direct["loglik"])
    other = hip.fd_perturbed_objective()
    assert np.isnan(other.get_dispersion()[0]) and other.get_dispersion()[1:].tolist() == [INF, 3.0]
    eps = 1e-4 * np.maximum(np.abs(x0[:, -1]), 1e-4)
    plus = x0.copy()
    plus[:, -1] += eps
    f_plus = other.eval_batch(plus)["loglik"]
    assert np.array_equal(g["grad"][:, -1], (f_plus - g["value"]) / eps)
    assert (g["grad"][:, -1] != 0.0).all()


def test_host_adapter_maps_the_names_and_sets_the_dispersion(mm, ref_fixture):
    """HipSEPAIHRDParameterManager resolves dispersion_H, HipSEPAIHRDObjectiveFunction::setDispersion fixes the others: the C++
    objective and its gradient objective give the values of the context driven directly, bit for bit"""
    plain = ref_fixture.with_(arith=mm.ARITH_STRICT, constraint_mode=mm.CONSTRAINT_CLAMP)
    pb = with_dispersion(plain, ("dispersion_H",), fixed=(INF, INF, 3.0))
    theta = np.column_stack([thetas(plain), K_H])
    hip = mm.HipObjective(pb)
    direct = hip.eval_batch(theta)
    host = mm.HostObjective(pb)
    assert host.current_parameters()[-1] == DISPERSION_BOUNDS[1]
    values, status = host.calculate_batch(theta)
    assert np.array_equal(values, direct["loglik"]) and np.array_equal(status, direct["status"])
    value, grad = host.evaluate_with_gradient(theta[2])
    g = hip.fd_gradient_batch(theta[2:3])
    assert value == direct["loglik"][2] == g["value"][0] and np.array_equal(grad, g["grad"][0]) and grad[-1] != 0.0
    # a fixed k set after construction
    host2, hip2 = mm.HostObjective(plain), mm.HipObjective(plain)
    before, _ = host2.calculate_batch(theta[:, :-1])
    host2.set_dispersion((4.0, INF, 0.8))
    hip2.set_dispersion((4.0, INF, 0.8))
    after, _ = host2.calculate_batch(theta[:, :-1])   # the same thetas: the cache was cleared with the old model's values
    assert np.array_equal(after, hip2.eval_batch(theta[:, :-1])["loglik"]) and not np.array_equal(after, before)
    with pytest.raises(RuntimeError, match=r"dispersion\[0\] \(k_H\) = -1 is not positive"):
        host2.set_dispersion((-1.0, INF, INF))


# ---- 6. the lgamma probe
def test_device_lgamma_has_the_hosts_bits(mm, ref_fixture):
    x = lgamma_grid()[::42]   # about 1e4 of the CPU test's arguments
    got = mm.HipObjective(ref_fixture).lgamma_device(x)
    assert np.array_equal(got, mm.hostabi.lgamma_pos(x))


# ---- 7. dispersion recovery
RECOVERY_SEED = 7


def recovery_case(pb, mean_inc, seed=RECOVERY_SEED, k_true=5.0):
    """observations drawn as negative binomial with size k_true around the mean increments (gamma-Poisson mixture)"""
    rs = np.random.RandomState(seed)
    obs = []
    for s in range(3):
        mu = np.maximum(mean_inc[:, s, :], 0.0) + 1e-10
        obs.append(rs.poisson(rs.gamma(k_true, mu / k_true)).astype(float))
    return obs


def test_dispersion_recovery(mm, oracle_py, ref_fixture):
    """64 chains that differ only in k on a log grid from 0.1 to 1000 (one k for the three series): the argmax of the likelihood
    is one of the two grid points nearest the k = 5 the observations were drawn with.  The seed was chosen on the CPU, where the
    Python likelihood over the oracle's increments alone meets the condition (it does for nine of the seeds 0 .. 9, all but 6)."""
    base = ref_fixture.with_(arith=mm.ARITH_STRICT)
    mean_inc = increments(oracle_py.Oracle(base).eval_batch(base.base_theta[None, :], want_traj=True)["traj"], base.n)[0]
    obs = recovery_case(base, mean_inc)
    pb_obs = base.with_(obs_H=obs[0], obs_ICU=obs[1], obs_D=obs[2])
    grid = np.logspace(-1, 3, 64)
    nearest = set(np.argsort(np.abs(np.log(grid) - np.log(5.0)))[:2].tolist())
    ll_py, _ = python_reference(np.tile(mean_inc, (64, 1, 1, 1)), observation_grid(pb_obs), np.tile(grid[:, None], (1, 3)))
    assert int(np.argmax(ll_py)) in nearest
    pb = with_dispersion(pb_obs, ("dispersion_H", "dispersion_ICU", "dispersion_D"), bounds=(0.1, 1000.0))
    theta = np.column_stack([np.tile(base.base_theta, (64, 1)), grid, grid, grid])
    got = mm.HipObjective(pb).eval_batch(theta)
    assert (got["status"] == 0).all()
    assert int(np.argmax(got["loglik"])) in nearest, (grid[int(np.argmax(got["loglik"]))], grid[sorted(nearest)])
    np.testing.assert_allclose(got["loglik"], ll_py, rtol=1e-8)
