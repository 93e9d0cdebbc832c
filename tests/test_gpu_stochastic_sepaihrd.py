"""Stochastic chain-binomial SEPAIHRD ensembles on the device (sepaihrd_ensemble_stochastic) against the host twin, bit for
bit: the twin is fed the device's own model values and status and the problem's fixed data."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
SEED = 0x1234_5678_9ABC_DEF0  # both words of the key in use
MULT = ["E0_multiplier", "P0_multiplier", "A0_multiplier", "I0_multiplier", "H0_multiplier", "ICU0_multiplier", "R0_multiplier", "D0_multiplier"]
INIT_FROM_THETA, INIT_FIXED = 0, 1


def problem(mm, ref_fixture, n=4, T=6):
    """the reference fixture cut to T output times, the eight initial-state multipliers calibrated, n age classes"""
    pb = ref_fixture.with_(times=ref_fixture.times[:T], obs_H=ref_fixture.obs_H[:T], obs_ICU=ref_fixture.obs_ICU[:T], obs_D=ref_fixture.obs_D[:T],
                           param_names=list(ref_fixture.param_names) + MULT,
                           sigmas={**ref_fixture.sigmas, **{k: 0.05 for k in MULT}},
                           bounds={**ref_fixture.bounds, **{k: (0.0, 1e7) for k in MULT}},
                           base_theta=np.concatenate([ref_fixture.base_theta, np.ones(8)]))
    if n < 4:
        pb = mm.problem.restrict_age_classes(pb, list(range(n)))
    elif n == 16:
        pb = mm.problem.widen_age_classes(pb, 4)
    elif n != 4:
        pb = mm.problem.restrict_age_classes(mm.problem.widen_age_classes(pb, 5), list(range(n)))
    return pb


def six_thetas(mm, pb):
    th = mm.draws.jitter_draws(pb, 11, 6)
    th[0] = pb.base_theta
    th[2, 0] = 5.0     # beta beyond its upper bound: clamped onto it
    th[3, 5] = 1e6     # E0 multiplier: E(0) exceeds the population, the initial-state rule rejects the sample
    th[4, 5:] = 1e-3   # every multiplier tiny: all compartments but S round to 0 or 1
    return th


def objective(mm, pb, mode=INIT_FROM_THETA, arith=None):
    hip = mm.HipObjective(pb.with_(arith=mm.ARITH_STRICT if arith is None else arith))
    hip.set_initial_state_mode(mode)
    return hip


def twin_of(mm, pb, got, R, m, keep, seed=SEED, probs=PROBS):
    return mm.hostabi.stochastic_from_values(got["model_values"], got["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, R, m, seed, probs,
                                             beta_end_times=pb.beta_end_times, keep=keep)


def check_against_twin(mm, pb, got, R, m, keep, **kw):
    twin = twin_of(mm, pb, got, R, m, keep, **kw)
    assert got["n_valid"] == twin["n_valid"] == int(np.sum(got["status"] == 0))
    for key in ("quantiles", "extinct", "final_state") + (("traj",) if keep > 0 else ()):
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    return twin


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_device_equals_twin(mm, ref_fixture, n, m):
    pb = problem(mm, ref_fixture, n)
    hip = objective(mm, pb)
    theta = six_thetas(mm, pb)
    for R in (1, 63, 64, 65, 200):
        got = hip.ensemble_stochastic(theta, R, m, SEED, PROBS, keep=R, want_values=True, want_final=True)
        assert list(got["status"]) == [0, 0, 0, 1, 0, 0] and got["n_valid"] == 5
        assert np.isnan(got["traj"][3]).all() and np.isnan(got["final_state"][3]).all() and np.isnan(got["extinct"][3])
        assert np.isfinite(got["traj"][[0, 1, 2, 4, 5]]).all() and np.isfinite(got["quantiles"]).all()
        check_against_twin(mm, pb, got, R, m, keep=R)
        tr = got["traj"]
        assert (tr[4, :, 0, 1:9] <= 1).all() and (tr[4, :, 0, 0] > 0).all()  # the tiny multipliers: next to nobody outside S
        assert np.array_equal(tr[:, :, -1], got["final_state"], equal_nan=True)
    assert (np.diff(tr[0, :, :, 0], axis=1) < 0).any()  # infections happen


def test_a_compartment_near_the_int32_limit(mm, ref_fixture):
    """N of the first age class scaled so that S(0) sits just below 2^31 - 1: the infection draw has n p far above 10, the
    rejection sampler's regime, at the largest n the sampler takes."""
    pb = problem(mm, ref_fixture)
    pb = pb.with_(N=np.array([2147483600.0, 4e6, 2e6, 1e6]))
    hip = objective(mm, pb)
    theta = six_thetas(mm, pb)
    theta[:, 0] = np.maximum(theta[:, 0], 0.2)
    got = hip.ensemble_stochastic(theta, 65, 3, SEED, PROBS, keep=65, want_values=True, want_final=True)
    S0 = got["traj"][0, 0, 0, 0, 0]
    assert 2147483647 - 1000 < S0 <= 2147483647 and got["n_valid"] == 5
    new = got["traj"][0, :, 0, 0, 0] - got["traj"][0, :, 1, 0, 0]
    assert new.min() > 100  # n p >= 10 by a wide margin
    check_against_twin(mm, pb, got, 65, 3, keep=65)
    # one unit more and the rounded S(0) leaves int32: every sample is invalid
    over = objective(mm, pb.with_(N=np.array([2147483648.0 + 200.0, 4e6, 2e6, 1e6])))
    bad = over.ensemble_stochastic(theta, 2, 1, SEED, PROBS)
    assert (bad["status"] == 1).all() and bad["n_valid"] == 0 and np.isnan(bad["quantiles"]).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_model_values_are_the_parameter_managers(mm, ref_fixture, mode):
    pb = problem(mm, ref_fixture)
    theta = six_thetas(mm, pb)
    theta[1, 1] = -0.3   # theta below its lower bound
    theta[5, 2] = 1.9    # kappa_1 above its upper bound
    host = mm.hostabi.HostObjective(pb, with_objective=False)
    n = pb.n
    for init_mode in (INIT_FROM_THETA, INIT_FIXED):
        hip = objective(mm, pb, init_mode)
        hip.set_constraint_mode(mode)
        got = hip.ensemble_stochastic(theta, 2, 1, SEED, PROBS, want_values=True)
        mv = got["model_values"]
        assert mv.shape == (6, mm.hostabi.stochastic_values_width(n, 0, len(pb.kappa_end_times)))
        for s in range(6):
            assert np.array_equal(mv[s, :-11 * n], host.stochastic_manager_values(theta[s], mode)), (init_mode, s)
        x0 = mv[:, -11 * n:].reshape(6, 11, n)
        if init_mode == INIT_FIXED:
            assert np.array_equal(x0, np.broadcast_to(c_round(pb.initial_state.reshape(11, n)), x0.shape)) and not got["status"].any()
        else:
            con = host.apply_constraints(theta, mode)
            state = pb.initial_state.reshape(11, n)
            for s in range(6):
                x = state.copy()
                x[1:9] *= con[s, 5:13, None]
                x[0] = pb.N - (((((((x[1] + x[2]) + x[3]) + x[4]) + x[5]) + x[6]) + x[7]) + x[8])
                assert np.array_equal(x0[s], c_round(x)), s
            assert list(got["status"]) == [0, 0, 0, 1, 0, 0]
    assert mv[2, 7] == (1.0 if mode == 0 else mm.draws.reflect_bound(np.array(5.0), np.array(0.01), np.array(1.0)))


def c_round(x):
    """round() of C: halves away from zero (np.round sends them to the even neighbour)"""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def numpy_quantiles(x, probs):
    """write_quantile's rule on the columns of x [count][...]"""
    srt = np.sort(x, axis=0)
    cnt = srt.shape[0]
    out = []
    for f in probs:
        pos = f * (cnt - 1)
        idx = int(pos)
        frac = pos - idx
        out.append(srt[idx] * (1.0 - frac) + srt[idx + 1] * frac if idx + 1 < cnt else srt[idx])
    return np.stack(out)


@pytest.mark.parametrize("R,path", [(256, "LDS"), (257, "global radix")])
def test_sort_path_boundary(mm, ref_fixture, R, path):
    """S = 64: S R = 16384 is the longest segment the LDS sort takes, S R = 16448 a multiple of 64 and no power of two."""
    pb = problem(mm, ref_fixture, n=2, T=2)
    hip = objective(mm, pb)
    theta = mm.draws.jitter_draws(pb, 23, 64)
    got = hip.ensemble_stochastic(theta, R, 4, SEED, PROBS, keep=1, want_values=True, want_final=True)
    assert got["n_valid"] == 64
    check_against_twin(mm, pb, got, R, 4, keep=1)
    x0 = got["model_values"][:, -22:].reshape(64, 1, 11, 2)
    daily = (got["final_state"] - x0)[:, :, [9, 10, 8]].reshape(64 * R, 3, 2)  # increments of CumH, CumICU, D over the one interval
    q = got["quantiles"]  # [6][n_probs][2][n]
    assert not q[:, :, 0].any()  # the first row of a run has no increment
    want = numpy_quantiles(daily, PROBS)  # [n_probs][3][n]
    assert np.array_equal(q[:3, :, 1], want.transpose(1, 0, 2)) and np.array_equal(q[3:, :, 1], want.transpose(1, 0, 2))
    assert q[0, -1, 1].max() > 0  # hospitalisations do occur


def test_paths_do_not_depend_on_the_call_around_them(mm, ref_fixture):
    pb = problem(mm, ref_fixture)
    hip = objective(mm, pb)
    theta = six_thetas(mm, pb)
    big = hip.ensemble_stochastic(theta, 256, 2, SEED, PROBS, keep=3, want_final=True)
    small = hip.ensemble_stochastic(theta, 64, 2, SEED, PROBS, want_final=True)
    assert np.array_equal(big["final_state"][:, :64], small["final_state"], equal_nan=True)
    assert np.array_equal(big["traj"][:, :, -1], small["final_state"][:, :3], equal_nan=True)
    # an invalid sample in front instead of a valid one: the sample behind it keeps its path
    swapped = theta.copy()
    swapped[0] = theta[3]
    holes = hip.ensemble_stochastic(swapped[:2], 64, 2, SEED, PROBS, want_final=True)
    assert list(holes["status"]) == [1, 0]
    assert np.array_equal(holes["final_state"][1], small["final_state"][1])
    other = hip.ensemble_stochastic(theta, 64, 2, SEED + 1, PROBS, want_final=True)
    assert not np.array_equal(other["final_state"][0], small["final_state"][0])


def test_arithmetic_mode_does_not_change_the_result(mm, ref_fixture):
    pb = problem(mm, ref_fixture)
    theta = six_thetas(mm, pb)
    a = objective(mm, pb, arith=mm.ARITH_STRICT).ensemble_stochastic(theta, 40, 2, SEED, PROBS, keep=40, want_values=True, want_final=True)
    b = objective(mm, pb, arith=mm.ARITH_FMA).ensemble_stochastic(theta, 40, 2, SEED, PROBS, keep=40, want_values=True, want_final=True)
    for key in ("quantiles", "extinct", "model_values", "traj", "final_state", "status"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_argument_errors_leave_the_outputs_untouched(mm, ref_fixture):
    pb = problem(mm, ref_fixture)
    hip = objective(mm, pb)
    theta = np.ascontiguousarray(six_thetas(mm, pb))
    S, T, n = 6, 6, 4
    pr = np.array(PROBS)
    bad_pr = np.array([0.5, 1.5])

    def call(R=4, m=2, keep=0, probs=pr, with_traj=True, ctx=None):
        q = np.full((6, probs.size, T, n), -7.0)
        ext, status, nv = np.full(S, -7.0), np.full(S, -7, dtype=np.int32), C.c_int32(-7)
        traj = np.full((S, max(keep, 1), T, 11, n), -7.0)
        rc = hip.lib.sepaihrd_ensemble_stochastic(hip.ctx if ctx is None else ctx, theta.ctypes.data, S, R, m, SEED, probs.ctypes.data, probs.size,
                                                  keep, q.ctypes.data, ext.ctypes.data, None, traj.ctypes.data if with_traj else None, None,
                                                  status.ctypes.data, C.byref(nv))
        untouched = (q == -7).all() and (ext == -7).all() and (status == -7).all() and nv.value == -7 and (traj == -7).all()
        return rc, untouched, hip.lib.sepaihrd_last_error(hip.ctx if ctx is None else ctx).decode()

    for kw, word in ((dict(R=0), "R must be >= 1"), (dict(m=0), "steps_per_interval must be >= 1"), (dict(keep=5), "keep must lie in [0, R]"),
                     (dict(keep=-1), "keep must lie in [0, R]"), (dict(keep=2, with_traj=False), "keep > 0 needs traj"),
                     (dict(R=2 ** 30), "below 2^31"), (dict(m=2 ** 20), "below 2^22"), (dict(probs=bad_pr), "probabilities must lie in [0, 1]"),
                     (dict(R=2 ** 27), "device memory")):
        rc, untouched, msg = call(**kw)
        assert rc == -1 and untouched and word in msg, (kw, rc, msg)
    assert hip.lib.sepaihrd_eval_batch_begin(hip.ctx, theta.ctypes.data, 3) == 0
    rc, untouched, msg = call()
    assert rc == -1 and untouched and "sepaihrd_eval_batch_begin is pending" in msg
    ll = np.empty(3)
    assert hip.lib.sepaihrd_eval_batch_end(hip.ctx, ll.ctypes.data, None, None, None, None) == 0
    # fp32 contexts are not served
    f32 = objective(mm, pb)
    f32.set_precision(mm.PRECISION_F32)
    rc, untouched, msg = call(ctx=f32.ctx)
    assert rc == -4 and untouched and "fp64" in msg
    # more than 16 age classes: no context of that width exists to call with
    with pytest.raises(RuntimeError, match="n_age > 16"):
        mm.HipObjective(problem(mm, ref_fixture, n=17))
    # a valid call afterwards succeeds, on both contexts that refused
    rc, untouched, _ = call(keep=2)
    assert rc == 0 and not untouched
    f32.set_precision(mm.PRECISION_F64)
    assert call(ctx=f32.ctx)[0] == 0


def test_cpp_adapter_equals_the_direct_call(mm, ref_fixture):
    pb = problem(mm, ref_fixture)
    samples = mm.draws.jitter_draws(pb, 5, 9)
    host = mm.hostabi.HostObjective(pb)
    for num, select_seed in ((0, 1), (4, 7)):
        via = host.posterior_stochastic(samples, num, select_seed, 33, 2, SEED, PROBS, initial_state_mode=INIT_FIXED)
        assert via["selected"].size == (9 if num == 0 else 4) and via["samples_used"] == via["selected"].size
        direct = objective(mm, pb, INIT_FIXED).ensemble_stochastic(samples[via["selected"]], 33, 2, SEED, PROBS)
        assert np.array_equal(via["quantiles"], direct["quantiles"]) and np.array_equal(via["extinct"], direct["extinct"])
        assert np.array_equal(via["status"], direct["status"])
