"""The bootstrap particle filter of the stochastic SEPAIHRD model on the device (sepaihrd_particle_loglik) against the host twin,
bit for bit: the twin is fed the device's own model values and status, the problem's fixed data and its observations."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_stochastic_sepaihrd import INIT_FIXED, INIT_FROM_THETA, objective, problem as cut_fixture
from test_particle_filter_cpu import DBL_MAX, logw_sets

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF0  # both words of the key in use
T, RUNUP = 10, 2              # ten output times, the first two of them run-up (t < 0)
KEYS = ("loglik", "increments", "ess", "final_state")


def problem(mm, ref_fixture, n, m=2):
    """The reference fixture cut to T output times of which RUNUP lie before t = 0, a population of 10^4 .. 10^5 per age class, the
    eight initial-state multipliers calibrated.  The observations are the daily counts of one path of the stochastic model at the
    base parameters (the host twin's replicate 0), with a NaN cell, a negative cell and a row without any usable cell."""
    pb = cut_fixture(mm, ref_fixture, n, T - RUNUP)
    x0 = pb.initial_state.reshape(11, n).copy()
    x0[0] = pb.N / 50.0 - x0[1:9].sum(axis=0)
    pb = pb.with_(N=pb.N / 50.0, initial_state=x0.ravel(), times=np.arange(T, dtype=np.float64) - RUNUP)
    hip = objective(mm, pb)
    mv = hip.particle_loglik(pb.base_theta, 1, m, SEED, want_values=True)
    assert mv["status"][0] == 0
    tr = mm.hostabi.stochastic_from_values(mv["model_values"], mv["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, 1, m, SEED ^ 0x5555, [0.5],
                                           beta_end_times=pb.beta_end_times, keep=1)["traj"][0, 0]  # [T][11][n]
    obs = [np.diff(tr[:, c], axis=0, prepend=tr[:1, c])[RUNUP:].copy() for c in (9, 10, 8)]
    obs[0][1, 0] = np.nan
    obs[2][2, n - 1] = -1.0
    for o in obs:
        o[4] = np.nan
    return pb.with_(obs_H=obs[0], obs_ICU=obs[1], obs_D=obs[2])


def three_thetas(mm, pb):
    th = mm.draws.jitter_draws(pb, 11, 3)
    th[0] = pb.base_theta
    th[1, 0] = 5.0   # beta beyond its upper bound: clamped onto it
    th[2, 5] = 1e6   # E0 multiplier: E(0) exceeds the population, the initial-state rule rejects the vector
    return th


def twin_of(mm, pb, got, J, m, seed=SEED):
    return mm.hostabi.particle_from_values(got["model_values"], got["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H, pb.obs_ICU,
                                           pb.obs_D, J, m, seed, beta_end_times=pb.beta_end_times)


def max_particles(mm, n):
    return mm.hostabi.particle_max_particles(n)


# (n, m, J): J = 1; 5 (no power of two); J lpc = 68 (just over one wavefront: 68 at n = 1, 17 at n = 3); more than the 512 / lpc
# particles a block runs at a time, so that a second, ragged pass follows (129 and the limit at n = 3, 33 and the limit at
# n = 16; n = 1 has no such J: its limit is below 512); the limit of every n.  "max" is sepaihrd_particle_max_particles(n).
CASES = [(1, 1, 1), (1, 3, 5), (1, 3, 68), (1, 1, "max"), (3, 3, 1), (3, 1, 5), (3, 3, 17), (3, 1, 129), (3, 3, "max"), (16, 1, 5), (16, 3, 33),
         (16, 1, "max")]


@pytest.mark.parametrize("n,m,J", CASES)
def test_device_equals_twin(mm, ref_fixture, n, m, J):
    pb = problem(mm, ref_fixture, n, m)
    J = max_particles(mm, n) if J == "max" else J
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    got = hip.particle_loglik(theta, J, m, SEED, want_final=True, want_values=True)
    assert list(got["status"]) == [0, 0, 1] and got["n_valid"] == 2
    assert got["loglik"][2] == -DBL_MAX and np.isnan(got["final_state"][2]).all() and np.isnan(got["increments"][2]).all()
    assert np.isfinite(got["loglik"][:2]).all() and (got["loglik"][:2] < 0).all() and np.isfinite(got["final_state"][:2]).all()
    twin = twin_of(mm, pb, got, J, m)
    for key in KEYS:
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    # the row without a usable cell, and the rows around it
    assert not got["increments"][:2, 4].any() and np.isnan(got["ess"][:2, 4]).all()
    ess = np.delete(got["ess"][:2], 4, axis=1)
    assert (ess >= 1.0 - 1e-12).all() and (ess <= J + 1e-9).all()
    if J > 1:
        assert (ess[:, 1:] > 1.0).any() and (ess < J).any()  # neither one surviving particle throughout nor equal weights
    else:
        ens = hip.ensemble_stochastic(theta, 1, m, SEED, [0.5], want_final=True)  # a single particle is replicate 0
        assert np.array_equal(ens["final_state"], got["final_state"], equal_nan=True)
    print(f"n {n} m {m} J {J}: loglik {got['loglik'][:2]}, mean ESS {ess.mean():.2f}, kernel {hip.particle_timing()[1]:.3f} ms")


def test_slots_are_the_stochastic_replicates_through_the_run_up(mm, ref_fixture):
    """no usable observation at all: the filter is sepaihrd_ensemble_stochastic, slot j its replicate j"""
    pb = problem(mm, ref_fixture, 4)
    blank = np.full_like(pb.obs_H, np.nan)
    pb = pb.with_(obs_H=blank, obs_ICU=blank, obs_D=blank)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    got = hip.particle_loglik(theta, 40, 2, SEED, want_final=True)
    ens = hip.ensemble_stochastic(theta, 40, 2, SEED, [0.5], want_final=True)
    assert np.array_equal(got["final_state"], ens["final_state"], equal_nan=True)
    assert not got["loglik"][:2].any() and np.isnan(got["ess"]).all()


def test_a_position_does_not_depend_on_the_call_around_it(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    full = hip.particle_loglik(theta, 20, 2, SEED, want_final=True)
    lean = hip.particle_loglik(theta[:2], 20, 2, SEED, want_increments=False, want_ess=False)
    assert np.array_equal(lean["loglik"], full["loglik"][:2]) and "ess" not in lean
    swapped = theta[[2, 1]]  # an invalid vector in front instead of a valid one
    holes = hip.particle_loglik(swapped, 20, 2, SEED, want_final=True)
    assert list(holes["status"]) == [1, 0] and holes["loglik"][1] == full["loglik"][1]
    assert np.array_equal(holes["final_state"][1], full["final_state"][1])
    assert hip.particle_loglik(theta[:2], 20, 2, SEED + 1)["loglik"][0] != full["loglik"][0]
    ms = hip.particle_timing()
    assert ms.shape == (2,) and (ms > 0).all()


def test_resample_probe_equals_the_twin(mm, ref_fixture):
    hip = objective(mm, cut_fixture(mm, ref_fixture, 4, 2))
    for k, (name, logw) in enumerate(logw_sets()):
        dev = hip.particle_resample_device(logw, SEED + k, b=k % 3, row=k)
        twin = mm.hostabi.particle_resample(logw, SEED + k, b=k % 3, row=k)
        assert np.array_equal(dev["ancestors"], twin["ancestors"]), name
        assert dev["increment"] == twin["increment"] and dev["ess"] == twin["ess"], name
    err = C.create_string_buffer(256)
    one = np.zeros(1)
    anc, inc, ess = np.full(1, -7, dtype=np.int32), C.c_double(-7.0), C.c_double(-7.0)
    for J in (0, 513):
        rc = hip.lib.sepaihrd_particle_resample_device(-1, SEED, 0, 0, one.ctypes.data, J, anc.ctypes.data, C.byref(inc), C.byref(ess), err, len(err))
        assert rc == -1 and b"J in [1, 512]" in err.value and anc[0] == -7 and inc.value == -7.0


def test_arithmetic_mode_does_not_change_the_result(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    a = objective(mm, pb, arith=mm.ARITH_STRICT).particle_loglik(theta, 33, 2, SEED, want_final=True, want_values=True)
    b = objective(mm, pb, arith=mm.ARITH_FMA).particle_loglik(theta, 33, 2, SEED, want_final=True, want_values=True)
    for key in KEYS + ("model_values", "status"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_argument_errors_leave_the_outputs_untouched(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = np.ascontiguousarray(three_thetas(mm, pb))
    B, n, Tp = 3, 4, T - RUNUP
    J_max = max_particles(mm, n)

    def call(B=B, J=8, m=2, ctx=None):
        ll, inc, ess = np.full(3, -7.0), np.full((3, Tp), -7.0), np.full((3, Tp), -7.0)
        fin, status, nv = np.full((3, 8, 11, n), -7.0), np.full(3, -7, dtype=np.int32), C.c_int32(-7)
        rc = hip.lib.sepaihrd_particle_loglik(hip.ctx if ctx is None else ctx, theta.ctypes.data, B, J, m, SEED, ll.ctypes.data, inc.ctypes.data,
                                              ess.ctypes.data, fin.ctypes.data if J <= 8 else None, None, status.ctypes.data, C.byref(nv))
        untouched = (ll == -7).all() and (inc == -7).all() and (ess == -7).all() and (fin == -7).all() and (status == -7).all() and nv.value == -7
        return rc, untouched, hip.lib.sepaihrd_last_error(hip.ctx if ctx is None else ctx).decode()

    for kw, word in ((dict(B=0), "B must be >= 1"), (dict(J=0), "J must lie in [1, %d]" % J_max), (dict(J=J_max + 1), "J must lie in [1, %d]" % J_max),
                     (dict(m=0), "steps_per_interval must be >= 1"), (dict(m=2 ** 20), "below 2^22"), (dict(B=2 ** 30), "device memory")):
        rc, untouched, msg = call(**kw)
        assert rc == -1 and untouched and word in msg and msg.startswith("particle_loglik: "), (kw, rc, msg)
    assert hip.lib.sepaihrd_eval_batch_begin(hip.ctx, theta.ctypes.data, 2) == 0
    rc, untouched, msg = call()
    assert rc == -1 and untouched and "sepaihrd_eval_batch_begin is pending" in msg
    ll = np.empty(2)
    assert hip.lib.sepaihrd_eval_batch_end(hip.ctx, ll.ctypes.data, None, None, None, None) == 0
    # fp32 contexts are not served
    f32 = objective(mm, pb)
    f32.set_precision(mm.PRECISION_F32)
    rc, untouched, msg = call(ctx=f32.ctx)
    assert rc == -4 and untouched and "fp64" in msg
    # more than 16 age classes: no context of that width exists to call with, and no particle limit either
    with pytest.raises(RuntimeError, match="n_age > 16"):
        mm.HipObjective(cut_fixture(mm, ref_fixture, n=17))
    assert hip.lib.sepaihrd_particle_max_particles(17) == -1
    # a valid call afterwards succeeds, on both contexts that refused
    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    f32.set_precision(mm.PRECISION_F64)
    assert call(ctx=f32.ctx)[0] == 0
    # a NULL loglik or theta
    assert hip.lib.sepaihrd_particle_loglik(hip.ctx, theta.ctypes.data, B, 8, 2, SEED, None, None, None, None, None, None, None) == -1


def test_cpp_adapter_equals_the_direct_call(mm, ref_fixture):
    """HipParticleLikelihood::calculateBatch is the device call at seed0 + (calls so far): two successive calls at the same
    parameter vectors see fresh noise"""
    pb = problem(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    host = mm.hostabi.HostObjective(pb)
    via = host.particle_likelihood(theta, 24, 2, SEED, n_calls=3, initial_state_mode=INIT_FROM_THETA)
    hip = objective(mm, pb, INIT_FROM_THETA)
    for c in range(3):
        direct = hip.particle_loglik(theta, 24, 2, SEED + c)
        assert np.array_equal(via["values"][c], direct["loglik"]) and np.array_equal(via["status"][c], direct["status"]), c
    assert via["values"][0, 2] == -DBL_MAX and list(via["status"][0]) == [0, 0, 1]
    assert (via["values"][0, :2] != via["values"][1, :2]).all() and (via["values"][1, :2] != via["values"][2, :2]).all()
    fixed = host.particle_likelihood(theta, 24, 2, SEED, initial_state_mode=INIT_FIXED)
    assert np.array_equal(fixed["values"][0], objective(mm, pb, INIT_FIXED).particle_loglik(theta, 24, 2, SEED)["loglik"])
    assert not fixed["status"].any()
