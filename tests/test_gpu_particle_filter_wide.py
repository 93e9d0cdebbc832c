"""The wide form of the particle filter on the device (sepaihrd_particle_loglik_wide: the particles in device memory, one launch per
segment of output rows and per weighted row) against the LDS kernel where that takes J and against the host twin for every J,
bit for bit.  The twin is fed the device's own model values and status, the problem's fixed data and its observations."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_particle_filter import KEYS, SEED, T, max_particles, three_thetas
from test_gpu_stochastic_sepaihrd import INIT_FROM_THETA, objective, problem as cut_fixture
from test_particle_filter_cpu import DBL_MAX

pytestmark = pytest.mark.gpu

WIDE_MAX = 65536


def problem(mm, ref_fixture, n, m=2, runup=2):
    """tests/test_gpu_particle_filter.py's problem with `runup` of its T = 10 output times before t = 0 (0: the run's first row is
    observed): the observations are one path of the model with a NaN cell, a negative cell and a row without any usable cell"""
    pb = cut_fixture(mm, ref_fixture, n, T - runup)
    x0 = pb.initial_state.reshape(11, n).copy()
    x0[0] = pb.N / 50.0 - x0[1:9].sum(axis=0)
    pb = pb.with_(N=pb.N / 50.0, initial_state=x0.ravel(), times=np.arange(T, dtype=np.float64) - runup)
    hip = objective(mm, pb)
    mv = hip.particle_loglik(pb.base_theta, 1, m, SEED, want_values=True)
    assert mv["status"][0] == 0
    tr = mm.hostabi.stochastic_from_values(mv["model_values"], mv["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, 1, m, SEED ^ 0x5555, [0.5],
                                           beta_end_times=pb.beta_end_times, keep=1)["traj"][0, 0]  # [T][11][n]
    obs = [np.diff(tr[:, c], axis=0, prepend=tr[:1, c])[runup:].copy() for c in (9, 10, 8)]
    obs[0][1, 0] = np.nan
    obs[2][2, n - 1] = -1.0
    for o in obs:
        o[4] = np.nan
    return pb.with_(obs_H=obs[0], obs_ICU=obs[1], obs_D=obs[2])


def wide_twin_of(mm, pb, got, J, m, seed=SEED):
    return mm.hostabi.particle_wide_from_values(got["model_values"], got["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H, pb.obs_ICU,
                                                pb.obs_D, J, m, seed, beta_end_times=pb.beta_end_times)


def check_three(got, blank_rows=(4,)):
    """three_thetas: two valid vectors and a rejected one"""
    assert list(got["status"]) == [0, 0, 1] and got["n_valid"] == 2
    assert got["loglik"][2] == -DBL_MAX and np.isnan(got["final_state"][2]).all() and np.isnan(got["increments"][2]).all() and np.isnan(got["ess"][2]).all()
    assert np.isfinite(got["loglik"][:2]).all() and (got["loglik"][:2] < 0).all() and np.isfinite(got["final_state"][:2]).all()
    for t in blank_rows:
        assert not got["increments"][:2, t].any() and np.isnan(got["ess"][:2, t]).all()
    assert np.isfinite(np.delete(got["ess"][:2], blank_rows, axis=1)).all()


@pytest.mark.parametrize("n,m,J", [(1, 1, 1), (3, 3, 17), (3, 1, 129), (16, 1, "max")])
def test_wide_equals_narrow(mm, ref_fixture, n, m, J):
    pb = problem(mm, ref_fixture, n, m)
    J = max_particles(mm, n) if J == "max" else J
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    narrow = hip.particle_loglik(theta, J, m, SEED, want_final=True, want_values=True)
    wide = hip.particle_loglik_wide(theta, J, m, SEED, want_final=True, want_values=True)
    check_three(wide)
    for key in KEYS + ("model_values", "status"):
        assert np.array_equal(narrow[key], wide[key], equal_nan=True), key
    assert narrow["n_valid"] == wide["n_valid"]
    ms = hip.particle_wide_timing()
    assert ms.shape == (2,) and (ms > 0).all()
    print(f"n {n} m {m} J {J}: loglik {wide['loglik'][:2]}, wide {ms[1]:.3f} ms, LDS kernel {hip.particle_timing()[1]:.3f} ms")


# (n, J, m), every J above sepaihrd_particle_max_particles(n) and none a power of two: 465 the first above the limit of n = 1, 513
# and 1025 one past a power of two (1025 also the first J whose scans leave LDS for device memory), 137 and 36 the first above
# the limits of n = 3 and n = 16, 700 and 300 several blocks of the propagation.  J lpc is no multiple of 64 except at (16, 36).
ABOVE = [(1, 465, 1), (1, 513, 3), (1, 1025, 1), (3, 137, 3), (3, 700, 1), (16, 36, 3), (16, 300, 1)]


@pytest.mark.parametrize("runup", [2, 0])
@pytest.mark.parametrize("n,J,m", ABOVE)
def test_wide_equals_twin_above_the_limit(mm, ref_fixture, n, J, m, runup):
    """runup = 0: no run-up, the run's first row is weighted and resampled before any step"""
    assert J > max_particles(mm, n) and J & (J - 1)
    pb = problem(mm, ref_fixture, n, m, runup)
    assert (pb.times[0] == 0.0) == (runup == 0)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    got = hip.particle_loglik_wide(theta, J, m, SEED, want_final=True, want_values=True)
    check_three(got)
    twin = wide_twin_of(mm, pb, got, J, m)
    for key in KEYS:
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    ess = np.delete(got["ess"][:2], 4, axis=1)
    assert (ess >= 1.0 - 1e-12).all() and (ess <= J + 1e-9).all() and (ess[:, 1:] > 1.0).any() and (ess < J).any()
    if runup == 0:
        assert (got["ess"][:2, 0] == J).all()  # the first row's increments are 0 for every particle: equal weights
    with pytest.raises(RuntimeError, match="J must lie in"):
        hip.particle_loglik(theta, J, m, SEED)
    print(f"n {n} m {m} J {J} runup {runup}: loglik {got['loglik'][:2]}, mean ESS {ess.mean():.1f}, {hip.particle_wide_timing()[1]:.3f} ms")


def test_the_last_two_rows_blank(mm, ref_fixture):
    """the final state comes out of a segment that ends without a resampling"""
    n, J, m = 3, 200, 2
    pb = problem(mm, ref_fixture, n, m)
    obs = [o.copy() for o in (pb.obs_H, pb.obs_ICU, pb.obs_D)]
    for o in obs:
        o[-2:] = np.nan
    cut = pb.with_(obs_H=obs[0], obs_ICU=obs[1], obs_D=obs[2])
    hip = objective(mm, cut)
    theta = three_thetas(mm, cut)
    got = hip.particle_loglik_wide(theta, J, m, SEED, want_final=True, want_values=True)
    check_three(got, blank_rows=(4, 6, 7))
    twin = wide_twin_of(mm, cut, got, J, m)
    for key in KEYS:
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    full = objective(mm, pb).particle_loglik_wide(theta, J, m, SEED, want_final=True)
    assert np.array_equal(got["increments"][:, :-2], full["increments"][:, :-2], equal_nan=True)
    assert not np.array_equal(got["final_state"][:2], full["final_state"][:2])


def test_no_usable_observation_is_the_stochastic_ensemble(mm, ref_fixture):
    """the whole grid one segment: slot j is replicate j of sepaihrd_ensemble_stochastic"""
    pb = problem(mm, ref_fixture, 4)
    blank = np.full_like(pb.obs_H, np.nan)
    pb = pb.with_(obs_H=blank, obs_ICU=blank, obs_D=blank)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    got = hip.particle_loglik_wide(theta, 600, 2, SEED, want_final=True)
    ens = hip.ensemble_stochastic(theta, 600, 2, SEED, [0.5], want_final=True)
    assert np.array_equal(got["final_state"], ens["final_state"], equal_nan=True)
    assert not got["loglik"][:2].any() and got["loglik"][2] == -DBL_MAX and np.isnan(got["ess"]).all()
    assert not got["increments"][:2].any() and np.isnan(got["increments"][2]).all()


def test_the_chunking_does_not_change_a_result(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = np.concatenate([three_thetas(mm, pb), mm.draws.jitter_draws(pb, 12, 2)])
    J, m = 150, 2
    runs = {chunk: hip.particle_loglik_wide(theta, J, m, SEED, theta_chunk=chunk, want_final=True) for chunk in (1, 2, 5, 0)}
    assert list(runs[0]["status"]) == [0, 0, 1, 0, 0]
    for chunk in (1, 2, 5):
        for key in KEYS + ("status",):
            assert np.array_equal(runs[chunk][key], runs[0][key], equal_nan=True), (chunk, key)
    assert len(set(runs[0]["loglik"])) == 5
    # an invalid vector in front of a valid one; fewer outputs asked for; another seed
    holes = hip.particle_loglik_wide(theta[[2, 1]], J, m, SEED, theta_chunk=1, want_final=True)
    assert list(holes["status"]) == [1, 0] and holes["loglik"][1] == runs[0]["loglik"][1]
    assert np.array_equal(holes["final_state"][1], runs[0]["final_state"][1]) and np.isnan(holes["final_state"][0]).all()
    lean = hip.particle_loglik_wide(theta[:2], J, m, SEED, want_increments=False, want_ess=False)
    assert np.array_equal(lean["loglik"], runs[0]["loglik"][:2]) and "ess" not in lean
    assert hip.particle_loglik_wide(theta[:2], J, m, SEED + 1)["loglik"][0] != runs[0]["loglik"][0]


def wide_logw_sets():
    """tests/test_particle_filter_cpu.py's logw_sets patterns at J = 513 (LDS scans), 4097 and 65 536 (device memory): random, one
    dominant weight, ties, a spread of 1400 in log"""
    rng = np.random.default_rng(20250101)
    out = []
    for J in (513, 4097, WIDE_MAX):
        out.append((f"random-{J}", rng.normal(-300.0, 3.0, J)))
        dominant = rng.normal(-50.0, 1.0, J)
        dominant[J // 2] = 40.0
        out.append((f"dominant-{J}", dominant))
        out.append((f"ties-{J}", np.full(J, -12.5)))
        out.append((f"two-levels-{J}", np.where(np.arange(J) % 3 == 0, -1.0, -1.0 + math.log(2.0))))
        out.append((f"spread-down-{J}", np.linspace(0.0, -1400.0, J)))
    return out


def test_wide_resample_probe_equals_the_twin(mm, ref_fixture):
    hip = objective(mm, cut_fixture(mm, ref_fixture, 4, 2))
    for k, (name, logw) in enumerate(wide_logw_sets()):
        dev = hip.particle_wide_resample_device(logw, SEED + k, b=k % 3, row=k)
        twin = mm.hostabi.particle_resample(logw, SEED + k, b=k % 3, row=k)
        assert np.array_equal(dev["ancestors"], twin["ancestors"]), name
        assert dev["increment"] == twin["increment"] and dev["ess"] == twin["ess"], name
        if name.startswith("ties"):
            assert np.array_equal(dev["ancestors"], np.arange(len(logw))) and dev["ess"] == len(logw)
        if name.startswith("dominant"):
            assert (dev["ancestors"] == len(logw) // 2).all()
    err = C.create_string_buffer(256)
    one = np.zeros(1)
    anc, inc, ess = np.full(1, -7, dtype=np.int32), C.c_double(-7.0), C.c_double(-7.0)
    for J in (0, WIDE_MAX + 1):
        rc = hip.lib.sepaihrd_particle_wide_resample_device(-1, SEED, 0, 0, one.ctypes.data, J, anc.ctypes.data, C.byref(inc), C.byref(ess), err,
                                                            len(err))
        assert rc == -1 and b"J in [1, 65536]" in err.value and anc[0] == -7 and inc.value == -7.0 and ess.value == -7.0


def test_arithmetic_mode_does_not_change_the_result(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    J = max_particles(mm, 4) + 64
    a = objective(mm, pb, arith=mm.ARITH_STRICT).particle_loglik_wide(theta, J, 2, SEED, want_final=True, want_values=True)
    b = objective(mm, pb, arith=mm.ARITH_FMA).particle_loglik_wide(theta, J, 2, SEED, want_final=True, want_values=True)
    for key in KEYS + ("model_values", "status"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_argument_errors_leave_the_outputs_untouched(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = np.ascontiguousarray(three_thetas(mm, pb))
    B, n, Tp = 3, 4, T - 2

    def call(B=B, J=8, m=2, chunk=0, ctx=None):
        ll, inc, ess = np.full(3, -7.0), np.full((3, Tp), -7.0), np.full((3, Tp), -7.0)
        fin, status, nv = np.full((3, 8, 11, n), -7.0), np.full(3, -7, dtype=np.int32), C.c_int32(-7)
        rc = hip.lib.sepaihrd_particle_loglik_wide(hip.ctx if ctx is None else ctx, theta.ctypes.data, B, J, m, SEED, chunk, ll.ctypes.data,
                                                   inc.ctypes.data, ess.ctypes.data, fin.ctypes.data if J <= 8 else None, None, status.ctypes.data,
                                                   C.byref(nv))
        untouched = (ll == -7).all() and (inc == -7).all() and (ess == -7).all() and (fin == -7).all() and (status == -7).all() and nv.value == -7
        return rc, untouched, hip.lib.sepaihrd_last_error(hip.ctx if ctx is None else ctx).decode()

    for kw, word in ((dict(B=0), "B must be >= 1"), (dict(J=0), "J must lie in [1, 65536]"), (dict(J=WIDE_MAX + 1), "J must lie in [1, 65536]"),
                     (dict(chunk=-1), "theta_chunk must be >= 0"), (dict(m=0), "steps_per_interval must be >= 1"), (dict(m=2 ** 20), "below 2^22"),
                     (dict(B=2 ** 30), "B x J must stay below 2^31"), (dict(B=2 ** 15, J=WIDE_MAX), "B x J must stay below 2^31"),
                     (dict(B=2 ** 20, J=1024, chunk=2 ** 20), "device memory")):  # 2^30 particles at once: 396 GiB of scratch
        rc, untouched, msg = call(**kw)
        assert rc == -1 and untouched and word in msg and msg.startswith("particle_loglik_wide: "), (kw, rc, msg)
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
    # a valid call afterwards succeeds, on both contexts that refused
    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    f32.set_precision(mm.PRECISION_F64)
    assert call(ctx=f32.ctx)[0] == 0
    # a NULL loglik or theta
    assert hip.lib.sepaihrd_particle_loglik_wide(hip.ctx, theta.ctypes.data, B, 8, 2, SEED, 0, None, None, None, None, None, None, None) == -1
    # the LDS kernel's limit and its message are where they were
    with pytest.raises(RuntimeError, match=r"particle_loglik: J must lie in \[1, %d\]" % max_particles(mm, n)):
        hip.particle_loglik(theta, max_particles(mm, n) + 1, 2, SEED)


def test_each_form_keeps_its_own_timing(mm, ref_fixture):
    """the LDS and the wide calls share one body: a call of one form, Poisson or dispersed, writes that form's pair of times and
    leaves the other form's exactly as it was"""
    from test_gpu_particle_nb import twin_of  # (that module imports this one)
    n, m, J = 3, 2, 17
    pb = problem(mm, ref_fixture, n, m)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    assert not hip.particle_timing().any() and not hip.particle_wide_timing().any()
    for disp in (None, (1.0, np.inf, 5.0)):
        before = hip.particle_timing(), hip.particle_wide_timing()
        narrow = hip.particle_loglik(theta, J, m, SEED, want_final=True, want_values=True, dispersion=disp)
        after_narrow = hip.particle_timing(), hip.particle_wide_timing()
        wide = hip.particle_loglik_wide(theta, J, m, SEED, want_final=True, want_values=True, dispersion=disp)
        after_wide = hip.particle_timing(), hip.particle_wide_timing()
        print(f"dispersion {disp}: before {before}, after the LDS call {after_narrow}, after the wide call {after_wide}")
        assert np.array_equal(after_narrow[1], before[1]), disp
        if disp is None:
            assert list(after_narrow[1]) == [0.0, 0.0]
        assert np.array_equal(after_wide[0], after_narrow[0]), disp
        assert np.isfinite(after_narrow[0]).all() and (after_narrow[0] > 0).all(), disp
        assert np.isfinite(after_wide[1]).all() and (after_wide[1] > 0).all(), disp
        if disp is not None:
            for got, is_wide in ((narrow, False), (wide, True)):
                twin = twin_of(mm, pb, got, J, m, disp, is_wide)
                for key in KEYS:
                    assert np.array_equal(got[key], twin[key], equal_nan=True), (is_wide, key)


def test_cpp_adapter_goes_wide_above_the_limit(mm, ref_fixture):
    """HipParticleLikelihood::calculateBatch with more particles than the LDS kernel takes is sepaihrd_particle_loglik_wide at
    seed0 + (calls so far)"""
    pb = problem(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    J = max_particles(mm, 4) + 50
    host = mm.hostabi.HostObjective(pb)
    via = host.particle_likelihood(theta, J, 2, SEED, n_calls=2, initial_state_mode=INIT_FROM_THETA)
    hip = objective(mm, pb, INIT_FROM_THETA)
    for c in range(2):
        direct = hip.particle_loglik_wide(theta, J, 2, SEED + c)
        assert np.array_equal(via["values"][c], direct["loglik"]) and np.array_equal(via["status"][c], direct["status"]), c
    assert via["values"][0, 2] == -DBL_MAX and list(via["status"][0]) == [0, 0, 1]
    assert (via["values"][0, :2] != via["values"][1, :2]).all()
