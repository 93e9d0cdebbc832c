"""The negative-binomial observation model of both particle filters on the device (sepaihrd_particle_loglik_nb,
sepaihrd_particle_loglik_wide_nb) against the host twin, bit for bit: the twin is fed the device's own model
values and status, the problem's fixed data, its observations and the dispersion.  Also the Poisson path through the new calls, the
two forms against each other, the probe of the device's term, the argument rules, the C++ adapter after setDispersion and the exact
likelihood of a tiny epidemic."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_particle_filter import CASES as LDS_CASES, KEYS, SEED, T, max_particles, three_thetas
from test_gpu_particle_filter_exact import tiny_problem
from test_gpu_particle_filter_wide import problem
from test_gpu_stochastic_sepaihrd import INIT_FIXED, INIT_FROM_THETA, objective
from test_particle_filter_cpu import DBL_MAX
from test_particle_filter_exact_cpu import CASES as TINY, check_prefix_likelihoods
from test_particle_nb_cpu import DISPERSION_EXACT, EXACT_B, EXACT_K, EXACT_SEED, GRID_K, INF, MIXED, exact_filter_nb, term_grid

pytestmark = pytest.mark.gpu

EVEN = (3.0, 3.0, 3.0)
DISPERSIONS = (MIXED, EVEN)
ALL = KEYS + ("model_values", "status")
_problems = {}


def problem_of(mm, ref_fixture, n, m=2, runup=2):
    """tests/test_gpu_particle_filter_wide.py's problem (ten output times; a theta at a bound and a rejected one come with
    three_thetas; a NaN cell, a negative cell and a row without a usable cell), built once per shape.  Every usable observation
    is raised by 2: g(0, k) = g(1, k) = 0 for every k, and the path's own counts are mostly 0 and 1, so that without it the row
    constants would be next to all zero."""
    key = (n, m, runup)
    if key not in _problems:
        pb = problem(mm, ref_fixture, n, m, runup)
        lift = lambda o: np.where(np.asarray(o) >= 0.0, np.asarray(o) + 2.0, o)
        _problems[key] = pb.with_(obs_H=lift(pb.obs_H), obs_ICU=lift(pb.obs_ICU), obs_D=lift(pb.obs_D))
    return _problems[key]


def twin_of(mm, pb, got, J, m, dispersion, wide, seed=SEED):
    call = mm.hostabi.particle_wide_from_values if wide else mm.hostabi.particle_from_values
    return call(got["model_values"], got["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H, pb.obs_ICU, pb.obs_D, J, m, seed,
                beta_end_times=pb.beta_end_times, dispersion=dispersion)


def check_three(got, blank_row=4):
    """three_thetas: two valid vectors and a rejected one (the sign of loglik is not fixed: the weights leave out -lgamma(obs + 1))"""
    assert list(got["status"]) == [0, 0, 1] and got["n_valid"] == 2
    assert got["loglik"][2] == -DBL_MAX and np.isnan(got["final_state"][2]).all() and np.isnan(got["increments"][2]).all() and np.isnan(got["ess"][2]).all()
    assert np.isfinite(got["loglik"][:2]).all() and np.isfinite(got["final_state"][:2]).all()
    assert not got["increments"][:2, blank_row].any() and np.isnan(got["ess"][:2, blank_row]).all()
    assert np.isfinite(np.delete(got["ess"][:2], blank_row, axis=1)).all()


def same(a, b, keys, what):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


@pytest.mark.parametrize("n,m,J", LDS_CASES)
def test_lds_kernel_equals_twin(mm, ref_fixture, n, m, J):
    pb = problem_of(mm, ref_fixture, n, m)
    J = max_particles(mm, n) if J == "max" else J
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    poisson = hip.particle_loglik(theta, J, m, SEED)
    for disp in DISPERSIONS:
        got = hip.particle_loglik(theta, J, m, SEED, want_final=True, want_values=True, dispersion=disp)
        check_three(got)
        same(got, twin_of(mm, pb, got, J, m, disp, False), KEYS, disp)
        assert (got["loglik"][:2] != poisson["loglik"][:2]).all()
        G = hip.particle_nb_row_constants(disp)
        assert np.array_equal(G, mm.hostabi.particle_nb_row_constants(pb.obs_H, pb.obs_ICU, pb.obs_D, n, T - 2, disp)) and G[4] == 0.0 and G[0] != 0.0
        print(f"n {n} m {m} J {J} k {disp}: loglik {got['loglik'][:2]}, kernel {hip.particle_timing()[1]:.3f} ms")


# (n, J, m): one above the limit of n = 1 and of n = 3, the first J whose scans leave LDS, and n = 16 one above its limit
WIDE_CASES = [(1, 465, 1), (1, 1025, 3), (3, 137, 3), (16, 36, 1)]


@pytest.mark.parametrize("runup", [2, 0])
@pytest.mark.parametrize("n,J,m", WIDE_CASES)
def test_wide_form_equals_twin(mm, ref_fixture, n, J, m, runup):
    assert J > max_particles(mm, n)
    pb = problem_of(mm, ref_fixture, n, m, runup)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    for disp in DISPERSIONS:
        got = hip.particle_loglik_wide(theta, J, m, SEED, want_final=True, want_values=True, dispersion=disp)
        check_three(got)
        same(got, twin_of(mm, pb, got, J, m, disp, True), KEYS, disp)
        with pytest.raises(RuntimeError, match="J must lie in"):
            hip.particle_loglik(theta, J, m, SEED, dispersion=disp)
        print(f"n {n} m {m} J {J} runup {runup} k {disp}: loglik {got['loglik'][:2]}, {hip.particle_wide_timing()[1]:.3f} ms")


@pytest.mark.parametrize("n,m,J", [(3, 3, 17), (16, 1, 35)])
def test_infinite_dispersion_is_the_poisson_call_and_wide_equals_lds(mm, ref_fixture, n, m, J):
    pb = problem_of(mm, ref_fixture, n, m)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    none = (INF, INF, INF)
    kw = dict(want_final=True, want_values=True)
    same(hip.particle_loglik(theta, J, m, SEED, dispersion=none, **kw), hip.particle_loglik(theta, J, m, SEED, **kw), ALL, "LDS")
    same(hip.particle_loglik_wide(theta, J, m, SEED, dispersion=none, **kw), hip.particle_loglik_wide(theta, J, m, SEED, **kw), ALL, "wide")
    assert not hip.particle_nb_row_constants(none).any()
    for disp in DISPERSIONS:
        same(hip.particle_loglik_wide(theta, J, m, SEED, dispersion=disp, **kw), hip.particle_loglik(theta, J, m, SEED, dispersion=disp, **kw), ALL, disp)


def test_the_chunking_does_not_change_a_result(mm, ref_fixture):
    pb = problem_of(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = np.concatenate([three_thetas(mm, pb), mm.draws.jitter_draws(pb, 12, 2)])
    J, m = 150, 2
    runs = {chunk: hip.particle_loglik_wide(theta, J, m, SEED, theta_chunk=chunk, want_final=True, dispersion=MIXED) for chunk in (1, 2, 0)}
    assert list(runs[0]["status"]) == [0, 0, 1, 0, 0] and len(set(runs[0]["loglik"])) == 5
    for chunk in (1, 2):
        same(runs[chunk], runs[0], KEYS + ("status",), chunk)
    lean = hip.particle_loglik_wide(theta[:2], J, m, SEED, want_increments=False, want_ess=False, dispersion=MIXED)
    assert np.array_equal(lean["loglik"], runs[0]["loglik"][:2]) and "ess" not in lean


def test_term_probe_equals_the_twin(mm, ref_fixture):
    hip = objective(mm, problem_of(mm, ref_fixture, 4))
    obs, inc = term_grid()
    obs = np.concatenate([obs, [np.nan, -1.0, np.inf, 2.0, 3.0]])
    inc = np.concatenate([inc, np.array([3, 3, 3, -4, 2 ** 31 - 1], dtype=np.int32)])
    for k in GRID_K + (1e-3,):
        dev = hip.particle_nb_term_device(obs, inc, k)
        assert np.array_equal(dev, mm.hostabi.particle_nb_term(obs, inc, k)), k
        assert not dev[-5:-2].any() and np.isfinite(dev).all()
    err = C.create_string_buffer(256)
    out = np.full(3, -7.0)
    for count, k in ((0, 1.0), (3, INF), (3, float("nan")), (3, 0.0), (3, 2e6)):
        rc = hip.lib.sepaihrd_particle_nb_term_device(-1, obs.ctypes.data, inc.ctypes.data, count, k, out.ctypes.data, err, len(err))
        assert rc == -1 and b"finite k in [1e-3, 1e6]" in err.value and (out == -7.0).all(), (count, k)


def test_arithmetic_mode_does_not_change_the_result(mm, ref_fixture):
    pb = problem_of(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    J = max_particles(mm, 4)
    for wide, JJ in ((False, J), (True, J + 64)):
        runs = []
        for arith in (mm.ARITH_STRICT, mm.ARITH_FMA):
            hip = objective(mm, pb, arith=arith)
            call = hip.particle_loglik_wide if wide else hip.particle_loglik
            runs.append(call(theta, JJ, 2, SEED, want_final=True, want_values=True, dispersion=MIXED))
        same(runs[0], runs[1], ALL, wide)


def test_argument_errors_leave_the_outputs_untouched(mm, ref_fixture):
    pb = problem_of(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = np.ascontiguousarray(three_thetas(mm, pb))
    B, n, Tp = 3, 4, T - 2
    good = np.array(MIXED)

    def call(wide, disp=good, B=B, J=8, m=2):
        ll, inc, ess = np.full(3, -7.0), np.full((3, Tp), -7.0), np.full((3, Tp), -7.0)
        fin, status, nv = np.full((3, 8, 11, n), -7.0), np.full(3, -7, dtype=np.int32), C.c_int32(-7)
        d = None if disp is None else np.ascontiguousarray(disp, dtype=np.float64).ctypes.data
        outs = (ll.ctypes.data, inc.ctypes.data, ess.ctypes.data, fin.ctypes.data if J <= 8 else None, None, status.ctypes.data, C.byref(nv))
        if wide:
            rc = hip.lib.sepaihrd_particle_loglik_wide_nb(hip.ctx, theta.ctypes.data, B, J, m, SEED, d, 0, *outs)
        else:
            rc = hip.lib.sepaihrd_particle_loglik_nb(hip.ctx, theta.ctypes.data, B, J, m, SEED, d, *outs)
        untouched = (ll == -7).all() and (inc == -7).all() and (ess == -7).all() and (fin == -7).all() and (status == -7).all() and nv.value == -7
        return rc, untouched, hip.lib.sepaihrd_last_error(hip.ctx).decode()

    for wide in (False, True):
        for disp, word in ((None, "need dispersion"), ((np.nan, 1, 1), "dispersion[0] (k_H) is NaN"), ((1, -np.inf, 1), "dispersion[1] (k_ICU) is -inf"),
                           ((1, 1, 0.0), "dispersion[2] (k_D) = 0 is not positive"), ((9e-4, 1, 1), "is below 1e-3"), ((1, 1, 1.5e6), "is above 1e6")):
            rc, untouched, msg = call(wide, disp)
            assert rc == -1 and untouched and word in msg, (wide, disp, msg)
        # the form's own rules, with their messages
        who = "particle_loglik_wide: " if wide else "particle_loglik: "
        for kw, word in ((dict(B=0), "B must be >= 1"), (dict(J=0), "J must lie in"), (dict(m=0), "steps_per_interval must be >= 1")):
            rc, untouched, msg = call(wide, **kw)
            assert rc == -1 and untouched and word in msg and msg.startswith(who), (wide, kw, msg)
        rc, untouched, _ = call(wide)
        assert rc == 0 and not untouched
        rc, untouched, _ = call(wide, (1e-3, 1e6, INF))
        assert rc == 0 and not untouched
    rc, untouched, msg = call(False, J=max_particles(mm, n) + 1)
    assert rc == -1 and untouched and "J must lie in" in msg
    G = np.full(Tp, -7.0)
    assert hip.lib.sepaihrd_particle_nb_row_constants(hip.ctx, np.array([1.0, -1.0, 1.0]).ctypes.data, G.ctypes.data) == -1 and (G == -7.0).all()


def test_cpp_adapter_after_set_dispersion(mm, ref_fixture):
    """HipParticleLikelihood::calculateBatch after setDispersion is the _nb call of the form its particle count selects, at
    seed0 + (calls so far)"""
    pb = problem_of(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    host = mm.hostabi.HostObjective(pb)
    hip = objective(mm, pb, INIT_FROM_THETA)
    limit = max_particles(mm, 4)
    for J in (limit, limit + 50):
        via = host.particle_likelihood(theta, J, 2, SEED, n_calls=2, initial_state_mode=INIT_FROM_THETA, dispersion=MIXED)
        call = hip.particle_loglik_wide if J > limit else hip.particle_loglik
        for c in range(2):
            direct = call(theta, J, 2, SEED + c, dispersion=MIXED)
            assert np.array_equal(via["values"][c], direct["loglik"]) and np.array_equal(via["status"][c], direct["status"]), (J, c)
        assert via["values"][0, 2] == -DBL_MAX and list(via["status"][0]) == [0, 0, 1]
        plain = host.particle_likelihood(theta, J, 2, SEED, n_calls=1, initial_state_mode=INIT_FROM_THETA)
        assert (plain["values"][0, :2] != via["values"][0, :2]).all()
        assert np.array_equal(plain["values"][0], call(theta, J, 2, SEED)["loglik"])
        none = host.particle_likelihood(theta, J, 2, SEED, n_calls=1, initial_state_mode=INIT_FROM_THETA, dispersion=(INF, INF, INF))
        assert np.array_equal(none["values"], plain["values"])
    with pytest.raises(RuntimeError, match=r"dispersion\[2\] \(k_D\) = -1 is not positive"):
        host.particle_likelihood(theta, 8, 2, SEED, dispersion=(1.0, 1.0, -1.0))


def test_exact_likelihood_of_a_tiny_epidemic_on_the_device(mm, ref_fixture):
    """the n = 1 case of tests/test_particle_nb_cpu.py (five people, m = 1, J = 64, k = (0.5, 2, +inf)) on the device: E = 8192
    estimates, every prefix mean of exp(sum of the increments) / Z[k] within 5 standard errors of 1, every standard error at most
    0.05; the first call equals the twin bit for bit"""
    case = TINY["n1"]
    pb = tiny_problem(mm, ref_fixture, case)
    hip = objective(mm, pb, INIT_FIXED)
    theta = np.stack([pb.base_theta] * EXACT_B)
    inc, first = [], None
    for k in range(EXACT_K):
        got = hip.particle_loglik(theta, case.J, case.m, EXACT_SEED + k, want_values=True, want_final=True, dispersion=DISPERSION_EXACT)
        assert not got["status"].any() and got["n_valid"] == EXACT_B
        first = got if first is None else first
        inc.append(got["increments"])
    inc = np.concatenate(inc)
    twin = twin_of(mm, pb, first, case.J, case.m, DISPERSION_EXACT, False, seed=EXACT_SEED)
    same(first, twin, KEYS, "n1")
    mv = first["model_values"]
    assert (mv == mv[0]).all()
    Z = exact_filter_nb(mv[0], case.n, len(pb.beta_end_times), len(pb.kappa_end_times), pb.times, pb.N, pb.M, list(pb.beta_end_times),
                        list(pb.kappa_end_times), case.m, 1, pb.obs_H, pb.obs_ICU, pb.obs_D, DISPERSION_EXACT)
    assert inc.shape == (8192, case.Tp)
    check_prefix_likelihoods("n1 on the device under k = (0.5, 2, inf)", inc, Z)
