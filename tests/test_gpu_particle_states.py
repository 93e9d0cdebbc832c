"""The per-row summaries of the particle filter on the device (sepaihrd_particle_filter_states: the wide form's launches with every
output row a segment, a gather launch and a sort-and-pick launch after each) against the host twin bit for bit, against the wide
form's own outputs, on a cut grid, across chunkings and arithmetic modes, with the argument rules, through the C++ adapter, and
against the exact filtering moments of a tiny epidemic.  The twin is fed the device's own model values and status."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_particle_filter import SEED, T, max_particles, three_thetas
from test_gpu_particle_filter_exact import tiny_problem
from test_gpu_particle_filter_wide import WIDE_MAX, problem
from test_gpu_stochastic_sepaihrd import INIT_FIXED, INIT_FROM_THETA, objective
from test_particle_filter_cpu import DBL_MAX
from test_particle_filter_exact_cpu import CASES, ESTIMATES, SEED as EXACT_SEED
from test_particle_states_cpu import DISPERSION, PROBS, check_exact_case, numpy_stats, same

pytestmark = pytest.mark.gpu

FILTER_KEYS = ("loglik", "increments", "ess", "model_values", "status")
STATE_KEYS = ("loglik", "increments", "ess", "state_mean", "state_quantiles")


def twin_of(mm, pb, got, J, m, probs=PROBS, dispersion=None, seed=SEED):
    return mm.hostabi.particle_states_from_values(got["model_values"], got["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H, pb.obs_ICU,
                                                  pb.obs_D, J, m, seed, probs, beta_end_times=pb.beta_end_times, dispersion=dispersion)


def check_three(got):
    """three_thetas: a valid vector, one with beta clamped onto its bound, a rejected one"""
    assert list(got["status"]) == [0, 0, 1] and got["n_valid"] == 2 and got["loglik"][2] == -DBL_MAX
    assert np.isnan(got["state_mean"][2]).all() and np.isnan(got["state_quantiles"][2]).all()
    assert np.isfinite(got["state_mean"][:2]).all() and np.isfinite(got["state_quantiles"][:2]).all()
    assert not got["increments"][:2, 4].any() and np.isnan(got["ess"][:2, 4]).all()  # the blank row


# (n, m, J): the shapes of the wide form's tests; the first J above the LDS kernel's limit of every n (465, 137, 36); 1025, the
# first J whose scans leave LDS; J lpc is no multiple of 64 except at (16, 36)
SHAPES = [(1, 1, 1), (3, 3, 17), (3, 1, 129), (16, 1, 35), (1, 1, 465), (3, 3, 137), (16, 3, 36), (3, 1, 1025)]


@pytest.mark.parametrize("dispersion", [None, DISPERSION])
@pytest.mark.parametrize("runup", [2, 0])
@pytest.mark.parametrize("n,m,J", SHAPES)
def test_device_equals_twin(mm, ref_fixture, n, m, J, runup, dispersion):
    """every output against the twin; the filter's outputs against the wide call on the device; row T - 1 against the numpy
    statistics of that call's final state"""
    if J in (465, 137, 36):
        assert J == max_particles(mm, n) + 1
    pb = problem(mm, ref_fixture, n, m, runup)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)
    got = hip.particle_filter_states(theta, J, m, SEED, PROBS, dispersion=dispersion, want_values=True)
    check_three(got)
    twin = twin_of(mm, pb, got, J, m, dispersion=dispersion)
    for key in STATE_KEYS:
        assert same(got[key], twin[key]), key
    wide = hip.particle_loglik_wide(theta, J, m, SEED, want_final=True, want_values=True, dispersion=dispersion)
    for key in FILTER_KEYS:
        assert same(got[key], wide[key]), key
    assert got["n_valid"] == wide["n_valid"]
    mean, quant = numpy_stats(wide["final_state"], PROBS)
    assert same(got["state_mean"][:, T - 1], mean) and same(got["state_quantiles"][:, T - 1], quant)
    ms = hip.particle_states_timing()
    assert ms.shape == (3,) and (ms > 0).all() and ms[2] < ms[1]
    print(f"n {n} m {m} J {J} runup {runup} dispersion {dispersion}: decode {ms[0]:.3f} launches {ms[1]:.3f} of which summaries {ms[2]:.3f} ms; "
          f"the wide call {hip.particle_wide_timing()[1]:.3f} ms")


@pytest.mark.parametrize("dispersion", [None, DISPERSION])
@pytest.mark.parametrize("runup", [2, 0])
@pytest.mark.parametrize("J", [16384, 16385])
def test_the_largest_lds_segment_and_the_first_sorted_in_device_memory(mm, ref_fixture, J, runup, dispersion):
    """runup = 0: the run's first row is weighted, so the first summary already goes through the ancestors"""
    n, m = 1, 1
    pb = problem(mm, ref_fixture, n, m, runup)
    assert (pb.times[0] == 0.0) == (runup == 0)
    hip = objective(mm, pb)
    theta = three_thetas(mm, pb)[1:]  # B = 2: the vector at its bound and the rejected one
    got = hip.particle_filter_states(theta, J, m, SEED, PROBS, dispersion=dispersion, want_values=True)
    assert list(got["status"]) == [0, 1] and np.isnan(got["state_mean"][1]).all() and np.isfinite(got["state_quantiles"][0]).all()
    twin = twin_of(mm, pb, got, J, m, dispersion=dispersion)
    for key in STATE_KEYS:
        assert same(got[key], twin[key]), key
    q = got["state_quantiles"][0]
    assert (np.diff(q, axis=-1) >= 0).all() and (q[..., 0] < q[..., -1]).any()
    print(f"J {J} runup {runup}: {hip.particle_states_timing()} ms")


def test_one_cut_grid(mm, ref_fixture):
    """row k = 4 of the whole grid is the final state of a context built on the problem cut after row 4"""
    n, m, J, k = 3, 3, 17, 4
    pb = problem(mm, ref_fixture, n, m)
    theta = three_thetas(mm, pb)
    got = objective(mm, pb).particle_filter_states(theta, J, m, SEED, PROBS)
    runup = int(np.sum(pb.times < 0))
    cut = pb.with_(times=pb.times[:k + 1], obs_H=pb.obs_H[:k + 1 - runup], obs_ICU=pb.obs_ICU[:k + 1 - runup], obs_D=pb.obs_D[:k + 1 - runup])
    hip = objective(mm, cut)
    fin = hip.particle_loglik_wide(theta, J, m, SEED, want_final=True)
    mean, quant = numpy_stats(fin["final_state"], PROBS)
    assert same(got["state_mean"][:, k], mean) and same(got["state_quantiles"][:, k], quant)
    assert same(got["increments"][:, :k + 1 - runup], fin["increments"])
    short = hip.particle_filter_states(theta, J, m, SEED, PROBS)
    assert same(short["state_mean"], got["state_mean"][:, :k + 1]) and same(short["state_quantiles"], got["state_quantiles"][:, :k + 1])


def test_the_chunking_the_probabilities_and_the_outputs_asked_for_do_not_change_a_result(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = np.concatenate([three_thetas(mm, pb), mm.draws.jitter_draws(pb, 12, 2)])
    J, m = 150, 2
    runs = {chunk: hip.particle_filter_states(theta, J, m, SEED, PROBS, theta_chunk=chunk) for chunk in (1, 2, 5, 0)}
    assert list(runs[0]["status"]) == [0, 0, 1, 0, 0]
    for chunk in (1, 2, 5):
        for key in STATE_KEYS + ("status",):
            assert same(runs[chunk][key], runs[0][key]), (chunk, key)
    # an invalid vector in front of a valid one, one theta per chunk
    holes = hip.particle_filter_states(theta[[2, 1]], J, m, SEED, PROBS, theta_chunk=1)
    assert list(holes["status"]) == [1, 0] and np.isnan(holes["state_mean"][0]).all() and np.isnan(holes["state_quantiles"][0]).all()
    assert same(holes["state_mean"][1], runs[0]["state_mean"][1]) and same(holes["state_quantiles"][1], runs[0]["state_quantiles"][1])
    # no probabilities; 64 of them; fewer outputs
    lean = hip.particle_filter_states(theta[:2], J, m, SEED, want_increments=False, want_ess=False)
    assert "state_quantiles" not in lean and "ess" not in lean and same(lean["state_mean"], runs[0]["state_mean"][:2])
    many = np.linspace(0.0, 1.0, 64)
    full = hip.particle_filter_states(theta[:2], J, m, SEED, many, want_values=True)
    twin = twin_of(mm, pb, full, J, m, probs=many)
    assert same(full["state_quantiles"], twin["state_quantiles"]) and same(full["state_mean"], runs[0]["state_mean"][:2])
    assert same(full["state_quantiles"][..., 0], runs[0]["state_quantiles"][:2, ..., 0])
    assert same(full["state_quantiles"][..., 63], runs[0]["state_quantiles"][:2, ..., 4])


def test_arithmetic_mode_does_not_change_the_result(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    J = max_particles(mm, 4) + 64
    a = objective(mm, pb, arith=mm.ARITH_STRICT).particle_filter_states(theta, J, 2, SEED, PROBS, want_values=True)
    b = objective(mm, pb, arith=mm.ARITH_FMA).particle_filter_states(theta, J, 2, SEED, PROBS, want_values=True)
    for key in STATE_KEYS + ("model_values", "status"):
        assert same(a[key], b[key]), key


def test_argument_errors_leave_the_outputs_untouched(mm, ref_fixture):
    pb = problem(mm, ref_fixture, 4)
    hip = objective(mm, pb)
    theta = np.ascontiguousarray(three_thetas(mm, pb))
    n, Tp = 4, T - 2
    good = np.array(PROBS)

    def call(B=3, J=8, m=2, chunk=0, disp=None, probs=good, n_probs=None, want_q=True, ctx=None, want_mean=True):
        ll, inc, ess = np.full(3, -7.0), np.full((3, Tp), -7.0), np.full((3, Tp), -7.0)
        mean, quant = np.full((3, T, 11, n + 1), -7.0), np.full((3, T, 11, n + 1, 8), -7.0)
        status, nv = np.full(3, -7, dtype=np.int32), C.c_int32(-7)
        pr = None if probs is None else np.ascontiguousarray(probs, dtype=np.float64)
        dp = None if disp is None else np.ascontiguousarray(disp, dtype=np.float64)
        rc = hip.lib.sepaihrd_particle_filter_states(hip.ctx if ctx is None else ctx, theta.ctypes.data, B, J, m, SEED, chunk,
                                                     None if dp is None else dp.ctypes.data, None if pr is None else pr.ctypes.data,
                                                     (0 if pr is None else pr.size) if n_probs is None else n_probs, ll.ctypes.data, inc.ctypes.data,
                                                     ess.ctypes.data, mean.ctypes.data if want_mean else None, quant.ctypes.data if want_q else None, None,
                                                     status.ctypes.data, C.byref(nv))
        untouched = all((a == -7).all() for a in (ll, inc, ess, mean, quant, status)) and nv.value == -7
        return rc, untouched, hip.lib.sepaihrd_last_error(hip.ctx if ctx is None else ctx).decode()

    for kw, word in ((dict(B=0), "B must be >= 1"), (dict(J=0), "J must lie in [1, 65536]"), (dict(J=WIDE_MAX + 1), "J must lie in [1, 65536]"),
                     (dict(chunk=-1), "theta_chunk must be >= 0"), (dict(m=0), "steps_per_interval must be >= 1"),
                     (dict(B=2 ** 15, J=WIDE_MAX), "B x J must stay below 2^31"), (dict(n_probs=65), "n_probs must lie in [0, 64]"),
                     (dict(n_probs=-1), "n_probs must lie in [0, 64]"), (dict(probs=None, n_probs=2), "n_probs > 0 needs probs"),
                     (dict(probs=[0.5, np.nan]), "every probability must lie in [0, 1]"), (dict(probs=[1.0000001]), "every probability must lie in [0, 1]"),
                     (dict(probs=None), "state_quantiles needs n_probs > 0"), (dict(want_mean=False), "need theta, loglik and state_mean"),
                     (dict(B=2 ** 20, J=1024, chunk=2 ** 20), "device memory")):
        rc, untouched, msg = call(**kw)
        assert rc == -1 and untouched and word in msg and msg.startswith("particle_filter_states: "), (kw, rc, msg)
    rc, untouched, msg = call(disp=[0.5, -1.0, 8.0])
    assert rc == -1 and untouched and "dispersion[1]" in msg
    f32 = objective(mm, pb)
    f32.set_precision(mm.PRECISION_F32)
    rc, untouched, msg = call(ctx=f32.ctx)
    assert rc == -4 and untouched and "fp64" in msg
    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    assert call(probs=None, want_q=False)[0] == 0 and call(probs=[0.0, 1.0])[0] == 0
    # the wide form's messages are where they were
    with pytest.raises(RuntimeError, match=r"particle_loglik_wide: J must lie in \[1, 65536\]"):
        hip.particle_loglik_wide(theta, WIDE_MAX + 1, 2, SEED)


def test_cpp_adapter_filter_states(mm, ref_fixture):
    """HipParticleLikelihood::filterStates is sepaihrd_particle_filter_states at the seed of the next calculateBatch, under the
    dispersion set, and leaves that call's seed alone"""
    pb = problem(mm, ref_fixture, 4)
    theta = three_thetas(mm, pb)
    J = max_particles(mm, 4) + 50
    host = mm.hostabi.HostObjective(pb)
    hip = objective(mm, pb, INIT_FROM_THETA)
    for disp in (None, DISPERSION):
        via = host.particle_filter_states(theta, J, 2, SEED, PROBS, n_calls_before=1, initial_state_mode=INIT_FROM_THETA, dispersion=disp)
        assert list(via["calls"]) == [1, 1]
        direct = hip.particle_filter_states(theta, J, 2, SEED + 1, PROBS, dispersion=disp, want_values=True)
        for key in ("state_mean", "state_quantiles", "loglik"):
            assert same(via[key], direct[key]), (disp, key)
        twin = twin_of(mm, pb, direct, J, 2, dispersion=disp, seed=SEED + 1)
        assert same(via["state_mean"], twin["state_mean"]) and same(via["state_quantiles"], twin["state_quantiles"])
        nxt = hip.particle_loglik_wide(theta, J, 2, SEED + 1, dispersion=disp)
        assert same(via["next_values"], nxt["loglik"]) and same(via["next_values"], via["loglik"])


def test_the_exact_case_n1_on_the_device(mm, ref_fixture):
    """the CPU test's assertions on the device's estimates, and the first call against the twin"""
    name = "n1"
    case = CASES[name]
    pb = tiny_problem(mm, ref_fixture, case)
    hip = objective(mm, pb, INIT_FIXED)
    B, K = ESTIMATES[name]
    theta = np.stack([pb.base_theta] * B)
    runs = [hip.particle_filter_states(theta, case.J, case.m, EXACT_SEED + k, (1.0,), want_values=(k == 0)) for k in range(K)]
    assert all(not r["status"].any() for r in runs)
    twin = twin_of(mm, pb, runs[0], case.J, case.m, probs=(1.0,), seed=EXACT_SEED)
    for key in STATE_KEYS:
        assert same(runs[0][key], twin[key]), key
    mv = runs[0]["model_values"]
    assert (mv == mv[0]).all()
    check_exact_case(name, np.concatenate([r["increments"] for r in runs]), np.concatenate([r["state_mean"] for r in runs]),
                     np.concatenate([r["state_quantiles"][..., 0] for r in runs]), mm, row=mv[0])
