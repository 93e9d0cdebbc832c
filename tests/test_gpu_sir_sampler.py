"""Adaptive-Metropolis chains of the age-structured SIR objective resident on the device (sepaihrd_sir_mh_create,
MultiChainMetropolisHastings::optimizeChainsOnDevice on HipPoissonLikelihoodObjective, the calibrator on that objective).

The yardstick is the host loop optimizeChains on the same objective: the reference's algorithm, pinned bit for bit to the
oracle's MetropolisHastingsSampler restatement on the SEPAIHRD path, and both sides evaluate through the same SIR kernel,
whose results do not depend on the batch (tests/test_gpu_sir.py).  So every comparison here is exact equality, in both
arithmetics: no tolerance, no share of chains left out."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRUE = np.array([0.03, 1.0, 0.2, 0.2, 0.15])
ALL = ["q", "scale_C_total", "gamma_0", "gamma_1", "gamma_2"]
RESULT_KEYS = ("accept_trace", "accepted", "samples", "sample_values", "best", "best_value", "final_scale", "final_cov")
RUN = dict(seed=29, iterations=600, burn_in=0, adaptation_period=100, thinning=5)


@pytest.fixture(scope="module")
def pb5(mm, oracle_py):
    return mm.workloads.sir_config0(oracle_py.sir_simulate)


def starts(chains, truth=TRUE, seed=5):
    rng = np.random.default_rng(seed)
    return truth * np.exp(rng.normal(0.0, 0.01, size=(chains, len(truth))))


def assert_same_run(got, want, label):
    for k in RESULT_KEYS:
        assert np.array_equal(got[k], want[k]), (label, k)


def assert_both_branches(res, label):
    """a run in which no chain ever accepts, or every test accepts, exercises one branch of the accept rule only"""
    tr = res["accept_trace"]
    print(f"{label}: accept rate {tr.mean():.3f} (per chain {tr.mean(axis=1).min():.3f} .. {tr.mean(axis=1).max():.3f})")
    assert tr.any() and not tr.all(), label


_host_loop = {}


def host_loop(mm, pb5, arith, two_pass):
    """the host loop's result of RUN on 64 chains (it does not depend on where the streams are drawn: computed once per mode)"""
    key = (arith, two_pass)
    if key not in _host_loop:
        h = mm.HostSIRObjective(pb5.with_(arith=mm.ARITH_FMA if arith == "fma" else mm.ARITH_STRICT))
        _host_loop[key] = h.metropolis_hastings_ex(starts(64), device_state=False, two_pass_covariance=two_pass, **RUN)
    return _host_loop[key]


# ---- 1. device-resident = host loop ----
@pytest.mark.parametrize("two_pass", [False, True], ids=["running", "two_pass"])
@pytest.mark.parametrize("device_streams", [True, False], ids=["device_streams", "host_streams"])
@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_device_resident_run_equals_the_host_loop(mm, pb5, arith, device_streams, two_pass):
    """64 chains x 600 iterations, adaptation period 100 (rank-one updates, five Cholesky refreshes, full recomputes with a
    history of >= P + 10 states), thinning 5."""
    host = host_loop(mm, pb5, arith, two_pass)
    assert_both_branches(host, f"host loop {arith}")
    h = mm.HostSIRObjective(pb5.with_(arith=mm.ARITH_FMA if arith == "fma" else mm.ARITH_STRICT))
    dev = h.metropolis_hastings_ex(starts(64), device_state=True, device_streams=device_streams, two_pass_covariance=two_pass, **RUN)
    assert not dev["fell_back"] and dev["failures"] == [0, 0, 0]
    assert_same_run(dev, host, (arith, device_streams, two_pass))


# ---- 2. packed = block-per-chain, same bits ----
def synthetic_problem(mm, oracle_py, n, seed=7):
    """n age classes, a fixed-seed contact matrix with R0 around 2, Poisson observations of the true incidence
    (tools/bench_sir.py's construction, 121 output days)"""
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


def problem_with_P(mm, oracle_py, pb5, P):
    if P == 1:
        return pb5.with_(param_names=["q"])
    if P == 2:
        return pb5.with_(param_names=["q", "scale_C_total"])
    if P == 5:
        return pb5
    return synthetic_problem(mm, oracle_py, P - 2)


def run_self_contained(mm, lib, hip, x0, cov0, iterations, adaptation_period, thinning, seed, form, diag_first=None):
    """the self-contained sampler (streams, accept test and scale adaptation on the device) through the C ABI, with the
    loop of optimizeChainsOnDevice; everything the device keeps, read back"""
    from mmid_amd import hipabi
    Cn, P = x0.shape
    mh = hipabi.sir_mh_create(lib, hip.ctx, Cn, iterations, x0, cov0, thinning=thinning, adaptation_window=adaptation_period + 1)
    assert mh, lib.sepaihrd_sir_last_error(hip.ctx)
    try:
        assert hipabi.mh_set_kernel_form(lib, mh, form) == 0
        assert form == hipabi.MH_FORM_AUTO or lib.sepaihrd_mh_get_kernel_form(mh) == form

        def ok(rc):
            assert rc == 0, lib.sepaihrd_sir_last_error(hip.ctx)
        lp0, st0 = np.empty(Cn), np.empty(Cn, dtype=np.int32)
        ok(lib.sepaihrd_mh_evaluate_current(mh, lp0.ctypes.data, st0.ctypes.data))
        lp0 = np.where((st0 >= 2) | ~np.isfinite(lp0), -1e18, lp0)
        ok(lib.sepaihrd_mh_keep_scale_on_device(mh, 1, 0.234, 1))
        ok(lib.sepaihrd_mh_set_values(mh, lp0.ctypes.data))
        ok(lib.sepaihrd_mh_seed_streams(mh, seed))

        def adapt_mode(t):  # burn_in 0
            if t % adaptation_period != 0:
                return 1
            return 3 if t >= P + 10 else 2
        ok(lib.sepaihrd_mh_draw_first(mh))
        ones = np.ones(Cn)
        ok(lib.sepaihrd_mh_step(mh, None, ones.ctypes.data, None, None, 0, 10.0 / 101.0, adapt_mode(1)))
        for t in range(1, iterations):
            ok(lib.sepaihrd_mh_step_tested(mh, 10.0 / ((t + 1) + 100.0), adapt_mode(t + 1), 0 if t + 1 < iterations else 1))
        out = {k: np.empty(Cn) for k in ("values", "best_values", "scales")}
        out["accepted"], out["emergency"] = np.empty(Cn, dtype=np.int32), np.empty(Cn, dtype=np.int32)
        ok(lib.sepaihrd_mh_read_run_state(mh, *[out[k].ctypes.data for k in ("values", "best_values", "scales", "accepted", "emergency")]))
        ns = lib.sepaihrd_mh_sample_count(mh)
        out["samples"], out["sample_values"] = np.empty((Cn, ns, P)), np.empty((Cn, ns))
        ok(lib.sepaihrd_mh_read_samples(mh, 0, ns, out["samples"].ctypes.data))
        ok(lib.sepaihrd_mh_read_sample_values(mh, 0, ns, out["sample_values"].ctypes.data))
        out["trace"] = np.empty((iterations - 1, Cn), dtype=np.uint8)
        ok(lib.sepaihrd_mh_read_accept_trace(mh, out["trace"].ctypes.data))
        out["best"], out["proposal"], out["cov"] = np.empty((Cn, P)), np.empty((Cn, P)), np.empty((Cn, P, P))
        ok(lib.sepaihrd_mh_read_best(mh, out["best"].ctypes.data))
        ok(lib.sepaihrd_mh_read_proposal(mh, out["proposal"].ctypes.data))
        ok(lib.sepaihrd_mh_read_covariance(mh, out["cov"].ctypes.data))
        if diag_first is not None:
            d = hipabi.mh_diagnostics(lib, mh, P, Cn, first_sample=diag_first, with_values=True)
            out["diag_table"], out["diag_max_lag"] = d["table"], d["max_lag"]
        return out
    finally:
        lib.sepaihrd_mh_destroy(mh)


@pytest.mark.parametrize("chains", [1, 67, 4099])
@pytest.mark.parametrize("P", [1, 2, 5, 18, 64])
def test_packed_form_gives_the_bits_of_block_per_chain(mm, oracle_py, pb5, P, chains):
    """260 iterations (more than 624 words of every chain's generator per ~20 iterations at P = 5: the state twists
    several times per chain at every P), adaptation period 50: rank-one updates, refreshes and full recomputes on the way.
    Chain counts that do not fill the last wavefront, one chain, one parameter."""
    from mmid_amd import hipabi
    pb = problem_with_P(mm, oracle_py, pb5, P).with_(arith=mm.ARITH_FMA)
    assert pb.n_params == P
    lib = hipabi.load_library()
    hip = mm.HipSIRObjective(pb)
    x0 = starts(chains, truth=pb.current_parameters(), seed=P)
    cov0 = np.diag((0.02 * pb.current_parameters()) ** 2) * (2.38 * 2.38 / P) + 1e-6 * np.eye(P)
    runs = {form: run_self_contained(mm, lib, hip, x0, cov0, 260, 50, 4, 1234, form)
            for form in (hipabi.MH_FORM_BLOCK_PER_CHAIN, hipabi.MH_FORM_PACKED)}
    a, b = runs[hipabi.MH_FORM_BLOCK_PER_CHAIN], runs[hipabi.MH_FORM_PACKED]
    print(f"P = {P}, C = {chains}: accept rate {a['trace'].mean():.3f}")
    assert a["trace"].any() and not a["trace"].all()
    for k in a:
        assert np.array_equal(a[k], b[k]), (P, chains, k)
    hip.close()


def test_packed_form_is_refused_beyond_64_parameters(mm, shipped):
    from mmid_amd import draws, hipabi
    pb = shipped.with_(constraint_mode=mm.CONSTRAINT_REFLECT)
    big = mm.HipObjective(pb)
    lib = hipabi.load_library()

    def sampler(hip, P):
        x0 = np.ones((3, P))
        return hipabi.mh_create(lib, hip.ctx, 3, 8, x0, 1e-4 * np.eye(P))
    mh = hipabi.mh_create(lib, big.ctx, 3, 8, draws.jitter_draws(pb, 1, 3), 1e-6 * np.eye(pb.n_params))
    assert mh
    assert lib.sepaihrd_mh_get_kernel_form(mh) == hipabi.MH_FORM_BLOCK_PER_CHAIN   # AUTO on a SEPAIHRD-backed sampler
    if pb.n_params > 64:
        assert hipabi.mh_set_kernel_form(lib, mh, hipabi.MH_FORM_PACKED) == -4
    else:
        assert hipabi.mh_set_kernel_form(lib, mh, hipabi.MH_FORM_PACKED) == 0
        assert hipabi.mh_set_kernel_form(lib, mh, hipabi.MH_FORM_AUTO) == 0
        assert lib.sepaihrd_mh_get_kernel_form(mh) == hipabi.MH_FORM_BLOCK_PER_CHAIN
    assert hipabi.mh_set_kernel_form(lib, mh, 7) == -1
    lib.sepaihrd_mh_destroy(mh)
    big.close()


def test_packed_form_refused_for_a_66_parameter_sir_problem(mm, oracle_py):
    from mmid_amd import hipabi
    pb = synthetic_problem(mm, oracle_py, 64)
    lib = hipabi.load_library()
    hip = mm.HipSIRObjective(pb)
    P = pb.n_params
    assert P == 66
    mh = hipabi.sir_mh_create(lib, hip.ctx, 2, 4, starts(2, truth=pb.current_parameters()), 1e-6 * np.eye(P))
    assert mh
    assert lib.sepaihrd_mh_get_kernel_form(mh) == hipabi.MH_FORM_BLOCK_PER_CHAIN   # AUTO never picks what cannot run
    assert hipabi.mh_set_kernel_form(lib, mh, hipabi.MH_FORM_PACKED) == -4
    assert b"64" in lib.sepaihrd_sir_last_error(hip.ctx)
    lib.sepaihrd_mh_destroy(mh)
    hip.close()


# ---- 3. the low-level entry points in a mixed call pattern, against the same pattern in host arithmetic ----
def chol_lower(A, add=0.0):
    """mh_cholesky_kernel's recurrences in its order (k ascending, one subtraction per k); None when not positive definite"""
    P = len(A)
    L = [[0.0] * P for _ in range(P)]
    for j in range(P):
        d = float(A[j][j]) + add
        for k in range(j):
            d -= L[j][k] * L[j][k]
        if not d > 0.0:
            return None
        L[j][j] = float(np.sqrt(np.float64(d)))
        for i in range(j + 1, P):
            v = float(A[i][j])
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    return L


def propose_host(x, L, z, scale, lower):
    """prop_i = clamp(x_i + scale * sum_{j <= i} L_ij z_j) with j ascending: the propose kernels' arithmetic in Python floats"""
    P = len(x)
    out = np.empty(P)
    for i in range(P):
        s = 0.0
        for j in range(i + 1):
            s += L[i][j] * float(z[j])
        raw = float(x[i]) + float(scale) * s
        out[i] = lower[i] if raw < lower[i] else raw   # upper = +inf never binds; no -0.0 arises from these states
    return out


@pytest.mark.parametrize("form", ["block_per_chain", "packed"])
def test_entry_points_in_a_mixed_call_pattern_equal_host_arithmetic(mm, pb5, form):
    """propose / fetch / commit / adapt (rank-one updates and one Cholesky refresh), then sepaihrd_mh_step with the caller's
    accept bytes, then sepaihrd_mh_step_tested with the accept test on the device -- on ONE SIR-backed handle, against the
    same pattern restated in Python floats (Cholesky recurrences, L z, the clamp, updateCovarianceRank1, the accept rule) with
    every proposal's value taken from the objective's own batched evaluation."""
    from mmid_amd import hipabi
    pb = pb5.with_(arith=mm.ARITH_STRICT)
    lib = hipabi.load_library()
    hip = mm.HipSIRObjective(pb)
    Cn, P = 9, pb.n_params
    rng = np.random.default_rng(8)
    x0 = starts(Cn)
    cov0 = np.diag((0.03 * TRUE) ** 2) + 1e-6 * np.eye(P)
    reg_eps = 1e-6
    mh = hipabi.sir_mh_create(lib, hip.ctx, Cn, 16, x0, cov0, reg_eps=reg_eps, thinning=2, adaptation_window=4)
    assert mh, lib.sepaihrd_sir_last_error(hip.ctx)
    assert hipabi.mh_set_kernel_form(lib, mh, hipabi.MH_FORM_PACKED if form == "packed" else hipabi.MH_FORM_BLOCK_PER_CHAIN) == 0
    lower, _, _ = hipabi.sir_constraint_bounds(lib, pb.field_map()[0])

    def ok(rc):
        assert rc == 0, lib.sepaihrd_sir_last_error(hip.ctx)
    # ---- the host's copy of the sampler
    x = x0.copy()
    states = [x0.copy()]
    cov = np.repeat(cov0[None], Cn, axis=0)
    mean = x0.copy()
    L = [chol_lower(cov0)] * Cn
    lp = np.empty(Cn)
    ok(lib.sepaihrd_mh_evaluate_current(mh, lp.ctypes.data, None))
    assert np.array_equal(lp, hip.eval_batch(x0)["loglik"])

    def expect_proposal(z, scale):
        return np.stack([propose_host(x[c], L[c], z[c], scale[c], lower) for c in range(Cn)])

    def read_proposal():
        prop = np.empty((Cn, P))
        ok(lib.sepaihrd_mh_read_proposal(mh, prop.ctypes.data))
        return prop

    def commit_host(acc, prop):
        x[:] = np.where(acc[:, None] & 1, prop, x)
        states.append(x.copy())

    def adapt_host(gamma, refresh):
        d = states[-1] - mean
        cov[:] = (1.0 - gamma) * cov + gamma * (d[:, :, None] * d[:, None, :])
        mean[:] += gamma * d
        if refresh:
            for c in range(Cn):
                f = chol_lower(cov[c], reg_eps)
                if f is not None:
                    L[c] = f
    # ---- A: propose / commit / adapt
    pattern = (np.arange(Cn) % 2).astype(np.uint8)
    for acc, adapt in ((pattern, None), (1 - pattern, (0.3, 0)), (pattern, (0.2, 1)), (np.ones(Cn, dtype=np.uint8), (0.1, 0))):
        z, scale = rng.standard_normal((Cn, P)), rng.uniform(0.3, 1.5, Cn)
        ll = np.empty(Cn)
        ok(lib.sepaihrd_mh_propose(mh, z.ctypes.data, scale.ctypes.data, ll.ctypes.data, None))
        prop = read_proposal()
        assert np.array_equal(prop, expect_proposal(z, scale))
        assert np.array_equal(ll, hip.eval_batch(prop)["loglik"])
        acc = np.ascontiguousarray(acc, dtype=np.uint8)
        ok(lib.sepaihrd_mh_commit(mh, acc.ctypes.data))
        commit_host(acc, prop)
        lp = np.where(acc & 1, ll, lp)
        if adapt:
            ok(lib.sepaihrd_mh_adapt(mh, adapt[0], adapt[1], 0))
            adapt_host(*adapt)
    # ---- B: sepaihrd_mh_step (commit with the caller's bytes, adapt, proposal from the staged normals, evaluation)
    pending = None
    for k, (gamma, adapt) in enumerate(((0.15, 1), (0.12, 2), (0.11, 1))):
        z, scale = rng.standard_normal((Cn, P)), rng.uniform(0.3, 1.5, Cn)
        ok(lib.sepaihrd_mh_stage_normals(mh, z.ctypes.data))
        if pending is None:
            ok(lib.sepaihrd_mh_step(mh, None, scale.ctypes.data, None, None, 0, gamma, adapt))
        else:
            prop, ll = pending
            acc = np.ascontiguousarray((np.arange(Cn) + k) % 3 == 0, dtype=np.uint8)
            ok(lib.sepaihrd_mh_step(mh, acc.ctypes.data, scale.ctypes.data, None, None, 0, gamma, adapt))
            commit_host(acc, prop)
            lp = np.where(acc & 1, ll, lp)
        adapt_host(gamma, adapt == 2)
        ll = np.empty(Cn)
        ok(lib.sepaihrd_mh_fetch(mh, ll.ctypes.data, None))
        prop = read_proposal()
        assert np.array_equal(prop, expect_proposal(z, scale)), k
        assert np.array_equal(ll, hip.eval_batch(prop)["loglik"])
        pending = (prop, ll)
    # ---- C: sepaihrd_mh_step_tested: the device tests the pending evaluation with the host's log(u) and picks the normals
    ok(lib.sepaihrd_mh_set_values(mh, lp.ctypes.data))
    best_lp = lp.copy()
    test = np.ctypeslib.as_array(C.cast(lib.sepaihrd_mh_test_buffer(mh), C.POINTER(C.c_double)), shape=(3 * Cn + Cn * P,))
    for k, (gamma, adapt) in enumerate(((0.1, 1), (0.09, 2), (0.08, 1), (0.07, 0))):
        last = k == 3
        prop, ll = pending
        # half the chains get a uniform that accepts a slightly worse proposal, the others one that rejects it
        log_u = np.where(np.arange(Cn) % 2 == 0, -1e-300, -1e300) if k % 2 == 0 else np.log(rng.uniform(size=Cn))
        s_rej, s_acc = rng.uniform(0.3, 1.0, Cn), rng.uniform(1.0, 1.5, Cn)
        z_u, z_p = rng.standard_normal((Cn, P)), rng.standard_normal((Cn, P))
        test[:Cn], test[Cn:2 * Cn], test[2 * Cn:3 * Cn] = log_u, s_rej, s_acc
        test[3 * Cn:] = z_p.ravel()
        if not last:
            ok(lib.sepaihrd_mh_stage_normals(mh, z_u.ctypes.data))
        ok(lib.sepaihrd_mh_step_tested(mh, gamma, adapt, int(last)))
        values, flags = np.empty(Cn), np.empty(Cn, dtype=np.uint8)
        ok(lib.sepaihrd_mh_fetch_test(mh, values.ctypes.data, flags.ctypes.data))
        v = np.where(np.isfinite(ll), ll, -1e18)
        ratio = v - lp
        no_u = ratio >= 0.0
        acc = no_u | (log_u < ratio)
        better = acc & (v > best_lp)
        assert np.array_equal(values, v)
        assert np.array_equal(flags, acc * 1 + better * 2 + no_u * 4), k
        commit_host(acc.astype(np.uint8), prop)
        lp = np.where(acc, v, lp)
        best_lp = np.where(better, v, best_lp)
        if last:
            break
        if adapt >= 1:
            adapt_host(gamma, adapt == 2)
        scale = np.where(acc, s_acc, s_rej)
        prop = read_proposal()
        assert np.array_equal(prop, expect_proposal(np.where(no_u[:, None], z_p, z_u), scale)), k
        ll = np.empty(Cn)
        ok(lib.sepaihrd_mh_fetch(mh, ll.ctypes.data, None))
        assert np.array_equal(ll, hip.eval_batch(prop)["loglik"])
        pending = (prop, ll)
    assert np.any(flags & 1) and not np.all(flags & 1)
    # ---- what the device kept
    got = np.empty((Cn, P, P))
    ok(lib.sepaihrd_mh_read_covariance(mh, got.ctypes.data))
    assert np.array_equal(got, cov)
    hist = np.stack(states, axis=1)
    n_states = hist.shape[1]
    assert lib.sepaihrd_mh_history_length(mh) == n_states
    ns = lib.sepaihrd_mh_sample_count(mh)
    assert ns == (n_states - 1) // 2 + 1
    kept = np.empty((Cn, ns, P))
    ok(lib.sepaihrd_mh_read_samples(mh, 0, ns, kept.ctypes.data))
    assert np.array_equal(kept, hist[:, ::2])
    vals, bests = np.empty(Cn), np.empty(Cn)
    ok(lib.sepaihrd_mh_read_run_state(mh, vals.ctypes.data, bests.ctypes.data, None, None, None))
    assert np.array_equal(vals, lp) and np.array_equal(bests, best_lp)
    assert lib.sepaihrd_mh_busy(mh) == 0
    lib.sepaihrd_mh_destroy(mh)
    hip.close()


# ---- 4. failures ----
@pytest.mark.parametrize("device_streams", [True, False], ids=["device_streams", "host_streams"])
def test_failed_evaluations_enter_the_test_as_in_the_host_loop(mm, pb5, device_streams):
    kw = dict(seed=3, iterations=120, burn_in=0, adaptation_period=40, thinning=3)
    x0 = starts(33)
    # the attempt budget: every evaluation has status 3
    pb = pb5.with_(max_attempts=5)
    host = mm.HostSIRObjective(pb).metropolis_hastings_ex(x0, device_state=False, **kw)
    dev = mm.HostSIRObjective(pb).metropolis_hastings_ex(x0, device_state=True, device_streams=device_streams, **kw)
    assert_same_run(dev, host, "status 3")
    assert np.all(dev["sample_values"] == -1e18) and np.all(dev["best_value"] == -1e18)
    # every tested proposal failed: one per chain and test
    assert dev["failures"] == [0, 33 * (kw["iterations"] - 1), 0]
    # a non-finite observation: every value is -inf with status 1 -- not a failed integration, so nothing is counted
    obs = pb5.obs.copy()
    obs[17, 1] = np.inf
    pb = pb5.with_(obs=obs)
    vals, st = mm.HostSIRObjective(pb).calculate_batch(x0)
    assert np.all(np.isneginf(vals)) and np.all(st == 1)
    host = mm.HostSIRObjective(pb).metropolis_hastings_ex(x0, device_state=False, **kw)
    dev = mm.HostSIRObjective(pb).metropolis_hastings_ex(x0, device_state=True, device_streams=device_streams, **kw)
    assert_same_run(dev, host, "status 1")
    assert dev["failures"] == [0, 0, 0]


# ---- 5. diagnostics on the resident samples ----
def test_diagnostics_of_the_resident_sir_samples(mm, pb5):
    """sepaihrd_mh_diagnostics on a SIR-backed handle against diagnostics.py's numpy restatement on the samples read back;
    the bars are those of tests/test_gpu_chain_diagnostics.py: mean and sd to 1e-12, the other columns to 1e-9 (relative), the
    same NaN pattern, the same truncation lags.  The run's compute_diagnostics key gives the same table."""
    from mmid_amd import hipabi
    pb = pb5.with_(arith=mm.ARITH_FMA)
    lib = hipabi.load_library()
    hip = mm.HipSIRObjective(pb)
    P, burn, thinning, iters = pb.n_params, 200, 2, 1400
    first = burn // thinning + 1
    cov0 = np.diag((0.02 * TRUE) ** 2) * (2.38 * 2.38 / P) + 1e-6 * np.eye(P)
    run = run_self_contained(mm, lib, hip, starts(64), cov0, iters, 100, thinning, 41, hipabi.MH_FORM_AUTO, diag_first=first)
    want = mm.diagnostics.chain_diagnostics(run["samples"][:, first:], run["sample_values"][:, first:])
    g, w = run["diag_table"], want["table"]
    assert g.shape == w.shape == (P + 1, 7)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    okm = ~np.isnan(w)
    rel = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
    print("max relative difference per column:", np.nanmax(np.where(okm, rel, np.nan), axis=0))
    assert np.all(rel[:, :2][okm[:, :2]] <= 1e-12), rel[:, :2]
    assert np.all(rel[:, 2:][okm[:, 2:]] <= 1e-9), rel[:, 2:]
    assert np.array_equal(run["diag_max_lag"], want["max_lag"])
    assert np.all(np.isfinite(g[:, 6]))
    hip.close()
    # the host layer's key: a table over the samples after burn-in of ITS run, formed from the resident store
    h = mm.HostSIRObjective(pb)
    res = h.metropolis_hastings_ex(starts(16), seed=41, iterations=300, burn_in=100, adaptation_period=100, thinning=thinning,
                                   device_state=True, compute_diagnostics=True)
    f2 = 100 // thinning + 1
    w2 = mm.diagnostics.chain_diagnostics(res["samples"][:, f2:], res["sample_values"][:, f2:])["table"]
    assert res["diagnostics"] is not None and res["diagnostics"].shape == w2.shape
    np.testing.assert_allclose(res["diagnostics"][:, :2], w2[:, :2], rtol=1e-12)
    np.testing.assert_allclose(res["diagnostics"][:, 2:], w2[:, 2:], rtol=1e-9)


# ---- 6. libm fall-back ----
def test_libm_fallback_keeps_the_streams_on_the_host_and_the_result(mm, pb5, tmp_path):
    """SEPAIHRD_LIBM_SELFCHECK=fail makes the self-check report a foreign libm: a fresh process (the result of the check is
    kept per context, the hook is read when it runs) must report the fall-back and give the host loop's result."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "fallback.py"
    out = tmp_path / "fallback.npz"
    script.write_text(f"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'oracle')!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
import numpy as np
import mmid_amd_loader, oracle_py
import test_gpu_sir_sampler as t
mm = mmid_amd_loader.load()
oracle_py.load()
pb = mm.workloads.sir_config0(oracle_py.sir_simulate)
from mmid_amd import hipabi
hip = mm.HipSIRObjective(pb)
assert hip.device_libm_check() != (0, 0)
lib = hipabi.load_library()
mh = hipabi.sir_mh_create(lib, hip.ctx, 4, 8, t.starts(4), 1e-6 * np.eye(5))
assert lib.sepaihrd_mh_seed_streams(mh, 1) == -4 and lib.sepaihrd_mh_keep_scale_on_device(mh, 1, 0.234, 0) == -4
assert b"libm" in lib.sepaihrd_sir_last_error(hip.ctx)
lib.sepaihrd_mh_destroy(mh)
res = mm.HostSIRObjective(pb).metropolis_hastings_ex(t.starts(64), device_state=True, device_streams=True, **t.RUN)
np.savez({str(out)!r}, fell_back=res['fell_back'], **{{k: res[k] for k in t.RESULT_KEYS}})
""")
    env = dict(os.environ, SEPAIHRD_LIBM_SELFCHECK="fail")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    assert bool(got["fell_back"])
    assert_same_run(got, host_loop(mm, pb5, "strict", False), "libm fall-back")


# ---- 7. calibration end to end ----
def test_two_phase_calibration_recovers_the_likelihood_of_the_truth(mm, pb5):
    """Start 30 % off, Hill-Climbing, then 64 device-resident chains x 2000 iterations.  The true parameters are a fixed point
    of the data-generating process, so the maximum cannot lie below their value; 5 log units is slack for an unconverged
    climb, not a measurement (the bar and the reasoning of tests/test_gpu_sir.py's host-loop calibration test).  Chain 0 of the
    multi-chain run is the single chain of a chains = 1 run with the same seeds."""
    start = TRUE * np.array([1.3, 0.7, 1.3, 0.7, 1.3])
    pb = pb5.with_(q=start[0], scale_C_total=start[1], gamma=start[2:])
    ll_true = mm.HostSIRObjective(pb5).calculate(TRUE)
    kw = dict(hc_seed=11, mh_seed=17, hc_iterations=300, mh_iterations=2000, burn_in=0, thinning=10)
    h = mm.HostSIRObjective(pb)
    assert np.array_equal(h.manager_info()["current"], start)
    many = h.calibrate(chains=64, **kw)
    print(f"ll(true) {ll_true:.3f}, ll(start) {many['initial_value']:.3f}, phase 1 {many['phase1_best_value']:.3f}, best {many['best_value']:.3f}, "
          f"accept rate {many['accept_trace'].mean():.3f}")
    assert np.isfinite(ll_true) and many["best_value"] >= ll_true - 5.0
    assert many["phase1_best_value"] >= many["initial_value"]
    # the objective value of every stored sample is the value the chain carried there
    assert np.array_equal(many["mcmc_objective_values"], many["sample_values"])
    assert many["accept_trace"].any() and not many["accept_trace"].all()
    one = mm.HostSIRObjective(pb).calibrate(chains=1, **kw)
    assert one["phase1_best_value"] == many["phase1_best_value"] and np.array_equal(one["phase2_cov"], many["phase2_cov"])
    assert np.array_equal(one["accept_trace"][0], many["accept_trace"][0])
    assert np.array_equal(one["samples"][0], many["samples"][0]) and np.array_equal(one["sample_values"][0], many["sample_values"][0])


# ---- 8. progress reports and checkpoints ----
def test_reports_and_checkpoints_of_a_sir_run(mm, pb5, tmp_path):
    """The Reporter is model-independent: a progress line every report_interval iterations, posterior_trace_final.csv with every
    stored sample of chain 0, and a checkpoint file that is a prefix of it."""
    out_dir, log = tmp_path / "mcmc", tmp_path / "progress.log"
    out_dir.mkdir()
    h = mm.HostSIRObjective(pb5)
    res = h.metropolis_hastings_ex(starts(8), seed=5, iterations=400, burn_in=50, adaptation_period=100, thinning=4, device_state=True,
                                   out_dir=str(out_dir), log_path=str(log), report_interval=100, want_trace=False)
    lines = [ln for ln in log.read_text().splitlines() if "Iter:" in ln]
    assert len(lines) >= 3 and all("LogPost:" in ln and "AccRate:" in ln for ln in lines)

    def rows(name):
        body = (out_dir / name).read_text().strip().splitlines()[1:]
        return np.array([[float(v) for v in ln.split(",")] for ln in body])
    final = rows("posterior_trace_final.csv")
    assert final.shape[0] == res["samples"].shape[1]
    # rows `i,value,theta...` printed with seven significant digits
    assert np.array_equal(final[:, 0], np.arange(final.shape[0]))
    np.testing.assert_allclose(final[:, 1], res["sample_values"][0], rtol=1e-6)
    np.testing.assert_allclose(final[:, 2:], res["samples"][0], rtol=1e-6)
    ck = rows("posterior_trace_checkpoint.csv")
    assert 0 < ck.shape[0] <= final.shape[0] and np.array_equal(ck, final[:ck.shape[0]])
