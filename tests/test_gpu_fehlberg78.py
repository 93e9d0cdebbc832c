"""Fehlberg 7(8) on the GPU (SEPAIHRD_SOLVER_FEHLBERG78 / FehlbergSolverStrategy).

The CPU oracle restates only Dopri5 and Cash-Karp, so this file carries its own reference: a plain-float restatement of
Boost.Odeint's integrate_times over controlled_runge_kutta<generic explicit RK> (not FSAL), driven by the oracle's
right-hand side.  It is proven first: with the Cash-Karp tableau it reproduces the oracle's Cash-Karp chain by chain, and
its likelihood step reproduces the oracle's.  Then the same driver with the Fehlberg 7(8) tableau is the reference for the
kernel.
"""
import math
from fractions import Fraction as F

import numpy as np
import pytest

from test_fehlberg78_cpu import A as F78_A, B as F78_B, BHAT as F78_BHAT, C as F78_C

pytestmark = pytest.mark.gpu

FORM_QUAD = 2
PRECISION_F32 = 1
LL_INLINE, LL_SEPARATE_PASS = 0, 1

CK_C = [F(0), F(1, 5), F(3, 10), F(3, 5), F(1), F(7, 8)]
CK_A = [[], [F(1, 5)], [F(3, 40), F(9, 40)], [F(3, 10), F(-9, 10), F(6, 5)], [F(-11, 54), F(5, 2), F(-70, 27), F(35, 27)],
        [F(1631, 55296), F(175, 512), F(575, 13824), F(44275, 110592), F(253, 4096)]]
CK_B = [F(37, 378), F(0), F(250, 621), F(125, 594), F(0), F(512, 1771)]
CK_BHAT = [F(2825, 27648), F(0), F(18575, 48384), F(13525, 55296), F(277, 14336), F(1, 4)]


class Tableau:
    """Coefficients as Boost holds them: each one quotient rounded once; the error weights are b - bhat in doubles."""

    def __init__(self, c, a, b, bhat, order, error_order):
        self.c = [float(v) for v in c]
        self.a = [[float(v) for v in row] for row in a]
        self.b = [float(v) for v in b]
        self.db = [float(x) - float(y) for x, y in zip(b, bhat)]
        self.order, self.error_order = order, error_order


CASH_KARP = Tableau(CK_C, CK_A, CK_B, CK_BHAT, 5, 4)
FEHLBERG78 = Tableau(F78_C, F78_A, F78_B, F78_BHAT, 8, 7)


def _scale_sum(first, terms):
    """first + f1 k1 + f2 k2 + ... left to right (zero factors left out, as the kernels do)"""
    acc = first
    for f, k in terms:
        if f != 0.0:
            acc = f * k if acc is None else acc + f * k
    return acc


def integrate_times(tab, rhs, x0, times, dt, abs_tol, rel_tol, max_attempts=1_000_000):
    """integrate_times(make_controlled(abs, rel, stepper), sys, x, times, dt, observer) -> (rows, accepted, rejected, status)"""
    x = np.array(x0, dtype=np.float64)
    rows = [x.copy()]
    acc = rej = attempts = fails = 0
    for k in range(1, len(times)):
        t_end = times[k]
        t = times[k - 1]
        while (t_end - t) > np.finfo(np.float64).eps:
            cur = min(dt, t_end - t)
            if attempts >= max_attempts:
                return rows, acc, rej, 3
            attempts += 1
            ks = [rhs(x, t)]
            for i in range(1, len(tab.c)):
                xt = _scale_sum(1.0 * x, [(tab.a[i][j] * cur, ks[j]) for j in range(i)])
                ks.append(rhs(xt, t + tab.c[i] * cur))
            xnew = _scale_sum(1.0 * x, [(tab.b[j] * cur, ks[j]) for j in range(len(ks))])
            xerr = _scale_sum(None, [(tab.db[j] * cur, ks[j]) for j in range(len(ks))])
            a_dxdt = 1.0 * cur
            err = float(np.max(np.abs(xerr) / (abs_tol + rel_tol * (1.0 * np.abs(x) + a_dxdt * np.abs(ks[0])))))
            if err > 1.0:  # default_step_adjuster::decrease_step
                cur *= max(9.0 / 10.0 * math.pow(err, -1.0 / (tab.error_order - 1)), 1.0 / 5.0)
                rej += 1
                if fails >= 500:
                    return rows, acc, rej, 2
                fails += 1
                dt = cur
                continue
            t += cur
            x = xnew
            if err < 0.5:  # increase_step
                e = max(math.pow(5.0, -float(tab.order)), err)
                cur *= 9.0 / 10.0 * math.pow(e, -1.0 / tab.order)
            acc += 1
            fails = 0
            dt = max(dt, cur)
        t = t_end
        rows.append(x.copy())
    return rows, acc, rej, 0


def loglik_from_trajectory(oracle_py, pb, traj):
    """SEPAIHRDObjectiveFunction: daily incidence of D, CumH, CumICU (cwiseMax(0)), the bottom n_obs rows, three Poisson
    sums; traj: T x 11n, row 0 the initial state."""
    n = pb.n
    inc = np.diff(traj, axis=0, prepend=traj[:1])
    inc = np.maximum(inc, 0.0)
    obs_H, obs_ICU, obs_D = (np.asarray(o, dtype=np.float64) for o in (pb.obs_H, pb.obs_ICU, pb.obs_D))
    rows = obs_H.shape[0]
    off = traj.shape[0] - rows
    h = oracle_py.poisson_loglik(inc[off:, 9 * n:10 * n], obs_H)
    i = oracle_py.poisson_loglik(inc[off:, 10 * n:11 * n], obs_ICU)
    d = oracle_py.poisson_loglik(inc[off:, 8 * n:9 * n], obs_D)
    return h + i + d


def restate(oracle_py, pb, theta, tab):
    """The driver on chain theta: initial state from row 0 of an oracle trajectory, RHS from the oracle."""
    orc = oracle_py.Oracle(pb.with_(solver=0))
    x0 = orc.eval_batch(theta[None, :], want_traj=True)["traj"][0][0]
    rows, acc, rej, status = integrate_times(tab, lambda x, t: orc.rhs(x, t, theta), x0, list(pb.times), pb.dt_hint,
                                             pb.abs_err, pb.rel_err)
    traj = np.array(rows)
    ll = loglik_from_trajectory(oracle_py, pb, traj) if status == 0 else None
    return {"traj": traj, "n_accept": acc, "n_reject": rej, "status": status, "loglik": ll}


def rel_err(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max())


def short(pb, days=120):
    pb.times = pb.times[:days]
    keep = days - 20
    return pb.with_(obs_H=pb.obs_H[:keep], obs_ICU=pb.obs_ICU[:keep], obs_D=pb.obs_D[:keep])


def jitter(mm, pb, B, seed=3):
    from mmid_amd import draws
    th = draws.jitter_draws(pb, seed, B)
    th[0] = pb.base_theta
    return th


# ---------------------------------------------------------------- 1. the driver itself
def test_driver_reproduces_the_oracle_cash_karp(mm, oracle_py, shipped):
    pb = shipped.with_(solver=mm.SOLVER_CASH_KARP54, arith=mm.ARITH_STRICT)
    theta = jitter(mm, pb, 3, seed=7)
    ref = oracle_py.Oracle(pb).eval_batch(theta, want_traj=True)
    for b in range(len(theta)):
        got = restate(oracle_py, pb, theta[b], CASH_KARP)
        assert got["status"] == ref["status"][b] == 0
        assert (got["n_accept"], got["n_reject"]) == (ref["n_accept"][b], ref["n_reject"][b]), b
        assert rel_err(got["traj"], ref["traj"][b]) <= 1e-12
        assert abs(got["loglik"] - ref["loglik"][b]) <= 1e-12 * abs(ref["loglik"][b])


def test_driver_likelihood_reproduces_the_oracle(mm, oracle_py, shipped, ref_fixture):
    for pb in (shipped.with_(solver=0), ref_fixture.with_(solver=0)):
        theta = jitter(mm, pb, 2, seed=5)
        ref = oracle_py.Oracle(pb).eval_batch(theta, want_traj=True)
        for b in range(len(theta)):
            ll = loglik_from_trajectory(oracle_py, pb, ref["traj"][b])
            assert abs(ll - ref["loglik"][b]) <= 1e-12 * abs(ref["loglik"][b])


# ---------------------------------------------------------------- 2. strict parity
def _check_strict(oracle_py, pb, got, theta, idx):
    for b in idx:
        want = restate(oracle_py, pb, theta[b], FEHLBERG78)
        assert want["status"] == got["status"][b] == 0, b
        assert (got["n_accept"][b], got["n_reject"][b]) == (want["n_accept"], want["n_reject"]), b
        if "traj" in got:
            assert rel_err(got["traj"][b], want["traj"]) <= 1e-9, b
        assert abs(got["loglik"][b] - want["loglik"]) <= 1e-10 * abs(want["loglik"]), b


@pytest.mark.parametrize("fixture_name", ["shipped", "ref_fixture", "synth400"])
def test_strict_matches_the_restatement(mm, oracle_py, request, fixture_name):
    pb = request.getfixturevalue(fixture_name).with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_STRICT)
    B = 37 if fixture_name != "ref_fixture" else 21  # ragged: not a multiple of the chains per wave
    theta = jitter(mm, pb, B)
    hip = mm.HipObjective(pb)
    assert hip.kernel_info(B)["likelihood_form"] == LL_SEPARATE_PASS
    assert "solver=2" in hip.kernel_info(B)["kernel_name"]
    got = hip.eval_batch(theta, want_traj=True)
    assert np.all(got["status"] == 0)
    _check_strict(oracle_py, pb, got, theta, [0, 1, B - 1])
    again = hip.eval_batch(theta)  # the likelihood-only launch: the same numbers
    assert np.array_equal(again["loglik"], got["loglik"])


@pytest.mark.parametrize("n_age", [1, 2, 8, 16])
def test_strict_other_lane_counts(mm, oracle_py, shipped, n_age):
    pb = mm.restrict_age_classes(shipped, list(range(n_age))) if n_age <= 2 else mm.widen_age_classes(shipped, n_age // 4)
    pb = short(pb).with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_STRICT)
    theta = jitter(mm, pb, 19)
    hip = mm.HipObjective(pb)
    assert f"lpc={n_age} solver=2" in hip.kernel_info(19)["kernel_name"]
    got = hip.eval_batch(theta, want_traj=True)
    _check_strict(oracle_py, pb, got, theta, [0, 18])


def test_strict_chip_filling_batch_runs_the_inline_likelihood(mm, oracle_py, synth400):
    """More than 1024 waves: the inline-likelihood kernel; the same chains in chunks through the separate pass give the
    same bits, and a sample of them matches the restatement."""
    pb = synth400.with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_STRICT)
    B = 16 * 1024 + 37
    hip = mm.HipObjective(pb)
    assert hip.kernel_info(B)["likelihood_form"] == LL_INLINE
    assert hip.kernel_info(4096)["likelihood_form"] == LL_SEPARATE_PASS
    theta = np.tile(jitter(mm, pb, 512), (B // 512 + 1, 1))[:B]
    big = hip.eval_batch(theta)
    assert np.all(big["status"] == 0)
    for off in range(0, B, 4096):
        part = hip.eval_batch(theta[off:off + 4096])
        for k in ("loglik", "status", "n_accept", "n_reject"):
            assert np.array_equal(part[k], big[k][off:off + 4096]), (k, off)
    _check_strict(oracle_py, pb, big, theta, [5, B - 1])


@pytest.mark.parametrize("n_age", [4, 16])
def test_strict_lane_counts_inline_likelihood(mm, oracle_py, shipped, n_age):
    pb = shipped if n_age == 4 else mm.widen_age_classes(shipped, 4)
    pb = short(pb, 80).with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_STRICT)
    cpw = 64 // n_age
    B = cpw * 1100 + 3
    hip = mm.HipObjective(pb)
    assert hip.kernel_info(B)["likelihood_form"] == LL_INLINE
    theta = np.tile(jitter(mm, pb, 256), (B // 256 + 1, 1))[:B]
    big = hip.eval_batch(theta)
    _check_strict(oracle_py, pb, big, theta, [0, B - 1])


# ---------------------------------------------------------------- 3. fma
def test_fma_within_tolerance_and_independent_of_the_batch(mm, oracle_py, synth400):
    pb = synth400.with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_FMA)
    theta = jitter(mm, pb, 64)
    hip = mm.HipObjective(pb)
    small = hip.eval_batch(theta, want_traj=True)
    assert np.all(small["status"] == 0)
    same = 0
    idx = [0, 1, 2, 3, 63]
    for b in idx:
        want = restate(oracle_py, pb, theta[b], FEHLBERG78)
        assert rel_err(small["traj"][b], want["traj"]) < 1e-6, b
        same += (small["n_accept"][b], small["n_reject"][b]) == (want["n_accept"], want["n_reject"])
    assert same >= 0.9 * len(idx)
    B = 16 * 1024 + 64
    assert hip.kernel_info(B)["likelihood_form"] == LL_INLINE and hip.kernel_info(64)["likelihood_form"] == LL_SEPARATE_PASS
    # one wave per SIMD only: the whole register file, nothing spilled to scratch (a two-wave form would spill ~210 registers)
    assert hip.kernel_info(B)["vgprs"] > 256 and hip.kernel_info(B)["scratch_bytes"] == 0
    big = hip.eval_batch(np.tile(theta, (B // 64, 1)))
    for k in ("loglik", "status", "n_accept", "n_reject"):
        assert np.array_equal(big[k][-64:], small[k]), k
        assert np.array_equal(big[k][:64], small[k]), k


# ---------------------------------------------------------------- 4. independent accuracy
# Boost's Fehlberg 7(8) cannot see a jump of beta(t) kappa(t) at the left end of a step: its error estimate
# 41/840 h (k1 + k11 - k12 - k13) pairs stages at c = 0 (k1, k12) and at c = 1 (k11, k13), and in the step that starts on a
# schedule breakpoint both c = 0 stages take the old segment's value and the other eleven the new one.  The estimate
# cancels, the step is accepted, and the solution carries an O(h delta(beta kappa)) error: on the shipped problem the
# states leave the high-precision answer by 4e-3 in the step [13, 14] (1e-8 before it), and tightening the tolerance to 1e-10
# still leaves 2e-4.  That is the method under integrate_times, restated bit for bit by the driver above (section 2), not
# the kernel; the golden bars of the other solvers therefore hold only up to the first breakpoint.
@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_golden_highprec(mm, golden, shipped, arith):
    g = golden["shipped"]
    pb = shipped.with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_STRICT if arith == "strict" else mm.ARITH_FMA)
    got = mm.HipObjective(pb).eval_batch(np.array(g["theta"])[None, :], want_traj=True)
    assert got["status"][0] == 0
    idx = np.array(g["time_index"])
    gs = np.array(g["states"])
    err = (np.abs(got["traj"][0][idx] - gs) / (np.abs(gs) + 1.0)).max(axis=1)
    first_break = float(np.min(pb.kappa_end_times))
    before = np.asarray(pb.times)[idx] <= first_break
    assert before.sum() >= 4
    assert err[before].max() < 1e-3  # test_golden_highprec's bar, up to and including the first breakpoint (measured 1e-8)
    assert err[before].max() < 1e-6
    # past it: the breakpoint step's error, bounded (measured 4e-3 on the states, 2.8e-4 on the log-likelihood)
    assert err.max() < 1e-2
    assert abs(got["loglik"][0] - g["loglik"]) / abs(g["loglik"]) < 1e-3


# ---------------------------------------------------------------- 5. refusals
def test_quad_form_and_fp32_are_refused_and_the_context_stays_usable(mm, shipped):
    pb = shipped.with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_FMA)
    theta = jitter(mm, pb, 24)
    hip = mm.HipObjective(pb)
    assert hip.kernel_info(24)["lanes_per_chain"] == 4  # AUTO never picks the sixteen-lane form for Fehlberg
    before = hip.eval_batch(theta)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        hip.set_integrator_form(FORM_QUAD)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        hip.set_precision(PRECISION_F32)
    after = hip.eval_batch(theta)
    for k in ("loglik", "status", "n_accept", "n_reject"):
        assert np.array_equal(before[k], after[k]), k
    with pytest.raises(RuntimeError, match="fp32"):
        mm.HipObjective(pb.with_(precision=PRECISION_F32))


@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_step_budget_gives_status_3(mm, ref_fixture, arith):
    pb = ref_fixture.with_(solver=mm.SOLVER_FEHLBERG78, abs_err=0.0, rel_err=1e-300, max_attempts=3000,
                           arith=mm.ARITH_STRICT if arith == "strict" else mm.ARITH_FMA)
    got = mm.HipObjective(pb).eval_batch(np.tile(pb.base_theta, (3, 1)))
    assert got["status"].tolist() == [3, 3, 3]
    assert np.all(got["loglik"] == mm.LOWEST)
    assert np.all(got["n_accept"] + got["n_reject"] == 3000)


# ---------------------------------------------------------------- 6. the adapter and a caller
def test_host_adapter_and_device_resident_sampler(mm, shipped):
    pb = shipped.with_(solver=mm.SOLVER_FEHLBERG78, arith=mm.ARITH_FMA, constraint_mode=1)
    theta = jitter(mm, pb, 8)
    hip = mm.HipObjective(pb)
    hip.set_constraint_mode(1)
    want = hip.eval_batch(theta)
    host = mm.HostObjective(pb)
    out, status = host.calculate_batch(theta)
    assert np.array_equal(status, want["status"]) and np.array_equal(out, want["loglik"])
    assert host.calculate(theta[1]) == want["loglik"][1]

    x0 = jitter(mm, pb, 6, seed=9)
    run = mm.HostObjective(pb).metropolis_hastings(x0, seed=21, iterations=80, burn_in=20, adaptation_period=20, thinning=5,
                                                   device_state=True)
    assert run["accepted"].sum() > 0
    vals = run["sample_values"].ravel()
    assert np.all(np.isfinite(vals)) and np.all(vals > -1e17)  # no failed evaluation among the stored samples
    again = hip.eval_batch(run["samples"].reshape(-1, pb.n_params))
    assert np.array_equal(again["loglik"], vals)
