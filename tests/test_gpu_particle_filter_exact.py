"""The particle filter and the stochastic ensemble ON THE DEVICE against exact likelihoods of tiny epidemics: the cases, the
exact forward recursion and the three families of assertions of test_particle_filter_exact_cpu.py, with the device's own model
values fed to the recursion, plus equality with the host twin bit for bit.  Populations of 1 or 2 per class (every binomial
draw has n <= 2) and age classes without people (N = 0) run on the device only here."""
import functools

import numpy as np
import pytest

from test_gpu_stochastic_sepaihrd import INIT_FIXED, objective, problem as cut_fixture
from test_particle_filter_exact_cpu import (BETA_ENDS, CASES, ESTIMATES, KAPPA_ENDS, KAPPA_VALUES, NAN, NUM_POP, RUNUP, T_ROWS, check_against_pmf,
                                            check_final_moments, check_prefix_likelihoods)

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF0  # both words of the key in use
KEYS = ("loglik", "increments", "ess", "final_state")


def tiny_problem(mm, ref_fixture, case, obs=None):
    """the reference fixture cut to the case's grid and age classes, with the case's N, M, initial counts, rates, schedules and
    observations in place of its own; the parameter vector carries theta, the three kappa values and multipliers that
    INIT_FIXED does not read"""
    ob = case.obs if obs is None else obs
    pb = cut_fixture(mm, ref_fixture, case.n, T_ROWS - RUNUP)
    base = pb.base_theta.copy()
    base[:5] = [case.scalars["beta"], case.scalars["theta"], *KAPPA_VALUES[1:]]
    assert list(pb.param_names[:5]) == ["beta", "theta", "kappa_1", "kappa_2", "kappa_3"]
    return pb.with_(N=case.N, M=case.M, initial_state=case.x0.ravel(), times=case.times, beta_end_times=np.array(BETA_ENDS),
                    beta_values=np.array(case.beta_values), kappa_end_times=np.array(KAPPA_ENDS), kappa_values=np.array(KAPPA_VALUES),
                    obs_H=ob[0], obs_ICU=ob[1], obs_D=ob[2], base_theta=base, **case.scalars, **case.vectors)


@functools.lru_cache(maxsize=None)
def device_estimates(mm, name, pb_key):
    """E = B K filter runs of a case on the device, K calls of B equal parameter vectors: increments [E][T_pos], loglik [E], the
    particle mean of the final counts [E][9][n], their maximum [9][n], the first call as it came back, the kernel's ms per call"""
    case, pb = CASES[name], pb_key.pb
    B, K = ESTIMATES[name]
    hip = objective(mm, pb, INIT_FIXED)
    theta = np.stack([pb.base_theta] * B)
    inc, ll, mean, top, first, ms = [], [], [], np.zeros((NUM_POP, case.n)), None, []
    for k in range(K):
        got = hip.particle_loglik(theta, case.J, case.m, SEED + k, want_values=True, want_final=True)
        ms.append(hip.particle_timing()[1])
        assert not got["status"].any() and got["n_valid"] == B
        first = got if first is None else first
        inc.append(got["increments"])
        ll.append(got["loglik"])
        mean.append(got["final_state"][:, :, :NUM_POP].mean(axis=1))
        top = np.maximum(top, got["final_state"][:, :, :NUM_POP].max(axis=(0, 1)))
    return np.concatenate(inc), np.concatenate(ll), np.concatenate(mean), top, first, np.array(ms)


class Keyed:
    """a problem under the name of its case, so that the runs above are made once per case"""

    def __init__(self, name, pb):
        self.name, self.pb = name, pb

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name


def run_of(mm, ref_fixture, name):
    pb = tiny_problem(mm, ref_fixture, CASES[name])
    return pb, device_estimates(mm, name, Keyed(name, pb))


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_twin_on_a_tiny_epidemic(mm, ref_fixture, name):
    """the first of the K calls (B = 1024 positions, every output) against the twin; the model values are the case's own row"""
    case = CASES[name]
    pb, (_, _, _, _, got, ms) = run_of(mm, ref_fixture, name)
    mv = got["model_values"]
    assert (mv == mv[0]).all()
    x0 = mv[0, -11 * case.n:].reshape(11, case.n)
    assert np.array_equal(x0, case.x0) and x0[:NUM_POP].sum() <= 6 and (pb.N[[a for a in range(case.n) if a not in case.occupied]] == 0).all()
    print(f"{name}: model values equal the hand-packed row: {np.array_equal(mv[0], case.row(mm))}")
    twin = mm.hostabi.particle_from_values(mv, got["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H, pb.obs_ICU, pb.obs_D, case.J,
                                           case.m, SEED, beta_end_times=pb.beta_end_times)
    for key in KEYS:
        assert np.array_equal(got[key], twin[key], equal_nan=True), key
    assert np.isnan(got["ess"][:, case.blank_row]).all() and np.isfinite(np.delete(got["ess"], case.blank_row, axis=1)).all()
    assert len(set(got["loglik"])) > got["loglik"].size // 2  # every position has a stream of its own
    print(f"{name}: B {mv.shape[0]} J {case.J} m {case.m}: filter kernel {ms.min():.3f} .. {ms.max():.3f} ms per call")


@pytest.mark.parametrize("name", list(CASES))
def test_prefix_likelihoods_are_unbiased_for_the_exact_ones(mm, ref_fixture, name):
    case = CASES[name]
    _, (inc, _, _, _, got, _) = run_of(mm, ref_fixture, name)
    exact = case.exact(got["model_values"][0])
    check_prefix_likelihoods(name, inc, exact.Z)


@pytest.mark.parametrize("name", list(CASES))
def test_final_state_moments_are_unbiased_for_the_exact_ones(mm, ref_fixture, name):
    case = CASES[name]
    _, (_, ll, mean, top, got, _) = run_of(mm, ref_fixture, name)
    exact = case.exact(got["model_values"][0])
    check_final_moments(name, ll, mean, top, exact.G)


@pytest.mark.parametrize("name", list(CASES))
def test_unweighted_run_has_the_exact_final_distribution(mm, ref_fixture, name):
    """no usable observation: the filter's particles and the replicates of sepaihrd_ensemble_stochastic (every case, n = 16 with
    its thirteen empty classes among them) follow the exact marginal pmf of every compartment at the final row"""
    case = CASES[name]
    blank = np.full_like(case.obs, NAN)
    pb = tiny_problem(mm, ref_fixture, case, blank)
    hip = objective(mm, pb, INIT_FIXED)
    B = 256
    theta = np.stack([pb.base_theta] * B)
    got = hip.particle_loglik(theta, case.J, case.m, SEED + 100, want_values=True, want_final=True)
    ms = hip.particle_timing()[1]
    assert not got["status"].any() and not got["loglik"].any()
    exact = case.exact(got["model_values"][0], blank)
    check_against_pmf(name, "filter", got["final_state"].reshape(B * case.J, 11, case.n), exact.pmf, case.occupied)
    ens = hip.ensemble_stochastic(theta, case.J, case.m, SEED + 101, [0.5], want_values=True, want_final=True)
    assert np.array_equal(ens["model_values"], got["model_values"]) and ens["n_valid"] == B
    check_against_pmf(name, "ensemble", ens["final_state"].reshape(B * case.J, 11, case.n), exact.pmf, case.occupied)
    twin = mm.hostabi.stochastic_from_values(ens["model_values"], ens["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, case.J, case.m, SEED + 101,
                                             [0.5], beta_end_times=pb.beta_end_times)
    assert np.array_equal(ens["final_state"], twin["final_state"]) and np.array_equal(ens["quantiles"], twin["quantiles"], equal_nan=True)
    print(f"{name}: blank run, filter kernel {ms:.3f} ms, ensemble step kernel {ens['phase_ms'][0]:.3f} ms")
