"""ctypes view of the C++ host mirror (host/, libsepaihrd_host.so) -- test plumbing.

The C++ classes (HipSEPAIHRDObjectiveFunction, HipSEPAIHRDParameterManager, SimulationCache,
MultiChainMetropolisHastings) are what a reference maintainer links against; the flat functions
of host/src/host_capi.cpp only exist so that the Python test-suite can drive them.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import hipabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsepaihrd_host.so")
_lib = None


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    hipabi.load_library()  # torch-first HIP runtime + libsepaihrd_hip.so, then the host library
    path = os.environ.get("SEPAIHRD_HOST_LIB") or LIB_PATH  # env override: experiment builds only
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found: run __graft_entry__.build()")
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.host_last_error.restype = C.c_char_p
    lib.host_last_mh_loop_seconds.restype = C.c_double
    lib.host_last_mh_diagnostics_seconds.restype = C.c_double
    lib.host_objective_create.restype = vp
    lib.host_objective_create.argtypes = [C.POINTER(hipabi.sepaihrd_problem), C.c_char_p, C.c_char_p, vp, C.c_int,
                                          C.c_int, C.c_int]
    lib.host_objective_destroy.restype = None
    lib.host_objective_destroy.argtypes = [vp]
    lib.host_model_holders.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int),
                                       C.c_char_p, C.c_int]
    lib.host_reference_constructors.argtypes = [C.POINTER(hipabi.sepaihrd_problem), C.c_char_p, C.c_char_p, vp, vp, C.c_int, vp, vp]
    lib.host_objective_calculate.argtypes = [vp, vp, C.POINTER(C.c_double)]
    lib.host_objective_calculate_batch.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.host_cache_stats.restype = None
    lib.host_cache_stats.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.host_apply_constraints.argtypes = [vp, C.c_int, vp, vp]
    lib.host_current_parameters.argtypes = [vp, vp]
    lib.host_mh_run.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                C.c_double, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int]
    lib.host_mh_run_groups.argtypes = [vp, C.c_int, C.c_int, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.host_mh_groups_summaries.argtypes = [vp, C.c_int, C.c_int, vp, C.c_uint32] + [C.c_int] * 5 + [vp] * 6
    lib.host_mh_run_reported.argtypes = [vp, C.c_int, vp, C.c_uint32] + [C.c_int] * 8 + \
        [C.c_char_p, C.c_char_p, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_long)]
    lib.host_mh_run_analytic.argtypes = [C.c_int, vp, vp, C.c_double, C.c_int, vp, C.c_uint32] + [C.c_int] * 4 + [vp] * 9
    lib.host_summary_quantiles.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.host_libm_selfcheck.restype = None
    lib.host_libm_selfcheck.argtypes = [C.POINTER(C.c_int)] * 3
    lib.host_libm_selfcheck_args.restype = None
    lib.host_libm_selfcheck_args.argtypes = [vp, vp]
    lib.host_default_arith.restype = C.c_int
    lib.host_default_arith.argtypes = []
    for f in (lib.host_glibc_log, lib.host_glibc_exp):
        f.restype = None
        f.argtypes = [vp, C.c_int, vp]
    lib.host_gradient.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_double, vp, vp]
    lib.host_calibrate.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.host_hc_run.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.host_calibrate_pso.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                       vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.host_nuts_run.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                  C.c_double, C.c_int, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.host_nuts_chains_run.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                         C.c_double, C.c_int, C.c_int, vp, C.c_uint32, C.c_int] + [vp] * 12
    lib.host_nuts_chains_analytic.argtypes = [C.c_int, vp, vp, C.c_double, vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double,
                                              C.c_int, C.c_int, vp, C.c_uint32] + [vp] * 12
    lib.host_pso_run.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.host_ensemble.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_int, C.c_int, C.c_uint32,
                                  vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.host_scenario_comparison.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                             C.c_char_p, vp, vp, vp]
    lib.host_ene_covid_validation.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                              C.c_char_p]
    lib.host_set_mh_diagnostics.argtypes = [vp, C.c_int]
    lib.host_set_mh_diagnostics.restype = None
    lib.host_mh_diagnostics.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    lib.host_chain_diagnostics.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.host_sir_rhs.argtypes = [C.c_int, vp, vp, vp, C.c_double, C.c_double, vp, vp]
    lib.host_sir_create.restype = vp
    lib.host_sir_create.argtypes = [C.POINTER(hipabi.sepaihrd_sir_problem), C.c_char_p, C.c_char_p, vp, C.c_int, C.c_int, C.c_int]
    lib.host_sir_destroy.restype = None
    lib.host_sir_destroy.argtypes = [vp]
    lib.host_sir_manager_info.argtypes = [vp, vp, vp, vp, vp]
    lib.host_sir_index_for_param.argtypes = [vp, C.c_char_p]
    lib.host_sir_apply_constraints.argtypes = [vp, vp, vp]
    lib.host_sir_update_model.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
    lib.host_sir_calculate.argtypes = [vp, vp, C.POINTER(C.c_double)]
    lib.host_sir_calculate_batch.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.host_sir_cache_stats.restype = None
    lib.host_sir_cache_stats.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.host_sir_hc_run.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_double)]
    lib.host_sir_mh_run.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp]
    lib.host_sir_mh_run_ex.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double] + \
        [C.c_int] * 9 + [C.c_char_p, C.c_char_p] + [vp] * 4 + [vp, C.POINTER(C.c_int32), vp, vp, vp, C.POINTER(C.c_int),
                                                             C.POINTER(C.c_long), vp, C.POINTER(C.c_int32)]
    lib.host_sir_scenario_events.argtypes = [vp, C.c_int, C.c_int, vp, C.c_char_p, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    lib.host_sir_write_scenario_csvs.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    lib.host_sir_scenario_comparison.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, vp, vp, C.c_char_p, vp, vp, C.c_int,
                                                 C.c_char_p, C.c_char_p, vp, vp, vp, vp, vp, vp]
    lib.host_sir_calibrate.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                       C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
    lib.host_stoch_philox.restype = None
    lib.host_stoch_philox.argtypes = [vp, vp, vp]
    lib.host_stoch_uniform.restype = C.c_double
    lib.host_stoch_uniform.argtypes = [C.c_uint32, C.c_uint32]
    lib.host_stoch_probabilities.restype = None
    lib.host_stoch_probabilities.argtypes = [C.c_double] * 5 + [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.host_stoch_binomial_at.restype = C.c_int32
    lib.host_stoch_binomial_at.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_double]
    lib.host_stoch_binomial_probe.restype = None
    lib.host_stoch_binomial_probe.argtypes = [C.c_uint64, vp, vp, C.c_int, vp]
    lib.host_stoch_sir_run.argtypes = [C.POINTER(hipabi.sepaihrd_stoch_sir_config), vp, vp, vp, vp, C.c_char_p, C.c_int]
    lib.host_stoch_sir_model.argtypes = [C.c_double] * 9 + [C.c_uint, C.c_uint64, C.c_int, C.c_char_p, vp, vp, C.POINTER(C.c_int),
                                                            C.c_char_p, C.c_int]
    lib.host_poisson_probe.restype = None
    lib.host_poisson_probe.argtypes = [C.c_uint64, vp, C.c_int, vp]
    lib.host_poisson_at.restype = C.c_double
    lib.host_poisson_at.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
    lib.host_predictive_from_means.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int, vp, vp, vp,
                                               C.c_char_p, C.c_int]
    lib.host_predictive.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint64,
                                    vp, C.c_int] + [vp] * 9
    lib.host_predictive_dispersed.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                              C.c_uint64, vp, C.c_int] + [vp] * 11
    lib.host_predictive_nb_from_means.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int, vp, vp, vp,
                                                  C.c_char_p, C.c_int]
    lib.host_predictive_scores_from_means.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int, vp, C.c_int,
                                                      vp, vp, vp, vp, vp, vp, C.c_char_p, C.c_int]
    lib.host_predictive_targets_from_means.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int, C.c_int, vp,
                                                       C.c_int, vp, C.c_int] + [vp] * 8 + [C.c_char_p, C.c_int]
    lib.host_predictive_targets.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                            C.c_uint64, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int] + [vp] * 13
    lib.host_score_cell.argtypes = [vp, C.c_int, C.c_double, vp, C.c_int, vp, vp, vp, C.c_char_p, C.c_int]
    lib.host_predictive_scores.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                           C.c_uint64, vp, C.c_int, vp, C.c_int] + [vp] * 13
    lib.host_gamma_at.restype = C.c_double
    lib.host_gamma_at.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
    lib.host_nb_draw_at.restype = C.c_double
    lib.host_nb_draw_at.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double]
    lib.host_gamma_probe.restype = None
    lib.host_gamma_probe.argtypes = [C.c_uint64, vp, C.c_int, vp]
    lib.host_nb_draw_probe.restype = None
    lib.host_nb_draw_probe.argtypes = [C.c_uint64, vp, vp, C.c_int, vp]
    lib.host_stochastic_from_values.argtypes = [C.c_int] * 4 + [vp] * 7 + [C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int, C.c_int] + \
        [vp] * 4 + [C.c_char_p, C.c_int]
    lib.host_stochastic_manager_values.argtypes = [vp, C.c_int, vp, vp]
    lib.host_stochastic.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                    C.c_uint64, vp, C.c_int] + [vp] * 6
    lib.host_particle_from_values.argtypes = [C.c_int] * 4 + [vp] * 5 + [C.c_int] + [vp] * 5 + [C.c_int, C.c_int, C.c_int, C.c_uint64] + \
        [vp] * 4 + [C.c_char_p, C.c_int]
    lib.host_particle_wide_from_values.argtypes = lib.host_particle_from_values.argtypes
    lib.host_particle_nb_from_values.argtypes = [C.c_int] * 4 + [vp] * 5 + [C.c_int] + [vp] * 5 + [C.c_int, C.c_int, C.c_int, C.c_uint64, vp] + \
        [vp] * 4 + [C.c_char_p, C.c_int]
    lib.host_particle_wide_nb_from_values.argtypes = lib.host_particle_nb_from_values.argtypes
    lib.host_particle_states_from_values.argtypes = [C.c_int] * 4 + [vp] * 5 + [C.c_int] + [vp] * 5 + [C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp,
                                                     C.c_int] + [vp] * 5 + [C.c_char_p, C.c_int]
    lib.host_particle_filter_states.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp,
                                                C.c_int, C.c_int, vp, C.c_int] + [vp] * 5
    lib.host_particle_nb_term.restype = None
    lib.host_particle_nb_term.argtypes = [vp, vp, C.c_int, C.c_double, vp]
    lib.host_particle_nb_row_constants.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_char_p, C.c_int]
    lib.host_particle_likelihood_nb.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp,
                                                C.c_int, C.c_int, vp, vp]
    lib.host_particle_resample.restype = None
    lib.host_particle_resample.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.host_particle_likelihood.argtypes = [vp, C.POINTER(hipabi.sepaihrd_problem), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int,
                                             C.c_int, vp, vp]
    lib.host_lgamma_pos.restype = C.c_double
    lib.host_lgamma_pos.argtypes = [C.c_double]
    lib.host_nb_objective.argtypes = [vp] * 5 + [C.c_int] * 3 + [vp] * 3
    lib.host_objective_set_dispersion.argtypes = [vp, vp]
    _lib = lib
    return lib


def _check(rc, prefix: str = "") -> None:
    """RuntimeError with the library's last message (host_last_error) behind ``prefix`` for a non-zero return code"""
    if rc:
        raise RuntimeError(prefix + load_library().host_last_error().decode())


_MH_ARRAYS = ("accepted", "best_value", "best", "final_scale", "accept_trace", "samples", "sample_values", "final_cov")


def _mh_arrays(Cn: int, P: int, iterations: int, thinning: int = 1, want_trace: bool = True, keys=_MH_ARRAYS) -> dict:
    """The named result arrays of a Metropolis-Hastings run, leading axis = chain (accept_trace None unless wanted).  The C
    side stores t = 0 and every thinning-th iteration after it: n_s samples per chain."""
    n_s = 1 + (max(iterations, 1) - 1) // max(1, thinning)
    spec = {"accepted": ((Cn,), np.int32), "best_value": ((Cn,), np.float64), "best": ((Cn, P), np.float64),
            "final_scale": ((Cn,), np.float64), "accept_trace": ((Cn, max(iterations - 1, 1)), np.uint8),
            "samples": ((Cn, n_s, P), np.float64), "sample_values": ((Cn, n_s), np.float64), "final_cov": ((Cn, P, P), np.float64)}
    return {k: np.zeros(*spec[k]) if k != "accept_trace" or want_trace else None for k in keys}


def _ptr(a):
    return None if a is None else a.ctypes.data


def _mh_result(a: dict, iterations: int, n_samples=None, **more) -> dict:
    """The result dictionary of a Metropolis-Hastings wrapper from its _mh_arrays: the accept trace cut to its
    iterations - 1 columns, the sample count the C side reported checked against the arrays, ``more`` behind them."""
    if n_samples is not None:
        assert n_samples == a["samples"].shape[1]
    out = dict(a)
    if out.get("accept_trace") is not None:
        out["accept_trace"] = out["accept_trace"][:, :iterations - 1]
    out.update(more)
    return out


def mh_analytic(mean, precision, initial, seed: int, iterations: int, burn_in: int, adaptation_period: int = 100, thinning: int = 1,
                sigma: float = 1.0, want_trace: bool = True) -> dict:
    """Test hook without a GPU (host_mh_run_analytic): MultiChainMetropolisHastings' scalar path, chain c through optimize()
    with seed + c, over the log-density of a Gaussian with the given mean and precision matrix -- through the settings
    builder and the output record of every MH entry point.  The arrays of HostObjective.metropolis_hastings."""
    lib = load_library()
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    prec = np.ascontiguousarray(precision, dtype=np.float64)
    x0 = np.ascontiguousarray(np.atleast_2d(initial), dtype=np.float64)
    Cn, D = x0.shape
    if mean.shape != (D,) or prec.shape != (D, D):
        raise ValueError("mean [D], precision [D][D], initial [C][D]")
    a = _mh_arrays(Cn, D, iterations, thinning, want_trace)
    ns = C.c_int32()
    ptrs = [_ptr(a[k]) for k in _MH_ARRAYS]
    _check(lib.host_mh_run_analytic(D, mean.ctypes.data, prec.ctypes.data, sigma, Cn, x0.ctypes.data, seed, iterations, burn_in,
                                    adaptation_period, thinning, *ptrs[:5], C.byref(ns), *ptrs[5:]), "host_mh_run_analytic: ")
    return _mh_result(a, iterations, ns.value)


def _calibration(entry, head, prefix: str, P: int, chains: int, mh_iterations: int, thinning: int) -> dict:
    """One of the two-phase calibration entry points: its own arguments ``head``, then the ten outputs they share.  Per-chain
    arrays are chain-major with cap samples per chain: t = 0 and every thinning-th iteration after it."""
    cap = 1 + (mh_iterations - 1) // max(1, thinning)
    out = {"best": np.empty(P), "phase2_cov": np.empty((P, P)), "accept_trace": np.empty((chains, mh_iterations - 1), dtype=np.uint8),
           "samples": np.empty((chains, cap, P)), "sample_values": np.empty((chains, cap)), "mcmc_objective_values": np.empty((chains, cap))}
    bv, iv, p1, ns = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    _check(entry(*head, out["best"].ctypes.data, C.byref(bv), C.byref(iv), C.byref(p1),
                 *[out[k].ctypes.data for k in ("phase2_cov", "accept_trace", "samples", "sample_values", "mcmc_objective_values")], C.byref(ns)),
           prefix)
    assert ns.value == cap, (ns.value, cap)
    out.update(best_value=bv.value, initial_value=iv.value, phase1_best_value=p1.value, n_samples=ns.value)
    return out


def _nuts_chains_outputs(Cn: int, iterations: int, P: int):
    """Arrays of a lock-step NUTS run, leading axis = chain, and their pointers in the order of the C entry points."""
    out = {"samples": np.empty((Cn, iterations, P)), "sample_values": np.empty((Cn, iterations)),
           "epsilon_trace": np.empty((Cn, iterations)), "depth_trace": np.empty((Cn, iterations), dtype=np.int32),
           "n_samples": np.empty(Cn, dtype=np.int32), "best": np.empty((Cn, P)), "best_value": np.empty(Cn),
           "gradient_calls": np.empty(Cn, dtype=np.int64), "rows_evaluated": np.empty(Cn, dtype=np.int64),
           "failure_status": np.empty(Cn, dtype=np.int32), "failure_iteration": np.empty(Cn, dtype=np.int32)}
    stats = np.zeros(6)
    return out, stats, [a.ctypes.data for a in out.values()] + [stats.ctypes.data]


def nuts_chains_analytic(mean, precision, theta0, seed0: int, iterations: int, adaptation_window: int, max_tree_depth: int = 10,
                         delta_target: float = 0.8, sigma: float = 1.0, lock_step: bool = True, fail_centre=None,
                         fail_radius: float = 0.0) -> dict:
    """Test hook without a GPU (host_nuts_chains_analytic): the lock-step sampler, or chain by chain HipNUTSSampler
    (lock_step=False), over the log-density of a Gaussian with the given mean and precision matrix and its exact gradient;
    inside the ball (fail_centre, fail_radius) the objective reports an integration failure.  Result as
    HostObjective.nuts_chains."""
    lib = load_library()
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    prec = np.ascontiguousarray(precision, dtype=np.float64)
    th = np.ascontiguousarray(np.atleast_2d(theta0), dtype=np.float64)
    D = mean.shape[0]
    if prec.shape != (D, D) or th.shape[1] != D:
        raise ValueError("mean [D], precision [D][D], theta0 [C][D]")
    fc = None if fail_centre is None else np.ascontiguousarray(fail_centre, dtype=np.float64)
    out, stats, ptrs = _nuts_chains_outputs(th.shape[0], iterations, D)
    _check(lib.host_nuts_chains_analytic(D, mean.ctypes.data, prec.ctypes.data, sigma, None if fc is None else fc.ctypes.data,
                                         fail_radius, int(lock_step), iterations, adaptation_window, delta_target, max_tree_depth,
                                         th.shape[0], th.ctypes.data, seed0, *ptrs), "host_nuts_chains_analytic: ")
    out.update(ticks=int(stats[0]), rows_total=int(stats[1]),
               mean_rows_per_tick=stats[1] / stats[0] if stats[0] > 0 else 0.0)
    return out


class HostObjective:
    """HipSEPAIHRDObjectiveFunction + its parameter manager + a SimulationCache (C++ objects)."""

    def __init__(self, pb, device: int = -1, cache_capacity: int = 1000, with_objective: bool = True):
        self.lib = load_library()
        self.pb = pb
        keep: list = []
        st = hipabi.build_problem_struct(pb, keep)
        sig = np.ascontiguousarray(pb.sigma_array())
        self.h = self.lib.host_objective_create(C.byref(st), "\n".join(pb.param_names).encode(),
                                                "\n".join(pb.npi_names).encode(), sig.ctypes.data, device,
                                                cache_capacity, int(with_objective))
        _check(not self.h, "host_objective_create failed: ")
        self.P = pb.n_params
        if with_objective and getattr(pb, "dispersion", None) is not None:
            self.set_dispersion(pb.dispersion)

    def set_dispersion(self, k) -> None:
        """HipSEPAIHRDObjectiveFunction::setDispersion: the fixed negative-binomial dispersions of the H, ICU, D series (+inf:
        Poisson) for everything that evaluates through this object's objective"""
        kk = np.ascontiguousarray(k, dtype=np.float64)
        if kk.shape != (3,):
            raise ValueError("dispersion must have three entries: k_H, k_ICU, k_D")
        _check(self.lib.host_objective_set_dispersion(self.h, kk.ctypes.data), "setDispersion: ")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.host_objective_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def hill_climbing(self, x0, seed: int, iterations: int, cloud_size_multiplier: int = 8, threads: int = 16,
                      use_scalar_interface: bool = False) -> dict:
        """BatchedHillClimbingOptimizer::optimize in OPTIMIZATION_CLAMP mode (calibration phase 1)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        best = np.empty(self.P)
        cov = np.empty((self.P, self.P))
        trace = np.empty(iterations)
        bv = C.c_double(0.0)
        ne, nl = C.c_long(0), C.c_long(0)
        _check(self.lib.host_hc_run(self.h, x0.ctypes.data, seed, threads, iterations, cloud_size_multiplier,
                                    int(use_scalar_interface), best.ctypes.data, C.byref(bv), cov.ctypes.data,
                                    trace.ctypes.data, C.byref(ne), C.byref(nl)), "host_hc_run: ")
        return {"best": best, "best_value": bv.value, "final_cov": cov, "trace": trace,
                "evaluations": ne.value, "launches": nl.value}

    def particle_swarm(self, x0, seed: int, **settings) -> dict:
        """BatchedParticleSwarmOptimization::optimize in OPTIMIZATION_CLAMP mode; settings as in pso_settings.txt."""
        settings = dict(settings, seed=seed)
        keys = (C.c_char_p * len(settings))(*[k.encode() for k in settings])
        vals = np.array([float(v) for v in settings.values()])
        x0p = None
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            x0p = x0.ctypes.data
        iters = int(settings.get("iterations", 100))
        best = np.empty(self.P)
        cov = np.empty((self.P, self.P))
        trace = np.empty(iters)
        bv = C.c_double(0.0)
        ne, nl = C.c_long(0), C.c_long(0)
        _check(self.lib.host_pso_run(self.h, x0p, keys, vals.ctypes.data, len(settings), best.ctypes.data, C.byref(bv),
                                     cov.ctypes.data, trace.ctypes.data, C.byref(ne), C.byref(nl)), "host_pso_run: ")
        return {"best": best, "best_value": bv.value, "final_cov": cov, "trace": trace,
                "evaluations": ne.value, "launches": nl.value}

    def evaluate_with_gradient(self, theta, epsilon: float = 1e-4, device: int = -1):
        """HipSEPAIHRDGradientObjectiveFunction::evaluate_with_gradient: (value, gradient)."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        g = np.empty(self.P)
        v = C.c_double(0.0)
        _check(self.lib.host_gradient(self.h, C.byref(st), device, th.ctypes.data, epsilon, C.byref(v), g.ctypes.data), "host_gradient: ")
        return v.value, g

    def nuts(self, theta0, seed: int, iterations: int, adaptation_window: int, max_tree_depth: int = 10,
             delta_target: float = 0.8, fd_epsilon: float = 1e-4, constraint_mode: int = 1, device: int = -1) -> dict:
        """HipNUTSSampler::optimize over a HipSEPAIHRDGradientObjectiveFunction (SEPAIHRDModelCalibration::runNUTS)."""
        th = np.ascontiguousarray(theta0, dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        samples = np.empty((iterations, self.P))
        values, eps = np.empty(iterations), np.empty(iterations)
        depth = np.empty(iterations, dtype=np.int32)
        best = np.empty(self.P)
        bv = C.c_double(0.0)
        nc, nl = C.c_long(0), C.c_long(0)
        ns = self.lib.host_nuts_run(self.h, C.byref(st), device, iterations, adaptation_window, delta_target,
                                    max_tree_depth, fd_epsilon, constraint_mode, th.ctypes.data, seed,
                                    samples.ctypes.data, values.ctypes.data, eps.ctypes.data, depth.ctypes.data,
                                    best.ctypes.data, C.byref(bv), C.byref(nc), C.byref(nl))
        _check(ns < 0, "host_nuts_run: ")
        return {"samples": samples[:ns], "sample_values": values[:ns], "epsilon_trace": eps[:ns], "depth_trace": depth[:ns],
                "best": best, "best_value": bv.value, "gradient_calls": nc.value, "gradient_launches": nl.value}

    def nuts_chains(self, theta0, seed0: int, iterations: int, adaptation_window: int, max_tree_depth: int = 10,
                    delta_target: float = 0.8, fd_epsilon: float = 1e-4, constraint_mode: int = 1, device: int = -1,
                    kernel_timing: bool = False) -> dict:
        """MultiChainNUTSSampler: C = len(theta0) No-U-Turn chains in lock step over the finite-difference objective,
        chain c from theta0[c] with std::mt19937(seed0 + c) -- each equal to nuts(theta0[c], seed0 + c, ...) -- every
        tick's requests in one sepaihrd_fd_gradient_batch.  Arrays have a leading chain axis: samples [C][iterations][P]
        and sample_values [C][iterations] go straight into chain_diagnostics (rows past n_samples[c] are NaN: a chain
        that stopped on an integration failure, failure_status[c] >= 2 in iteration failure_iteration[c], or began
        with non-finite values); gradient_calls counts what nuts() counts, rows_evaluated the rows that ran."""
        th = np.ascontiguousarray(np.atleast_2d(theta0), dtype=np.float64)
        if th.shape[1] != self.P:
            raise ValueError(f"theta0 must be C x {self.P}")
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        out, stats, ptrs = _nuts_chains_outputs(th.shape[0], iterations, self.P)
        _check(self.lib.host_nuts_chains_run(self.h, C.byref(st), device, iterations, adaptation_window, delta_target,
                                             max_tree_depth, fd_epsilon, constraint_mode, th.shape[0], th.ctypes.data, seed0,
                                             int(kernel_timing), *ptrs), "host_nuts_chains_run: ")
        out.update(ticks=int(stats[0]), rows_total=int(stats[1]), mean_rows_per_tick=stats[1] / stats[0] if stats[0] > 0 else 0.0,
                   seconds=stats[2], evaluation_seconds=stats[3], centre_kernel_ms=stats[4], perturbed_kernel_ms=stats[5])
        return out

    def calibrate(self, hc_seed: int, mh_seed: int, hc_iterations: int, mh_iterations: int, burn_in: int,
                  cloud_size_multiplier: int = 8, threads: int = 16, adaptation_period: int = 100, thinning: int = 1,
                  chains: int = 1) -> dict:
        """HipModelCalibrator: HC (clamp) -> covariance conditioning -> `chains` MH chains (reflect)."""
        return _calibration(self.lib.host_calibrate, (self.h, hc_iterations, cloud_size_multiplier, threads, hc_seed, mh_iterations, burn_in,
                                                      adaptation_period, thinning, mh_seed, chains),
                            "host_calibrate: ", self.P, chains, mh_iterations, thinning)

    def calibrate_pso(self, pso_settings: dict, mh_seed: int, mh_iterations: int, burn_in: int,
                      adaptation_period: int = 100, thinning: int = 1, chains: int = 1) -> dict:
        """HipModelCalibrator with the particle swarm as phase 1 (SEPAIHRDModelCalibration::runPSOMCMC)."""
        keys = (C.c_char_p * len(pso_settings))(*[k.encode() for k in pso_settings])
        vals = np.array([float(v) for v in pso_settings.values()])
        return _calibration(self.lib.host_calibrate_pso, (self.h, keys, vals.ctypes.data, len(pso_settings), mh_iterations, burn_in,
                                                          adaptation_period, thinning, mh_seed, chains),
                            "host_calibrate_pso: ", self.P, chains, mh_iterations, thinning)

    def posterior_ensemble(self, samples, num_for_ppc: int, seed: int, burn_in: int = 0, thinning: int = 1,
                           want_sero: bool = True, want_rt: bool = False, device: int = -1) -> dict:
        """HipPosteriorEnsemble::aggregatePosteriorPredictives (+ aggregateSeroprevalence) over this handle's
        parameter manager and data.  ppc: [6][5: lower_95, lower_90, median, upper_90, upper_95][T_pos][n]."""
        ps = np.ascontiguousarray(np.atleast_2d(samples), dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        n, T = self.pb.n, self.pb.n_times
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        ppc = np.empty((6, 5, Tp, n))
        sel = np.empty(max(ps.shape[0], num_for_ppc, 1), dtype=np.int32)
        nsel, used = C.c_int32(0), C.c_int32(0)
        sero = np.empty((5, T)) if want_sero else None
        rt = np.empty((5, T)) if want_rt else None
        _check(self.lib.host_ensemble(self.h, C.byref(st), device, ps.ctypes.data, ps.shape[0], num_for_ppc, seed,
                                      ppc.ctypes.data, sel.ctypes.data, C.byref(nsel), C.byref(used), burn_in, thinning,
                                      sero.ctypes.data if want_sero else None, rt.ctypes.data if want_rt else None), "host_ensemble: ")
        return {"ppc": ppc, "selected": sel[:nsel.value].copy(), "samples_used": used.value, "sero": sero, "rt": rt}

    def posterior_predictive(self, samples, num_for_ppc: int, ppc_seed: int, R: int, seed: int,
                             probs=(0.025, 0.05, 0.5, 0.95, 0.975), want_means: bool = False, want_draws: bool = False,
                             device: int = -1) -> dict:
        """HipPosteriorPredictive::draw over this handle's parameter manager and data: the samples picked by the PPC rule of
        posterior_ensemble, R replicates each -- Poisson, or negative-binomial where the objective is dispersed (set_dispersion on
        this handle, or calibrated dispersion_* names): then `dispersed` is True and k_used [S][3] holds every sample's dispersions.
        pred [6][n_probs][T_pos][n], pit and observed [3][T_pos][n], selected, status, samples_used; means [S][3][T_pos][n] and
        draws [S][R][3][T_pos][n] on request."""
        ps = np.ascontiguousarray(np.atleast_2d(samples), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        n = self.pb.n
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        cap = max(ps.shape[0], num_for_ppc, 1)
        S = num_for_ppc if 0 < num_for_ppc < ps.shape[0] else ps.shape[0]
        pred, pit, obs = np.empty((6, pr.size, Tp, n)), np.empty((3, Tp, n)), np.empty((3, Tp, n))
        means = np.empty((S, 3, Tp, n)) if want_means else None
        draws = np.empty((S, max(int(R), 0), 3, Tp, n)) if want_draws else None
        sel, status = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        nsel, used, dispersed = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        k_used = np.full((cap, 3), np.inf)
        _check(self.lib.host_predictive_dispersed(self.h, C.byref(st), device, ps.ctypes.data, ps.shape[0], num_for_ppc, ppc_seed, int(R),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, pr.size, pred.ctypes.data, pit.ctypes.data,
                                                  obs.ctypes.data, means.ctypes.data if want_means else None,
                                                  draws.ctypes.data if want_draws else None, k_used.ctypes.data, C.byref(dispersed),
                                                  sel.ctypes.data, C.byref(nsel), status.ctypes.data, C.byref(used)), "host_predictive: ")
        out = {"pred": pred, "pit": pit, "observed": obs, "selected": sel[:nsel.value].copy(), "status": status[:nsel.value].copy(),
               "samples_used": used.value, "dispersed": bool(dispersed.value), "k_used": k_used[:nsel.value].copy()}
        if want_means:
            out["means"] = means
        if want_draws:
            out["draws"] = draws
        return out

    def posterior_predictive_scores(self, samples, num_for_ppc: int, ppc_seed: int, R: int, seed: int, probs, levels, observed=None,
                                    want_means: bool = False, want_draws: bool = False, device: int = -1) -> dict:
        """HipPosteriorPredictive::score over this handle's parameter manager and data: posterior_predictive's selection and
        dispersion rule through sepaihrd_ensemble_predictive_scores.  pred, pit, cell_scores [3][T_pos][n][5 + 4 L], summary
        [3][n + 1][4 + 2 L], exact, k_used, selected, status, samples_used; means and draws on request.  observed [3][T_pos][n]
        (None: the handle's data) is the table scored against."""
        ps = np.ascontiguousarray(np.atleast_2d(samples), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        n, L = self.pb.n, lv.size
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        ob = None if observed is None else np.ascontiguousarray(observed, dtype=np.float64)
        if ob is not None and ob.shape != (3, Tp, n):
            raise ValueError("observed must be [3][T_pos][n]")
        cap = max(ps.shape[0], num_for_ppc, 1)
        S = num_for_ppc if 0 < num_for_ppc < ps.shape[0] else ps.shape[0]
        pred, pit = np.empty((6, pr.size, Tp, n)), np.empty((3, Tp, n))
        cell_scores, summary = np.empty((3, Tp, n, 5 + 4 * L)), np.empty((3, n + 1, 4 + 2 * L))
        means = np.empty((S, 3, Tp, n)) if want_means else None
        draws = np.empty((S, max(int(R), 0), 3, Tp, n)) if want_draws else None
        sel, status = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        nsel, used, exact = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        k_used = np.full((cap, 3), np.inf)
        _check(self.lib.host_predictive_scores(self.h, C.byref(st), device, ps.ctypes.data, ps.shape[0], num_for_ppc, ppc_seed, int(R),
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, pr.size, lv.ctypes.data, L,
                                               None if ob is None else ob.ctypes.data, pred.ctypes.data, pit.ctypes.data,
                                               cell_scores.ctypes.data, summary.ctypes.data, means.ctypes.data if want_means else None,
                                               draws.ctypes.data if want_draws else None, k_used.ctypes.data, C.byref(exact),
                                               sel.ctypes.data, C.byref(nsel), status.ctypes.data, C.byref(used)), "host_predictive_scores: ")
        out = {"pred": pred, "pit": pit, "cell_scores": cell_scores, "summary": summary, "exact": bool(exact.value),
               "selected": sel[:nsel.value].copy(), "status": status[:nsel.value].copy(), "samples_used": used.value,
               "k_used": k_used[:nsel.value].copy()}
        if want_means:
            out["means"] = means
        if want_draws:
            out["draws"] = draws
        return out

    def posterior_predictive_targets(self, samples, num_for_ppc: int, ppc_seed: int, R: int, seed: int, probs, levels, age_group,
                                     window: int, origin: int = 0, observed=None, want_target_draws: bool = False, device: int = -1) -> dict:
        """HipPosteriorPredictive::scoreTargets over this handle's parameter manager and data: posterior_predictive_scores'
        selection and dispersion rule through sepaihrd_ensemble_predictive_targets.  target_quantiles, pit, target_obs,
        target_scores, summary, exact, W, G, k_used, selected, status, samples_used; target_draws on request."""
        ps = np.ascontiguousarray(np.atleast_2d(samples), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
        ag = np.ascontiguousarray(age_group, dtype=np.int32).ravel()
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        n, L = self.pb.n, lv.size
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        ob = None if observed is None else np.ascontiguousarray(observed, dtype=np.float64)
        if ob is not None and ob.shape != (3, Tp, n):
            raise ValueError("observed must be [3][T_pos][n]")
        cap = max(ps.shape[0], num_for_ppc, 1)
        S = num_for_ppc if 0 < num_for_ppc < ps.shape[0] else ps.shape[0]
        W, G = hipabi.predictive_targets_validate(S, R, Tp, n, ag, window, origin, pr, lv)
        tq, pit, tobs = np.empty((6, pr.size, W, G)), np.empty((6, W, G)), np.empty((6, W, G))
        tscores, summary = np.empty((6, W, G, 5 + 4 * L)), np.empty((6, G + 1, 4 + 2 * L))
        tdraws = np.empty((S, max(int(R), 0), 3, W, G)) if want_target_draws else None
        sel, status = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        nsel, used, exact = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        k_used = np.full((cap, 3), np.inf)
        _check(self.lib.host_predictive_targets(self.h, C.byref(st), device, ps.ctypes.data, ps.shape[0], num_for_ppc, ppc_seed, int(R),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, pr.size, lv.ctypes.data, L, ag.ctypes.data,
                                                ag.size, int(window), int(origin), None if ob is None else ob.ctypes.data, tq.ctypes.data,
                                                pit.ctypes.data, tscores.ctypes.data, summary.ctypes.data, tobs.ctypes.data,
                                                None if tdraws is None else tdraws.ctypes.data, k_used.ctypes.data, C.byref(exact),
                                                sel.ctypes.data, C.byref(nsel), status.ctypes.data, C.byref(used)), "host_predictive_targets: ")
        out = {"target_quantiles": tq, "pit": pit, "target_obs": tobs, "target_scores": tscores, "summary": summary,
               "exact": bool(exact.value), "W": W, "G": G, "selected": sel[:nsel.value].copy(), "status": status[:nsel.value].copy(),
               "samples_used": used.value, "k_used": k_used[:nsel.value].copy()}
        if want_target_draws:
            out["target_draws"] = tdraws
        return out

    def posterior_stochastic(self, samples, num_samples: int, select_seed: int, R: int, steps_per_interval: int, seed: int,
                             probs=(0.025, 0.05, 0.5, 0.95, 0.975), initial_state_mode: int = 1, device: int = -1) -> dict:
        """HipStochasticSEPAIHRD::run over this handle's parameter manager and data: the samples picked by the PPC rule of
        posterior_ensemble, R chain-binomial replicates each.  quantiles [6][n_probs][T_pos][n], extinct, selected, status,
        samples_used."""
        ps = np.ascontiguousarray(np.atleast_2d(samples), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        cap = max(ps.shape[0], num_samples, 1)
        q = np.empty((6, pr.size, Tp, self.pb.n))
        extinct, sel, status = np.empty(cap), np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        nsel, used = C.c_int32(0), C.c_int32(0)
        _check(self.lib.host_stochastic(self.h, C.byref(st), device, int(initial_state_mode), ps.ctypes.data, ps.shape[0], num_samples,
                                        select_seed, int(R), int(steps_per_interval), int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, pr.size,
                                        q.ctypes.data, extinct.ctypes.data, sel.ctypes.data, C.byref(nsel), status.ctypes.data, C.byref(used)),
               "host_stochastic: ")
        k = nsel.value
        return {"quantiles": q, "extinct": extinct[:k].copy(), "selected": sel[:k].copy(), "status": status[:k].copy(),
                "samples_used": used.value}

    def particle_filter_states(self, thetas, J: int, steps_per_interval: int, seed0: int, probs, n_calls_before: int = 0,
                               initial_state_mode: int = 0, device: int = -1, dispersion=None) -> dict:
        """HipParticleLikelihood::filterStates after n_calls_before calculateBatch calls, then one more calculateBatch: state_mean
        [B][T][11][n + 1], state_quantiles [B][T][11][n + 1][len(probs)], loglik [B] of the filterStates call, next_values [B] of
        the calculateBatch after it, calls (the adapter's call count before and after filterStates)."""
        th = np.ascontiguousarray(np.atleast_2d(thetas), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        B, n, T = th.shape[0], self.pb.n, len(self.pb.times)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        mean, quant = np.empty((B, T, 11, n + 1)), np.empty((B, T, 11, n + 1, pr.size))
        loglik, nxt, calls = np.empty(B), np.empty(B), np.zeros(2, dtype=np.uint64)
        disp = None if dispersion is None else _dispersion(dispersion)
        _check(self.lib.host_particle_filter_states(self.h, C.byref(st), device, int(initial_state_mode), int(J), int(steps_per_interval),
                                                    int(seed0) & 0xFFFFFFFFFFFFFFFF, None if disp is None else disp.ctypes.data, th.ctypes.data, B,
                                                    int(n_calls_before), pr.ctypes.data, pr.size, mean.ctypes.data, quant.ctypes.data,
                                                    loglik.ctypes.data, nxt.ctypes.data, calls.ctypes.data), "host_particle_filter_states: ")
        return {"state_mean": mean, "state_quantiles": quant, "loglik": loglik, "next_values": nxt, "calls": calls}

    def particle_likelihood(self, thetas, J: int, steps_per_interval: int, seed0: int, n_calls: int = 1, initial_state_mode: int = 0,
                            device: int = -1, dispersion=None) -> dict:
        """HipParticleLikelihood over this handle's parameter manager and data: n_calls successive calculateBatch calls on the same
        rows of thetas; call c runs at seed0 + c.  values [n_calls][B], status [n_calls][B].  dispersion = (k_H, k_ICU, k_D): the
        calls run after setDispersion (None: the adapter's default, every series Poisson)."""
        th = np.ascontiguousarray(np.atleast_2d(thetas), dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        B = th.shape[0]
        values, status = np.empty((n_calls, B)), np.empty((n_calls, B), dtype=np.int32)
        if dispersion is not None:
            disp = _dispersion(dispersion)
            _check(self.lib.host_particle_likelihood_nb(self.h, C.byref(st), device, int(initial_state_mode), int(J), int(steps_per_interval),
                                                        int(seed0) & 0xFFFFFFFFFFFFFFFF, disp.ctypes.data, th.ctypes.data, B, int(n_calls),
                                                        values.ctypes.data, status.ctypes.data), "host_particle_likelihood_nb: ")
            return {"values": values, "status": status}
        _check(self.lib.host_particle_likelihood(self.h, C.byref(st), device, int(initial_state_mode), int(J), int(steps_per_interval),
                                                 int(seed0) & 0xFFFFFFFFFFFFFFFF, th.ctypes.data, B, int(n_calls), values.ctypes.data,
                                                 status.ctypes.data), "host_particle_likelihood: ")
        return {"values": values, "status": status}

    def stochastic_manager_values(self, theta, mode: int) -> np.ndarray:
        """The parameter part of a model_values row of sepaihrd_ensemble_stochastic (all but the 11 n initial counts) as this
        handle's parameter manager writes it: updateModelParameters(theta) in the given constraint mode."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        W = stochastic_values_width(self.pb.n, len(self.pb.beta_end_times), len(self.pb.kappa_end_times)) - 11 * self.pb.n
        out = np.empty(W)
        _check(self.lib.host_stochastic_manager_values(self.h, int(mode), th.ctypes.data, out.ctypes.data), "host_stochastic_manager_values: ")
        return out

    def scenario_comparison(self, samples, burn_in: int = 0, thinning: int = 1, path: str | None = None, device: int = -1) -> dict:
        """The reference's scenario step (PostCalibrationAnalyser.cpp:94-141): the default lockdown scenarios of the last
        analysed sample, through HipPosteriorEnsemble::performScenarioAnalysis; writes scenario_comparison.csv to path.
        names [rows], metrics [rows][12 + 4 n], kappa [rows][n_kappa] (the scenario's own kappa_values)."""
        ps = np.ascontiguousarray(np.atleast_2d(samples), dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        met = np.empty((3, 12 + 4 * self.pb.n))
        kap = np.empty((3, len(self.pb.kappa_values)))
        rows = C.c_int32(0)
        _check(self.lib.host_scenario_comparison(self.h, C.byref(st), device, ps.ctypes.data, ps.shape[0], burn_in, thinning,
                                                 path.encode() if path else None, met.ctypes.data, kap.ctypes.data, C.byref(rows)),
               "host_scenario_comparison: ")
        names = ["baseline", "stricter_lockdown", "weaker_lockdown"][:rows.value]
        return {"names": names, "metrics": met[:rows.value].copy(), "kappa": kap[:rows.value].copy()}

    def ene_covid_validation(self, samples, path: str, burn_in: int = 0, thinning: int = 1, device: int = -1) -> None:
        """seroprevalence/ene_covid_validation.csv from the metric summary of the samples (PostCalibrationAnalyser.cpp:288-299)."""
        ps = np.ascontiguousarray(np.atleast_2d(samples), dtype=np.float64)
        keep: list = []
        st = hipabi.build_problem_struct(self.pb, keep)
        _check(self.lib.host_ene_covid_validation(self.h, C.byref(st), device, ps.ctypes.data, ps.shape[0], burn_in, thinning, path.encode()),
               "host_ene_covid_validation: ")

    def set_mh_diagnostics(self, on: bool) -> None:
        """Convergence diagnostics for the following metropolis_hastings(device_state=True) / calibrate / calibrate_pso runs
        (MultiChainMetropolisHastings::setComputeDiagnostics)."""
        self.lib.host_set_mh_diagnostics(self.h, int(bool(on)))

    def mh_diagnostics(self):
        """The last such run's table [P (+ 1 values row)][7] (columns hipabi.DIAG_COLUMNS), or None when it formed none."""
        rows = C.c_int32(0)
        self.lib.host_mh_diagnostics(self.h, None, C.byref(rows))
        if rows.value == 0:
            return None
        out = np.empty((rows.value, len(hipabi.DIAG_COLUMNS)))
        self.lib.host_mh_diagnostics(self.h, out.ctypes.data, C.byref(rows))
        return out

    def chain_diagnostics(self, samples, values=None) -> dict:
        """HipChainDiagnostics::compute over host draws samples [C][N][P] (+ values [C][N]) on this handle's device:
        table [P (+ 1)][7], max_lag [..][4] (the NUTS trace or any other sample set)."""
        s = np.ascontiguousarray(samples, dtype=np.float64)
        Cn, N, P = s.shape
        v = None if values is None else np.ascontiguousarray(np.reshape(values, (Cn, N)), dtype=np.float64)
        rows = P + (0 if v is None else 1)
        out = np.empty((rows, len(hipabi.DIAG_COLUMNS)))
        lag = np.empty((rows, 4), dtype=np.int32)
        _check(self.lib.host_chain_diagnostics(self.h, s.ctypes.data, None if v is None else v.ctypes.data, Cn, N, P,
                                               out.ctypes.data, lag.ctypes.data), "host_chain_diagnostics: ")
        return {"table": out, "columns": list(hipabi.DIAG_COLUMNS), "max_lag": lag}

    def calculate(self, theta) -> float:
        th = np.ascontiguousarray(theta, dtype=np.float64)
        v = C.c_double()
        _check(self.lib.host_objective_calculate(self.h, th.ctypes.data, C.byref(v)))
        return v.value

    def calculate_batch(self, thetas):
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        B = th.shape[0]
        out = np.empty(B)
        status = np.empty(B, dtype=np.int32)
        _check(self.lib.host_objective_calculate_batch(self.h, th.ctypes.data, B, out.ctypes.data, status.ctypes.data))
        return out, status

    def cache_stats(self):
        a, b, c = C.c_long(), C.c_long(), C.c_long()
        self.lib.host_cache_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        return {"calls": a.value, "hits": b.value, "size": c.value}

    def apply_constraints(self, theta, mode: int) -> np.ndarray:
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        out = np.empty_like(th)
        for b in range(th.shape[0]):
            self.lib.host_apply_constraints(self.h, mode, th[b].ctypes.data, out[b].ctypes.data)
        return out

    def current_parameters(self) -> np.ndarray:
        out = np.empty(self.P)
        self.lib.host_current_parameters(self.h, out.ctypes.data)
        return out

    def metropolis_hastings_reported(self, initial, seed: int, iterations: int, burn_in: int, out_dir: str, log_path: str,
                                     adaptation_period: int = 100, thinning: int = 1, report_interval: int = 100,
                                     checkpoint_chains: int = 1, device_state: bool = True, device_streams: bool = True) -> dict:
        """The sampler with the reference's progress reports and trace files ON (MetropolisHastingsSampler.cpp:363-383,
        399-411,440-469): lines into log_path, posterior_trace_checkpoint.csv / _final.csv / posterior_trace.csv into out_dir."""
        x0 = np.ascontiguousarray(np.atleast_2d(initial), dtype=np.float64)
        Cn, P = x0.shape
        a = _mh_arrays(Cn, P, iterations, thinning, keys=("samples", "sample_values"))
        ns, fb = C.c_int32(), C.c_int()
        failures = (C.c_long * 3)()
        _check(self.lib.host_mh_run_reported(self.h, Cn, x0.ctypes.data, seed, iterations, burn_in, adaptation_period, thinning,
                                             report_interval, checkpoint_chains, int(device_state), int(device_streams),
                                             out_dir.encode(), log_path.encode(), _ptr(a["samples"]), _ptr(a["sample_values"]),
                                             C.byref(ns), C.byref(fb), failures))
        return _mh_result(a, iterations, ns.value, fell_back=bool(fb.value), failures=list(failures))

    def metropolis_hastings(self, initial, seed: int, iterations: int, burn_in: int, adaptation_period: int = 100,
                            thinning: int = 1, reg_eps: float = 1e-6, target_acc: float = 0.234,
                            adapt_scale: bool = True, scalar_interface: bool = False, device_state: bool = False,
                            two_pass_covariance: bool = False, want_trace: bool = True, adaptation_window: int = 0,
                            device_streams: bool = True) -> dict:
        """MultiChainMetropolisHastings (MetropolisHastingsSampler.cpp:201-412 for C lock-step chains): host-state loop,
        scalar interface, or (device_state) adaptation state resident in HBM.  two_pass_covariance: the reference's
        literal covariance refresh over the whole history instead of running co-moments.  device_streams (device_state
        only): the chains' mt19937 streams drawn on the device (default) or on the host."""
        x0 = np.ascontiguousarray(np.atleast_2d(initial), dtype=np.float64)
        Cn, P = x0.shape
        a = _mh_arrays(Cn, P, iterations, thinning, want_trace)
        ns = C.c_int32()
        ptrs = [_ptr(a[k]) for k in _MH_ARRAYS]
        _check(self.lib.host_mh_run(self.h, Cn, x0.ctypes.data, seed, iterations, burn_in, adaptation_period, thinning,
                                    reg_eps, target_acc, int(adapt_scale), 2 if device_state else int(scalar_interface),
                                    *ptrs[:5], C.byref(ns), *ptrs[5:7], int(two_pass_covariance), ptrs[7], int(adaptation_window),
                                    int(device_streams)))
        return _mh_result(a, iterations, ns.value, loop_seconds=float(self.lib.host_last_mh_loop_seconds()))


def libm_selfcheck() -> dict:
    """The host twin of sepaihrd_device_libm_check (no device): csrc/sepaihrd_rng.inc's log / exp compiled for the host
    against this process's std::log / std::exp on the self-check arguments; also returns the arguments."""
    lib = load_library()
    n, dl, de = C.c_int(), C.c_int(), C.c_int()
    lib.host_libm_selfcheck(C.byref(n), C.byref(dl), C.byref(de))
    la, ea = np.empty(n.value), np.empty(n.value)
    lib.host_libm_selfcheck_args(la.ctypes.data, ea.ctypes.data)
    return {"n": n.value, "log_diff": dl.value, "exp_diff": de.value, "log_args": la, "exp_args": ea}


def metropolis_hastings_groups(objectives, initial, seed: int, iterations: int, burn_in: int, adaptation_period: int = 100,
                               thinning: int = 1) -> dict:
    """MultiChainMetropolisHastings::optimizeChainGroupsOnDevice over len(objectives) HostObjective handles
    (one device context, stream and host thread per group of chains)."""
    lib = load_library()
    x0 = np.ascontiguousarray(np.atleast_2d(initial), dtype=np.float64)
    Cn, P = x0.shape
    G = len(objectives)
    handles = (C.c_void_p * G)(*[o.h for o in objectives])
    a = _mh_arrays(Cn, P, iterations, keys=("accepted", "best_value", "best", "accept_trace"))
    _check(lib.host_mh_run_groups(handles, G, Cn, x0.ctypes.data, seed, iterations, burn_in, adaptation_period, thinning,
                                  *[_ptr(v) for v in a.values()]))
    return _mh_result(a, iterations, loop_seconds=float(lib.host_last_mh_loop_seconds()))


def reference_constructors(pb, thetas) -> dict:
    """The objective and the parameter manager built with the REFERENCE's constructor argument lists
    (model first; SEPAIHRDModelCalibration.cpp:84-118): values[manager][mode][b] of calculate() for a Hip manager
    built from the model and for a manager of another type, and the calibrated entries read back from the model
    after updateModelParameters(thetas[0])."""
    lib = load_library()
    keep: list = []
    st = hipabi.build_problem_struct(pb, keep)
    sig = np.ascontiguousarray(pb.sigma_array())
    th = np.ascontiguousarray(np.atleast_2d(thetas), dtype=np.float64)
    B, P = th.shape
    values = np.empty((2, 2, B))
    back = np.empty(P)
    _check(lib.host_reference_constructors(C.byref(st), "\n".join(pb.param_names).encode(), "\n".join(pb.npi_names).encode(),
                                           sig.ctypes.data, th.ctypes.data, B, values.ctypes.data, back.ctypes.data),
           "host_reference_constructors: ")
    return {"values": values, "model_back": back}


def model_holders(ends_after, values_after, baseline, baseline_end, t) -> dict:
    """PiecewiseConstantNpiStrategy::getReductionFactor at times t and what AgeSEPAIHRDModel reports (no device)."""
    lib = load_library()
    ea = np.ascontiguousarray(ends_after, dtype=np.float64)
    va = np.ascontiguousarray(values_after, dtype=np.float64)
    tt = np.ascontiguousarray(t, dtype=np.float64)
    kap = np.empty(len(tt))
    se, sv = np.empty(len(ea) + 1), np.empty(len(ea) + 1)
    size = C.c_int()
    buf = C.create_string_buffer(128)
    rc = lib.host_model_holders(ea.ctypes.data, va.ctypes.data, len(ea), baseline, baseline_end, tt.ctypes.data, len(tt),
                                kap.ctypes.data, se.ctypes.data, sv.ctypes.data, C.byref(size), buf, len(buf))
    _check(rc, "host_model_holders: rc %d " % rc)
    return {"kappa": kap, "schedule_ends": se, "schedule_values": sv, "state_size": size.value, "names": buf.value.decode()}


def summary_quantiles(table, probs) -> np.ndarray:
    """MultiChainMetropolisHastings::summaryQuantiles (pure host): exact-sort quantiles across chains of every column."""
    lib = load_library()
    t = np.ascontiguousarray(table, dtype=np.float64)
    q = np.ascontiguousarray(probs, dtype=np.float64)
    out = np.empty((len(q), t.shape[1]))
    _check(lib.host_summary_quantiles(t.ctypes.data, t.shape[0], t.shape[1], q.ctypes.data, len(q), out.ctypes.data))
    return out


def metropolis_hastings_group_summaries(objectives, initial, seed: int, iterations: int, burn_in: int, adaptation_period: int = 100,
                                        thinning: int = 1, backend: int = 0) -> dict:
    """optimizeChainGroupsOnDevice + gatherChainSummaries: the per-chain summary records (host concatenation), the table
    every group's device holds after the all-gather, and the samples they were formed from."""
    lib = load_library()
    x0 = np.ascontiguousarray(np.atleast_2d(initial), dtype=np.float64)
    Cn, P = x0.shape
    G = len(objectives)
    W = 2 * P + 2
    handles = (C.c_void_p * G)(*[o.h for o in objectives])
    out = {"records": np.zeros((Cn, W)), "gathered": np.zeros((G, Cn, W))}
    out.update(_mh_arrays(Cn, P, iterations, thinning, keys=("samples", "best_value", "accepted")))
    used = C.c_int32(-1)
    _check(lib.host_mh_groups_summaries(handles, G, Cn, x0.ctypes.data, seed, iterations, burn_in, adaptation_period, thinning, backend,
                                        *[_ptr(v) for v in out.values()], C.byref(used)))
    return _mh_result(out, iterations, backend_used=int(used.value))


def default_arith() -> int:
    """ARITH_* the reference-shaped constructors of the C++ adapters select (environment SEPAIHRD_ARITH; fma unless
    "strict").  No device needed."""
    lib = load_library()
    return int(lib.host_default_arith())


def glibc_log(x) -> np.ndarray:
    """csrc/sepaihrd_rng.inc's restatement of glibc's log, compiled for the host (test hook)."""
    lib = load_library()
    a = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(a)
    lib.host_glibc_log(a.ctypes.data, a.size, out.ctypes.data)
    return out


def glibc_exp(x) -> np.ndarray:
    """csrc/sepaihrd_rng.inc's restatement of glibc's exp, compiled for the host (test hook)."""
    lib = load_library()
    a = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(a)
    lib.host_glibc_exp(a.ctypes.data, a.size, out.ctypes.data)
    return out


def sir_rhs(N, Cm, gamma, q, scale_C, state) -> np.ndarray:
    """The host AgeSIRModel::computeDerivatives (C++; no device)."""
    N, Cm, gamma, state = (np.ascontiguousarray(a, dtype=np.float64) for a in (N, Cm, gamma, state))
    out = np.empty_like(state)
    lib = load_library()
    _check(lib.host_sir_rhs(len(N), N.ctypes.data, Cm.ctypes.data, gamma.ctypes.data, q, scale_C, state.ctypes.data, out.ctypes.data),
           "host_sir_rhs: ")
    return out


def sir_scenario_events(times, entries) -> list:
    """One scenario through the C++ SIRScenario::addIntervention (no device): ``entries`` are (time, name, params) with the
    reference's intervention names; returns the events [(time_index, kind, value)] in schedule order.  Raises ValueError for
    what the C++ side throws as InvalidParameterException and RuntimeError for any other exception."""
    lib = load_library()
    t = np.ascontiguousarray(times, dtype=np.float64)
    ev_t = np.array([float(e[0]) for e in entries] + [0.0])
    counts = np.array([len(np.atleast_1d(e[2])) for e in entries] + [0], dtype=np.int32)
    params = np.array([float(v) for e in entries for v in np.atleast_1d(e[2])] + [0.0])
    m = len(entries)
    ti, kind, val = np.zeros(m + 1, dtype=np.int32), np.zeros(m + 1, dtype=np.int32), np.zeros(m + 1)
    n = C.c_int(0)
    rc = lib.host_sir_scenario_events(t.ctypes.data, t.size, m, ev_t.ctypes.data, "\n".join(e[1] for e in entries).encode(), counts.ctypes.data,
                                      params.ctypes.data, ti.ctypes.data, kind.ctypes.data, val.ctypes.data, C.byref(n))
    if rc == 1:
        raise ValueError(lib.host_last_error().decode())
    _check(rc)
    return [(int(ti[e]), int(kind[e]), float(val[e])) for e in range(n.value)]


def write_sir_scenario_csvs(comparison_path, bands_path, scenario_names, times, probs, n_age, quantiles=None, metric_summary=None,
                            diff_quantiles=None):
    """HipSIRScenarioAnalysis::writeScenarioComparison / writePosteriorBands on arrays (no device); a None path skips the file."""
    lib = load_library()
    t, pr = np.ascontiguousarray(times, dtype=np.float64), np.ascontiguousarray(probs, dtype=np.float64)
    arr = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (quantiles, metric_summary, diff_quantiles)]
    _check(lib.host_sir_write_scenario_csvs(None if comparison_path is None else str(comparison_path).encode(),
                                            None if bands_path is None else str(bands_path).encode(), "\n".join(scenario_names).encode(),
                                            len(scenario_names), int(n_age), t.size, t.ctypes.data, pr.ctypes.data, pr.size,
                                            *[None if a is None else a.ctypes.data for a in arr]), "host_sir_write_scenario_csvs: ")


class HostSIRObjective:
    """AgeSIRModel + HipSIRParameterManager + SimulationCache + HipPoissonLikelihoodObjective (C++ objects).
    ``param_names`` overrides the problem's (the manager's name errors are the C++ ones); ``with_objective=False`` builds
    model and manager only and needs no device."""

    def __init__(self, pb, device: int = -1, cache_capacity: int = 1000, with_objective: bool = True, param_names=None,
                 sigmas: dict | None = None):
        self.lib = load_library()
        self.pb = pb
        names = list(pb.param_names if param_names is None else param_names)
        keep: list = []
        st = hipabi.build_sir_problem_struct(pb, keep)
        sg = dict(sigmas or {})
        sv = np.array(list(sg.values()) + [0.0])
        self.h = self.lib.host_sir_create(C.byref(st), "\n".join(names).encode(), "\n".join(sg.keys()).encode(), sv.ctypes.data,
                                          device, cache_capacity, int(with_objective))
        _check(not self.h, "host_sir_create failed: ")
        self.P, self.n = len(names), pb.n

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.host_sir_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def manager_info(self) -> dict:
        out = [np.empty(self.P) for _ in range(4)]
        _check(self.lib.host_sir_manager_info(self.h, *[a.ctypes.data for a in out]), "host_sir_manager_info: ")
        return dict(zip(("sigma", "lower", "upper", "current"), out))

    def index_for_param(self, name: str) -> int:
        return int(self.lib.host_sir_index_for_param(self.h, name.encode()))

    def apply_constraints(self, theta) -> np.ndarray:
        th = np.ascontiguousarray(theta, dtype=np.float64)
        out = np.empty(self.P)
        self.lib.host_sir_apply_constraints(self.h, th.ctypes.data, out.ctypes.data)
        return out

    def update_model(self, theta) -> dict:
        th = np.ascontiguousarray(theta, dtype=np.float64)
        q, sc, g = C.c_double(0.0), C.c_double(0.0), np.empty(self.n)
        _check(self.lib.host_sir_update_model(self.h, th.ctypes.data, C.byref(q), C.byref(sc), g.ctypes.data), "host_sir_update_model: ")
        return {"q": q.value, "scale_C_total": sc.value, "gamma": g}

    def calculate(self, theta) -> float:
        th = np.ascontiguousarray(theta, dtype=np.float64)
        v = C.c_double(0.0)
        _check(self.lib.host_sir_calculate(self.h, th.ctypes.data, C.byref(v)), "host_sir_calculate: ")
        return v.value

    def calculate_batch(self, thetas):
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        out, st = np.empty(len(th)), np.empty(len(th), dtype=np.int32)
        _check(self.lib.host_sir_calculate_batch(self.h, th.ctypes.data, len(th), out.ctypes.data, st.ctypes.data), "host_sir_calculate_batch: ")
        return out, st

    def cache_stats(self) -> dict:
        a, b, c = C.c_long(0), C.c_long(0), C.c_long(0)
        self.lib.host_sir_cache_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        return {"calls": a.value, "hits": b.value, "size": c.value}

    def hill_climbing(self, x0, seed: int, iterations: int, cloud_size_multiplier: int = 8, threads: int = 16) -> dict:
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        best, bv = np.empty(self.P), C.c_double(0.0)
        _check(self.lib.host_sir_hc_run(self.h, x0.ctypes.data, seed, threads, iterations, cloud_size_multiplier, best.ctypes.data, C.byref(bv)),
               "host_sir_hc_run: ")
        return {"best": best, "best_value": bv.value}

    def metropolis_hastings(self, initial, seed: int, iterations: int, burn_in: int = 0) -> dict:
        init = np.ascontiguousarray(initial, dtype=np.float64)
        chains = init.shape[0]
        bv, best, acc = np.empty(chains), np.empty((chains, self.P)), np.empty(chains, dtype=np.int32)
        _check(self.lib.host_sir_mh_run(self.h, chains, init.ctypes.data, seed, iterations, burn_in, bv.ctypes.data, best.ctypes.data,
                                        acc.ctypes.data), "host_sir_mh_run: ")
        return {"best_value": bv, "best": best, "accepted": acc}

    def metropolis_hastings_ex(self, initial, seed: int, iterations: int, burn_in: int = 0, adaptation_period: int = 100,
                               thinning: int = 1, reg_eps: float = 1e-6, target_acc: float = 0.234, adapt_scale: bool = True,
                               device_state: bool = True, device_streams: bool = True, two_pass_covariance: bool = False,
                               kernel_form: int = 0, want_trace: bool = True, adaptation_window: int = 0,
                               compute_diagnostics: bool = False, out_dir: str | None = None, log_path: str | None = None,
                               report_interval: int = 100, checkpoint_chains: int = 1) -> dict:
        """MultiChainMetropolisHastings on the SIR objective through either path: the host loop optimizeChains
        (device_state=False: every iteration through the host-pointer calculateBatch) or the device-resident sampler
        (sepaihrd_sir_mh_create).  Returns the dictionary HostObjective.metropolis_hastings returns, plus fell_back (the libm
        self-check refused the device streams), failures [3] and, with compute_diagnostics, diagnostics [P + 1][7].
        kernel_form: hipabi.MH_FORM_*.  out_dir switches the reference's progress reports and trace files on."""
        x0 = np.ascontiguousarray(np.atleast_2d(initial), dtype=np.float64)
        Cn, P = x0.shape
        a = _mh_arrays(Cn, P, iterations, thinning, want_trace)
        ptrs = [_ptr(a[k]) for k in _MH_ARRAYS]
        ns, fb, drows = C.c_int32(), C.c_int(), C.c_int32()
        failures = (C.c_long * 3)()
        diag = np.zeros((P + 1, len(hipabi.DIAG_COLUMNS)))
        _check(self.lib.host_sir_mh_run_ex(self.h, Cn, x0.ctypes.data, seed, iterations, burn_in, adaptation_period, thinning, reg_eps,
                                           target_acc, int(adapt_scale), int(device_state), int(device_streams), int(two_pass_covariance),
                                           int(adaptation_window), int(kernel_form), int(compute_diagnostics), int(report_interval),
                                           int(checkpoint_chains), out_dir.encode() if out_dir else None,
                                           log_path.encode() if log_path else None, *ptrs[:5], C.byref(ns), *ptrs[5:], C.byref(fb),
                                           failures, diag.ctypes.data, C.byref(drows)), "host_sir_mh_run_ex: ")
        return _mh_result(a, iterations, ns.value, loop_seconds=float(self.lib.host_last_mh_loop_seconds()), fell_back=bool(fb.value),
                          failures=list(failures), diagnostics=diag[:drows.value] if drows.value else None)

    def calibrate(self, hc_seed: int, mh_seed: int, hc_iterations: int, mh_iterations: int, burn_in: int,
                  cloud_size_multiplier: int = 8, threads: int = 16, adaptation_period: int = 100, thinning: int = 1,
                  chains: int = 1, kernel_form: int = 0, device_streams: bool = True) -> dict:
        """HipModelCalibrator on the SIR objective: Hill-Climbing from the manager's current parameters -> covariance
        conditioning -> `chains` device-resident MH chains -> the objective value of every stored sample.  The dictionary of
        HostObjective.calibrate."""
        return _calibration(self.lib.host_sir_calibrate, (self.h, hc_iterations, cloud_size_multiplier, threads, hc_seed, mh_iterations, burn_in,
                                                          adaptation_period, thinning, mh_seed, chains, int(kernel_form), int(device_streams)),
                            "host_sir_calibrate: ", self.P, chains, mh_iterations, thinning)

    def scenario_comparison(self, samples, scenarios, probs=(0.025, 0.05, 0.5, 0.95, 0.975), burn_in: int = 0, thinning: int = 1,
                            comparison_path: str | None = None, bands_path: str | None = None) -> dict:
        """HipSIRScenarioAnalysis (C++): the posterior ``samples`` [rows][P] after burn-in and thinning under the named
        ``scenarios`` -- {name: [(time, intervention name, value), ...]} with the reference's intervention names, the first
        one the baseline of the paired differences -- in one device call; writes sir_scenario_comparison.csv and
        sir_posterior_bands.csv to the given paths.  Returns the outputs of HipSIRObjective.scenario_ensemble."""
        ps = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, self.P)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        names = list(scenarios.keys())
        K, T, n = len(names), self.pb.n_times, self.n
        S = len(range(max(burn_in, 0), ps.shape[0], max(thinning, 1)))
        W = 6 + 2 * n
        counts = np.array([len(scenarios[k]) for k in names] + [0], dtype=np.int32)
        flat = [e for k in names for e in scenarios[k]]
        ev_t = np.array([float(e[0]) for e in flat] + [0.0])
        ev_v = np.array([float(e[2]) for e in flat] + [0.0])
        out = {"quantiles": np.empty((K, 3, pr.size, T, n + 1)), "metrics": np.empty((K, S, W)), "metric_summary": np.empty((K, W, 2 + pr.size)),
               "diff_quantiles": np.empty((K, W, pr.size)), "status": np.empty((K, S), dtype=np.int32), "n_valid": np.empty(K, dtype=np.int32)}
        _check(self.lib.host_sir_scenario_comparison(self.h, ps.ctypes.data, ps.shape[0], burn_in, thinning, "\n".join(names).encode(), K,
                                                     counts.ctypes.data, ev_t.ctypes.data, "\n".join(e[1] for e in flat).encode(), ev_v.ctypes.data,
                                                     pr.ctypes.data, pr.size, None if comparison_path is None else str(comparison_path).encode(),
                                                     None if bands_path is None else str(bands_path).encode(),
                                                     *[a.ctypes.data for a in out.values()]),
               "host_sir_scenario_comparison: ")
        out["scenario_names"], out["metric_names"] = names, hipabi.sir_metric_names(n)
        return out


# ---- stochastic chain-binomial SIR: the CPU twin of the device path and the pieces of csrc/sepaihrd_stoch.inc ----
STOCH_INFECTION, STOCH_RECOVERY = 0, 1
STOCH_HOST_TWIN = -2  # HipStochasticSIRModel::HOST_TWIN


def stoch_philox(counter, key) -> np.ndarray:
    """philox4x32_10(counter[4]; key[2]) -> 4 words"""
    c = np.ascontiguousarray(counter, dtype=np.uint32)
    k = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.empty(4, dtype=np.uint32)
    load_library().host_stoch_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return out


def stoch_uniform(lo: int, hi: int) -> float:
    """the stream's rule from two output words to a double inside (0, 1)"""
    return float(load_library().host_stoch_uniform(int(lo), int(hi)))


def stoch_probabilities(beta: float, I: float, h: float, N: float, gamma: float) -> tuple:
    """(pI, pR) of one step as the model text forms them"""
    a, b = C.c_double(), C.c_double()
    load_library().host_stoch_probabilities(beta, I, h, N, gamma, C.byref(a), C.byref(b))
    return a.value, b.value


def stoch_binomial_at(seed: int, group: int, replicate: int, step: int, transition: int, n: int, p: float) -> int:
    """the Binomial(n, p) variate at these coordinates of the stream"""
    return int(load_library().host_stoch_binomial_at(int(seed) & 0xFFFFFFFFFFFFFFFF, group, replicate, step, transition, int(n), float(p)))


def stoch_binomial_probe(n, p, seed: int) -> np.ndarray:
    """the twin of HipStochasticSIR.binomial"""
    n = np.ascontiguousarray(n, dtype=np.int32).ravel()
    p = np.ascontiguousarray(p, dtype=np.float64).ravel()
    out = np.empty(n.size, dtype=np.int32)
    load_library().host_stoch_binomial_probe(int(seed) & 0xFFFFFFFFFFFFFFFF, n.ctypes.data, p.ctypes.data, n.size, out.ctypes.data)
    return out


class HostStochasticSIR:
    """The CPU twin of HipStochasticSIR: the same model text on the host, OpenMP over replicates; same outputs bit for bit."""

    def __init__(self, pb):
        self.lib = load_library()
        self.pb = pb

    def run(self, replicates: int, seed: int, keep: int = 0, want_final: bool = False, max_workspace_bytes=None) -> dict:
        cfg = hipabi.stoch_sir_config(self.pb, replicates, seed, keep, max_workspace_bytes)
        tab = self.pb.group_table()
        err = C.create_string_buffer(512)
        if hipabi.load_library().sepaihrd_stoch_sir_validate(C.byref(cfg), tab.ctypes.data, err, len(err)) != 0:
            raise ValueError(err.value.decode())
        steps = hipabi.stoch_sir_num_steps(self.pb.t_start, self.pb.t_end, self.pb.h)
        out = hipabi.stoch_sir_outputs(self.pb, steps, int(replicates), int(keep), want_final)
        rc = self.lib.host_stoch_sir_run(C.byref(cfg), tab.ctypes.data, out["stats"].ctypes.data,
                                         None if out["traj"] is None else out["traj"].ctypes.data,
                                         None if out["final_state"] is None else out["final_state"].ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"host_stoch_sir_run failed ({rc}): " + err.value.decode())
        return out


def stoch_sir_model(N, beta, gamma, S0, I0, R0, t_start, t_end, h, num_simulations: int, seed: int = 0, device: int = STOCH_HOST_TWIN,
                    out_dir=None, run: bool = True) -> dict:
    """HipStochasticSIRModel end to end (constructor, runSimulations, writeCsv(out_dir), getStatistics, getResults).
    std::invalid_argument becomes ValueError, anything else RuntimeError; run=False stops after the constructor."""
    lib = load_library()
    err = C.create_string_buffer(512)
    steps = C.c_int(0)
    args = [float(N), float(beta), float(gamma), float(S0), float(I0), float(R0), float(t_start), float(t_end), float(h),
            int(num_simulations), int(seed) & 0xFFFFFFFFFFFFFFFF, int(device)]
    rc = lib.host_stoch_sir_model(*args, None, None, None, C.byref(steps), err, len(err))
    if rc == 0 and run:
        keep = min(int(num_simulations), 100)
        stats = np.empty((4, 3, steps.value))
        results = np.empty((keep, 3, steps.value))
        rc = lib.host_stoch_sir_model(*args, None if out_dir is None else os.fsencode(out_dir), stats.ctypes.data, results.ctypes.data,
                                      C.byref(steps), err, len(err))
    if rc == 1:
        raise ValueError(err.value.decode())
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return {"steps": steps.value, "stats": stats, "results": results} if run else {"steps": steps.value}


# ---- posterior predictive draws with Poisson noise: the CPU twin of sepaihrd_ensemble_predictive and its sampler ----
def poisson_probe(lam, seed: int) -> np.ndarray:
    """the twin of HipObjective.poisson: out[i] ~ Poisson(lam[i]) at (seed, c0 = i, c1 = c2 = 0)"""
    lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
    out = np.empty(lam.size)
    load_library().host_poisson_probe(int(seed) & 0xFFFFFFFFFFFFFFFF, lam.ctypes.data, lam.size, out.ctypes.data)
    return out


def poisson_at(seed: int, c0: int, c1: int, c2: int, lam: float) -> float:
    """the Poisson(lam) variate at these coordinates of the stream"""
    return float(load_library().host_poisson_at(int(seed) & 0xFFFFFFFFFFFFFFFF, int(c0), int(c1), int(c2), float(lam)))


def predictive_validate(S: int, R: int, T_pos: int, n_age: int, probs) -> None:
    """sepaihrd_predictive_validate (host only): ValueError with its message for arguments the predictive call refuses"""
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    err = C.create_string_buffer(512)
    if hipabi.load_library().sepaihrd_predictive_validate(int(S), int(R), int(T_pos), int(n_age), pr.ctypes.data, pr.size, err, len(err)) != 0:
        raise ValueError(err.value.decode())


def observed_table(pb) -> np.ndarray:
    """the problem's observations as the predictive call places them: [3: H, ICU, D][T_pos][n], NaN beyond the data's rows"""
    Tp = int(np.sum(np.asarray(pb.times) >= 0.0))
    out = np.full((3, Tp, pb.n), np.nan)
    for k, name in enumerate(("obs_H", "obs_ICU", "obs_D")):
        rows = np.asarray(getattr(pb, name), dtype=np.float64).reshape(-1, pb.n)[:Tp]
        out[k, :rows.shape[0]] = rows
    return out


def gamma_at(seed: int, c0: int, c1: int, c2: int, shape: float) -> float:
    """the Gamma(shape, 1) variate at these coordinates of the stream (csrc/sepaihrd_nb_draw.inc)"""
    return float(load_library().host_gamma_at(int(seed) & 0xFFFFFFFFFFFFFFFF, int(c0), int(c1), int(c2), float(shape)))


def nb_draw_at(seed: int, c0: int, c1: int, c2: int, mu: float, k: float) -> float:
    """the negative-binomial variate (mean mu, dispersion k; k = +inf: Poisson) at these coordinates of the stream"""
    return float(load_library().host_nb_draw_at(int(seed) & 0xFFFFFFFFFFFFFFFF, int(c0), int(c1), int(c2), float(mu), float(k)))


def gamma_probe(shape, seed: int) -> np.ndarray:
    """the twin of HipObjective.gamma_device: out[i] ~ Gamma(shape[i], 1) at (seed, c0 = i, c1 = c2 = 0)"""
    shape = np.ascontiguousarray(shape, dtype=np.float64).ravel()
    out = np.empty(shape.size)
    load_library().host_gamma_probe(int(seed) & 0xFFFFFFFFFFFFFFFF, shape.ctypes.data, shape.size, out.ctypes.data)
    return out


def nb_draw_probe(mu, k, seed: int) -> np.ndarray:
    """the twin of HipObjective.nb_draw_device: out[i] ~ NB(mu[i], k[i]) at (seed, c0 = i, c1 = c2 = 0)"""
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.float64), mu.shape), dtype=np.float64).ravel()
    out = np.empty(mu.size)
    load_library().host_nb_draw_probe(int(seed) & 0xFFFFFFFFFFFFFFFF, mu.ctypes.data, k.ctypes.data, mu.size, out.ctypes.data)
    return out


def predictive_from_means(means, status, observed, R: int, seed: int, probs, want_pit: bool = True, want_draws: bool = True,
                          k_used=None) -> dict:
    """The twin of HipObjective.ensemble_predictive after the integration: from means [S][3][T_pos][n] and status [S] (and
    observed [3][T_pos][n], NaN where there is none) the same pred [6][n_probs][T_pos][n], pit [3][T_pos][n] and draws
    [S][R][3][T_pos][n], bit for bit.  k_used [S][3] (None: Poisson draws): the twin of the dispersed call, negative-binomial
    draws with every sample's own dispersions as that call returns them."""
    m = np.ascontiguousarray(means, dtype=np.float64)
    if m.ndim != 4 or m.shape[1] != 3:
        raise ValueError("means must be [S][3][T_pos][n]")
    S, _, Tp, n = m.shape
    st = np.ascontiguousarray(status, dtype=np.int32)
    if st.shape != (S,):
        raise ValueError("status must have one entry per sample")
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    predictive_validate(S, R, Tp, n, pr)
    R = int(R)
    ob = None if observed is None else np.ascontiguousarray(observed, dtype=np.float64)
    if ob is not None and ob.shape != (3, Tp, n):
        raise ValueError("observed must be [3][T_pos][n]")
    pred = np.empty((6, pr.size, Tp, n))
    pit = np.empty((3, Tp, n)) if want_pit and ob is not None else None
    draws = np.empty((S, R, 3, Tp, n)) if want_draws else None
    err = C.create_string_buffer(512)
    tail = (None if ob is None else ob.ctypes.data, S, R, Tp, n, int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, pr.size, pred.ctypes.data,
            None if pit is None else pit.ctypes.data, None if draws is None else draws.ctypes.data, err, len(err))
    if k_used is None:
        rc = load_library().host_predictive_from_means(m.ctypes.data, st.ctypes.data, *tail)
    else:
        ku = np.ascontiguousarray(k_used, dtype=np.float64)
        if ku.shape != (S, 3):
            raise ValueError("k_used must be [S][3]")
        rc = load_library().host_predictive_nb_from_means(m.ctypes.data, st.ctypes.data, ku.ctypes.data, *tail)
    if rc != 0:
        raise ValueError(err.value.decode())
    out = {"pred": pred, "n_valid": int(np.sum(st == 0))}
    if pit is not None:
        out["pit"] = pit
    if draws is not None:
        out["draws"] = draws
    return out


# ---- scores of the posterior predictive draws: the CPU twin of sepaihrd_ensemble_predictive_scores ----
def predictive_scores_validate(S: int, R: int, T_pos: int, n_age: int, probs, levels) -> None:
    """sepaihrd_predictive_scores_validate (host only): ValueError with its message for arguments the scored call refuses"""
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    err = C.create_string_buffer(512)
    if hipabi.load_library().sepaihrd_predictive_scores_validate(int(S), int(R), int(T_pos), int(n_age), pr.ctypes.data, pr.size, lv.ctypes.data,
                                                                 lv.size, err, len(err)) != 0:
        raise ValueError(err.value.decode())


def predictive_scores_from_means(means, status, observed, R: int, seed: int, probs, levels, k_used=None, want_draws: bool = True) -> dict:
    """The twin of HipObjective.ensemble_predictive_scores after the integration: from means [S][3][T_pos][n], status [S], k_used
    [S][3] (None: Poisson draws) and observed [3][T_pos][n] the same draws, pred, pit, cell_scores, summary and exact -- std::sort
    and the text the kernels compile (csrc/sepaihrd_predictive_score.inc): bit for bit where exact is True.  The result carries
    the named views of hipabi.score_views too."""
    m = np.ascontiguousarray(means, dtype=np.float64)
    if m.ndim != 4 or m.shape[1] != 3:
        raise ValueError("means must be [S][3][T_pos][n]")
    S, _, Tp, n = m.shape
    st = np.ascontiguousarray(status, dtype=np.int32)
    if st.shape != (S,):
        raise ValueError("status must have one entry per sample")
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    predictive_scores_validate(S, R, Tp, n, pr, lv)
    R, L = int(R), lv.size
    if observed is None:
        raise ValueError("observed must be [3][T_pos][n]")
    ob = np.ascontiguousarray(observed, dtype=np.float64)
    if ob.shape != (3, Tp, n):
        raise ValueError("observed must be [3][T_pos][n]: (3, %d, %d), not %s" % (Tp, n, ob.shape))
    ku = None
    if k_used is not None:
        ku = np.ascontiguousarray(k_used, dtype=np.float64)
        if ku.shape != (S, 3):
            raise ValueError("k_used must be [S][3]")
    pred, pit = np.empty((6, pr.size, Tp, n)), np.empty((3, Tp, n))
    cell_scores, summary = np.empty((3, Tp, n, 5 + 4 * L)), np.empty((3, n + 1, 4 + 2 * L))
    draws = np.empty((S, R, 3, Tp, n)) if want_draws else None
    exact = C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = load_library().host_predictive_scores_from_means(
        m.ctypes.data, st.ctypes.data, None if ku is None else ku.ctypes.data, ob.ctypes.data, S, R, Tp, n, int(seed) & 0xFFFFFFFFFFFFFFFF,
        pr.ctypes.data, pr.size, lv.ctypes.data, L, pred.ctypes.data, pit.ctypes.data, cell_scores.ctypes.data, summary.ctypes.data,
        None if draws is None else draws.ctypes.data, C.byref(exact), err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())
    out = {"pred": pred, "pit": pit, "cell_scores": cell_scores, "summary": summary, "exact": bool(exact.value),
           "n_valid": int(np.sum(st == 0)), "levels": lv, "observed": ob}
    if draws is not None:
        out["draws"] = draws
    out.update(hipabi.score_views(cell_scores, summary, ob, lv))
    return out


def predictive_targets_validate(S: int, R: int, T_pos: int, n_age: int, age_group, window: int, origin: int, probs, levels) -> tuple:
    """sepaihrd_predictive_targets_validate (host only): (W, G), or ValueError with its message for arguments the call refuses"""
    return hipabi.predictive_targets_validate(S, R, T_pos, n_age, age_group, window, origin, probs, levels)


def predictive_targets_from_means(means, status, observed, R: int, seed: int, probs, levels, age_group, window: int, origin: int = 0,
                                  k_used=None, want_draws: bool = True, want_target_draws: bool = True) -> dict:
    """The twin of HipObjective.ensemble_predictive_targets after the integration: from means [S][3][T_pos][n], status [S], k_used
    [S][3] (None: Poisson draws) and observed [3][T_pos][n] the same daily draws summed into the targets of
    csrc/sepaihrd_predictive_targets.inc, then std::sort and the score text: target_quantiles, pit, target_obs, target_scores,
    summary, exact, W, G, window_first_row, draws and target_draws on request, and the named views of hipabi.target_views.  Bit for
    bit where exact is True."""
    m = np.ascontiguousarray(means, dtype=np.float64)
    if m.ndim != 4 or m.shape[1] != 3:
        raise ValueError("means must be [S][3][T_pos][n]")
    S, _, Tp, n = m.shape
    st = np.ascontiguousarray(status, dtype=np.int32)
    if st.shape != (S,):
        raise ValueError("status must have one entry per sample")
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    ag = np.ascontiguousarray(age_group, dtype=np.int32).ravel()
    W, G = hipabi.predictive_targets_validate(S, R, Tp, n, ag, window, origin, pr, lv)
    R, L = int(R), lv.size
    if observed is None:
        raise ValueError("observed must be [3][T_pos][n]")
    ob = np.ascontiguousarray(observed, dtype=np.float64)
    if ob.shape != (3, Tp, n):
        raise ValueError("observed must be [3][T_pos][n]: (3, %d, %d), not %s" % (Tp, n, ob.shape))
    ku = None
    if k_used is not None:
        ku = np.ascontiguousarray(k_used, dtype=np.float64)
        if ku.shape != (S, 3):
            raise ValueError("k_used must be [S][3]")
    tq, pit, tobs = np.empty((6, pr.size, W, G)), np.empty((6, W, G)), np.empty((6, W, G))
    tscores, summary = np.empty((6, W, G, 5 + 4 * L)), np.empty((6, G + 1, 4 + 2 * L))
    draws = np.empty((S, R, 3, Tp, n)) if want_draws else None
    tdraws = np.empty((S, R, 3, W, G)) if want_target_draws else None
    exact = C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = load_library().host_predictive_targets_from_means(
        m.ctypes.data, st.ctypes.data, None if ku is None else ku.ctypes.data, ob.ctypes.data, S, R, Tp, n, int(seed) & 0xFFFFFFFFFFFFFFFF,
        ag.ctypes.data, int(window), int(origin), pr.ctypes.data, pr.size, lv.ctypes.data, L, tq.ctypes.data, pit.ctypes.data,
        tscores.ctypes.data, summary.ctypes.data, tobs.ctypes.data, None if tdraws is None else tdraws.ctypes.data,
        None if draws is None else draws.ctypes.data, C.byref(exact), err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())
    out = {"target_quantiles": tq, "pit": pit, "target_obs": tobs, "target_scores": tscores, "summary": summary,
           "exact": bool(exact.value), "W": W, "G": G, "window_first_row": int(origin) + int(window) * np.arange(W),
           "n_valid": int(np.sum(st == 0)), "levels": lv, "age_group": ag}
    if draws is not None:
        out["draws"] = draws
    if tdraws is not None:
        out["target_draws"] = tdraws
    out.update(hipabi.target_views(tscores, summary, tobs, lv))
    return out


def score_cell(x, y: float, levels) -> dict:
    """One unsorted sample x against one observation y by the cell rule of csrc/sepaihrd_predictive_score.inc: scores [5 + 4 L]
    (mean, variance, median, crps, wis, then lower, upper, interval_score, covered per level) with their named entries, pit and
    exact (every sum stayed below 2^53)."""
    xs = np.ascontiguousarray(x, dtype=np.float64).ravel()
    lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    scores = np.empty(5 + 4 * lv.size)
    pit, exact = C.c_double(0.0), C.c_int32(0)
    err = C.create_string_buffer(512)
    if load_library().host_score_cell(xs.ctypes.data, xs.size, float(y), lv.ctypes.data, lv.size, scores.ctypes.data, C.byref(pit),
                                      C.byref(exact), err, len(err)) != 0:
        raise ValueError(err.value.decode())
    out = {"scores": scores, "pit": pit.value, "exact": bool(exact.value)}
    out.update({name: scores[f] for f, name in enumerate(("mean", "variance", "median", "crps", "wis"))})
    out.update({name: scores[5 + f::4] for f, name in enumerate(("lower", "upper", "interval_score", "covered"))})
    return out


# ---- stochastic chain-binomial SEPAIHRD ensembles: the CPU twin of sepaihrd_ensemble_stochastic ----
STOCH_COMPARTMENTS = ("S", "E", "P", "A", "I", "H", "ICU", "R", "D", "CumH", "CumICU")
STOCH_SCALARS = ("theta", "sigma", "gamma_p", "gamma_A", "gamma_I", "gamma_H", "gamma_ICU", "beta")
STOCH_VECTORS = ("a", "h_infec", "p", "h", "icu", "d_H", "d_ICU", "d_community")


def stochastic_values_width(n_age: int, n_beta: int, n_kappa: int) -> int:
    """sepaihrd_stochastic_values_width: the width W of a model_values row"""
    return int(hipabi.load_library().sepaihrd_stochastic_values_width(int(n_age), int(n_beta), int(n_kappa)))


def stochastic_pack_values(n_age: int, initial, beta_values=(), kappa_values=(1.0,), **fields) -> np.ndarray:
    """One model_values row in the layout include/sepaihrd_hip.h documents: the scalars of STOCH_SCALARS and the per-age vectors of
    STOCH_VECTORS by keyword (default 0), the schedule values, and initial [11][n_age] counts."""
    n = int(n_age)
    unknown = set(fields) - set(STOCH_SCALARS) - set(STOCH_VECTORS)
    if unknown:
        raise ValueError(f"unknown fields {sorted(unknown)}")
    row = [float(fields.get(k, 0.0)) for k in STOCH_SCALARS]
    row += [float(v) for v in beta_values] + [float(v) for v in kappa_values]
    for k in STOCH_VECTORS:
        row += list(np.broadcast_to(np.asarray(fields.get(k, 0.0), dtype=np.float64), (n,)))
    row += list(np.asarray(initial, dtype=np.float64).reshape(11, n).ravel())
    out = np.asarray(row, dtype=np.float64)
    assert out.size == stochastic_values_width(n, len(beta_values), len(kappa_values))
    return out


def stochastic_validate(S: int, R: int, steps_per_interval: int, keep: int, n_times: int, T_pos: int, n_age: int, probs) -> None:
    """sepaihrd_stochastic_validate (host only): ValueError with its message for arguments the stochastic call refuses"""
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    err = C.create_string_buffer(512)
    if hipabi.load_library().sepaihrd_stochastic_validate(int(S), int(R), int(steps_per_interval), int(keep), int(n_times), int(T_pos),
                                                          int(n_age), pr.ctypes.data, pr.size, err, len(err)) != 0:
        raise ValueError(err.value.decode())


def stochastic_from_values(model_values, status, times, N, M, kappa_end_times, R: int, steps_per_interval: int, seed: int, probs,
                           beta_end_times=(), keep: int = 0, want_final: bool = True) -> dict:
    """The twin of HipObjective.ensemble_stochastic after the decoding: from model_values [S][W] and status [S] and the problem's
    fixed data (times, N [n], M [n][n] with M[i, j] = M(i, j), the schedule end times) the same quantiles [6][n_probs][T_pos][n],
    extinct [S], traj [S][keep][T][11][n] and final_state [S][R][11][n], bit for bit."""
    mv = np.ascontiguousarray(np.atleast_2d(model_values), dtype=np.float64)
    st = np.ascontiguousarray(status, dtype=np.int32).ravel()
    tm = np.ascontiguousarray(times, dtype=np.float64).ravel()
    Nv = np.ascontiguousarray(N, dtype=np.float64).ravel()
    n = Nv.size
    Mm = np.ascontiguousarray(M, dtype=np.float64)
    be = np.ascontiguousarray(beta_end_times, dtype=np.float64).ravel()
    ke = np.ascontiguousarray(kappa_end_times, dtype=np.float64).ravel()
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    S, T, R, keep = mv.shape[0], tm.size, int(R), int(keep)
    Tp = int(np.sum(tm >= 0.0))
    if Mm.shape != (n, n) or st.shape != (S,) or mv.shape[1] != stochastic_values_width(n, be.size, ke.size):
        raise ValueError("model_values [S][W], status [S], N [n], M [n][n]")
    stochastic_validate(S, R, steps_per_interval, keep, T, Tp, n, pr)
    q, extinct = np.empty((6, pr.size, Tp, n)), np.empty(S)
    traj = np.empty((S, keep, T, 11, n)) if keep > 0 else None
    final = np.empty((S, R, 11, n)) if want_final else None
    err = C.create_string_buffer(512)
    rc = load_library().host_stochastic_from_values(n, T, be.size, ke.size, tm.ctypes.data, Nv.ctypes.data, Mm.ctypes.data,
                                                    be.ctypes.data if be.size else None, ke.ctypes.data, mv.ctypes.data, st.ctypes.data, S, R,
                                                    int(steps_per_interval), int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, pr.size, keep,
                                                    q.ctypes.data, extinct.ctypes.data, None if traj is None else traj.ctypes.data,
                                                    None if final is None else final.ctypes.data, err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())
    out = {"quantiles": q, "extinct": extinct, "n_valid": int(np.sum(st == 0))}
    if traj is not None:
        out["traj"] = traj
    if final is not None:
        out["final_state"] = final
    return out


# ---- bootstrap particle filter of the stochastic SEPAIHRD model: the CPU twin of sepaihrd_particle_loglik ----
def particle_max_particles(n_age: int) -> int:
    """sepaihrd_particle_max_particles (host only): the largest J the filter takes for n_age classes; -1 outside 1..16"""
    return int(hipabi.load_library().sepaihrd_particle_max_particles(int(n_age)))


def particle_validate(B: int, J: int, steps_per_interval: int, n_times: int, T_pos: int, n_age: int) -> None:
    """sepaihrd_particle_validate (host only): ValueError with its message for arguments the filter refuses"""
    err = C.create_string_buffer(512)
    if hipabi.load_library().sepaihrd_particle_validate(int(B), int(J), int(steps_per_interval), int(n_times), int(T_pos), int(n_age), err,
                                                        len(err)) != 0:
        raise ValueError(err.value.decode())


def particle_resample(logw, seed: int, b: int = 0, row: int = 0) -> dict:
    """The twin of HipObjective.particle_resample_device: ancestors [J], increment and ess of one weighted row with log-weights logw"""
    lw = np.ascontiguousarray(logw, dtype=np.float64).ravel()
    if lw.size < 1:
        raise ValueError("logw must hold at least one log-weight")
    anc = np.empty(lw.size, dtype=np.int32)
    inc, ess = C.c_double(0.0), C.c_double(0.0)
    load_library().host_particle_resample(int(seed) & 0xFFFFFFFFFFFFFFFF, int(b), int(row), lw.ctypes.data, lw.size, anc.ctypes.data,
                                          C.byref(inc), C.byref(ess))
    return {"ancestors": anc, "increment": inc.value, "ess": ess.value}


def particle_wide_max_particles() -> int:
    """sepaihrd_particle_wide_max_particles (host only): the largest J the wide form of the filter takes, 65 536"""
    return int(hipabi.load_library().sepaihrd_particle_wide_max_particles())


def particle_wide_validate(B: int, J: int, steps_per_interval: int, theta_chunk: int, n_times: int, T_pos: int, n_age: int) -> None:
    """sepaihrd_particle_wide_validate (host only): ValueError with its message for arguments the wide form refuses"""
    err = C.create_string_buffer(512)
    if hipabi.load_library().sepaihrd_particle_wide_validate(int(B), int(J), int(steps_per_interval), int(theta_chunk), int(n_times), int(T_pos),
                                                             int(n_age), err, len(err)) != 0:
        raise ValueError(err.value.decode())


def _dispersion(dispersion) -> np.ndarray:
    """(k_H, k_ICU, k_D) as three contiguous doubles"""
    disp = np.ascontiguousarray(dispersion, dtype=np.float64).ravel()
    if disp.size != 3:
        raise ValueError("dispersion must hold three entries: k_H, k_ICU, k_D")
    return disp


def particle_nb_validate(dispersion) -> None:
    """sepaihrd_particle_nb_validate (host only): ValueError with its message for a dispersion the filters refuse (None: NULL)"""
    err = C.create_string_buffer(512)
    disp = None if dispersion is None else _dispersion(dispersion)
    if hipabi.load_library().sepaihrd_particle_nb_validate(None if disp is None else disp.ctypes.data, err, len(err)) != 0:
        raise ValueError(err.value.decode())


def lgamma_pos(x) -> np.ndarray:
    """lgamma_pos of csrc/sepaihrd_lgamma.inc as this library compiles it, element by element (the twin of HipObjective.lgamma_device)"""
    fn = load_library().host_lgamma_pos
    xs = np.ascontiguousarray(x, dtype=np.float64)
    return np.array([fn(float(v)) for v in xs.ravel()]).reshape(xs.shape)


def nb_objective(increments, obs_H, obs_ICU, obs_D, k, lib: str = "host") -> dict:
    """The twin of the negative-binomial likelihood pass of the deterministic objective: increments
    [B][T][3][n] (series H, ICU, D: the daily differences of CumH, CumICU and D, not yet clamped at 0), observations obs_* [T][n]
    (NaN where there is none), k [B][3] (+inf: that series is Poisson) -> loglik [B], ll_parts [B][3], status [B].
    lib = "host": this library's compile (host_nb_objective); "hip": libsepaihrd_hip.so's (sepaihrd_nb_objective_host)."""
    inc = np.ascontiguousarray(increments, dtype=np.float64)
    if inc.ndim != 4 or inc.shape[2] != 3:
        raise ValueError("increments must be [B][T][3][n]")
    B, T, _, n = inc.shape
    ob = [np.ascontiguousarray(o, dtype=np.float64) for o in (obs_H, obs_ICU, obs_D)]
    if any(o.shape != (T, n) for o in ob):
        raise ValueError(f"obs_H, obs_ICU and obs_D must be [{T}][{n}]")
    kk = np.ascontiguousarray(k, dtype=np.float64)
    if kk.shape != (B, 3):
        raise ValueError(f"k must be [{B}][3]")
    out = {"loglik": np.empty(B), "ll_parts": np.empty((B, 3)), "status": np.empty(B, dtype=np.int32)}
    fn = load_library().host_nb_objective if lib == "host" else hipabi.load_library().sepaihrd_nb_objective_host
    rc = fn(inc.ctypes.data, ob[0].ctypes.data, ob[1].ctypes.data, ob[2].ctypes.data, kk.ctypes.data, B, T, n, out["loglik"].ctypes.data,
            out["ll_parts"].ctypes.data, out["status"].ctypes.data)
    if rc != 0:
        raise ValueError(f"nb_objective refused its arguments ({rc})")
    return out


def particle_nb_term(obs, inc, k: float) -> np.ndarray:
    """The twin of HipObjective.particle_nb_term_device: the negative-binomial term of csrc/sepaihrd_particle.inc for the observations
    obs, the increments inc (int32) and the dispersion k, cell by cell"""
    ob = np.ascontiguousarray(obs, dtype=np.float64).ravel()
    ic = np.ascontiguousarray(inc, dtype=np.int32).ravel()
    if ob.size != ic.size:
        raise ValueError("obs and inc must have the same number of cells")
    out = np.empty(ob.size)
    load_library().host_particle_nb_term(ob.ctypes.data, ic.ctypes.data, ob.size, float(k), out.ctypes.data)
    return out


def particle_nb_row_constants(obs_H, obs_ICU, obs_D, n_age: int, T_pos: int, dispersion) -> np.ndarray:
    """The twin of sepaihrd_particle_nb_row_constants: G [T_pos], the row constants of the observations obs_* [n_obs][n_age] under
    the dispersion (k_H, k_ICU, k_D); output rows beyond n_obs have no observation"""
    n = int(n_age)
    ob = [np.ascontiguousarray(np.asarray(o, dtype=np.float64).reshape(-1, n)) for o in (obs_H, obs_ICU, obs_D)]
    if not (ob[0].shape == ob[1].shape == ob[2].shape):
        raise ValueError("obs_H, obs_ICU and obs_D must have the same shape [n_obs][n]")
    disp = _dispersion(dispersion)
    G = np.empty(int(T_pos))
    err = C.create_string_buffer(512)
    if load_library().host_particle_nb_row_constants(n, int(T_pos), ob[0].shape[0], ob[0].ctypes.data, ob[1].ctypes.data, ob[2].ctypes.data,
                                                     disp.ctypes.data, G.ctypes.data, err, len(err)) != 0:
        raise ValueError(err.value.decode())
    return G


def particle_from_values(model_values, status, times, N, M, kappa_end_times, obs_H, obs_ICU, obs_D, J: int, steps_per_interval: int, seed: int,
                         beta_end_times=(), want_final: bool = True, dispersion=None) -> dict:
    """The twin of HipObjective.particle_loglik after the decoding: from model_values [B][W] and status [B], the problem's fixed data
    (times, N [n], M [n][n] with M[i, j] = M(i, j), the schedule end times) and the observations obs_* [n_obs][n] of the output times
    >= 0 the same loglik [B], increments [B][T_pos], ess [B][T_pos] and final_state [B][J][11][n], bit for bit."""
    return _particle_from_values(False, model_values, status, times, N, M, kappa_end_times, obs_H, obs_ICU, obs_D, J, steps_per_interval, seed,
                                 beta_end_times, want_final, dispersion)


def particle_wide_from_values(model_values, status, times, N, M, kappa_end_times, obs_H, obs_ICU, obs_D, J: int, steps_per_interval: int,
                              seed: int, beta_end_times=(), want_final: bool = True, dispersion=None) -> dict:
    """The twin of HipObjective.particle_loglik_wide: particle_from_values' walk behind the wide form's argument rules (J up to 65 536)"""
    return _particle_from_values(True, model_values, status, times, N, M, kappa_end_times, obs_H, obs_ICU, obs_D, J, steps_per_interval, seed,
                                 beta_end_times, want_final, dispersion)


def _particle_from_values(wide, model_values, status, times, N, M, kappa_end_times, obs_H, obs_ICU, obs_D, J, steps_per_interval, seed, beta_end_times,
                          want_final, dispersion=None) -> dict:
    # dispersion = (k_H, k_ICU, k_D): the negative-binomial twins (hostParticleLoglikNB, hostParticleLoglikWideNB); None: the Poisson twins
    mv = np.ascontiguousarray(np.atleast_2d(model_values), dtype=np.float64)
    st = np.ascontiguousarray(status, dtype=np.int32).ravel()
    tm = np.ascontiguousarray(times, dtype=np.float64).ravel()
    Nv = np.ascontiguousarray(N, dtype=np.float64).ravel()
    n = Nv.size
    Mm = np.ascontiguousarray(M, dtype=np.float64)
    be = np.ascontiguousarray(beta_end_times, dtype=np.float64).ravel()
    ke = np.ascontiguousarray(kappa_end_times, dtype=np.float64).ravel()
    ob = [np.ascontiguousarray(np.asarray(o, dtype=np.float64).reshape(-1, n)) for o in (obs_H, obs_ICU, obs_D)]
    B, T, J = mv.shape[0], tm.size, int(J)
    Tp = int(np.sum(tm >= 0.0))
    if Mm.shape != (n, n) or st.shape != (B,) or mv.shape[1] != stochastic_values_width(n, be.size, ke.size):
        raise ValueError("model_values [B][W], status [B], N [n], M [n][n]")
    if not (ob[0].shape == ob[1].shape == ob[2].shape):
        raise ValueError("obs_H, obs_ICU and obs_D must have the same shape [n_obs][n]")
    if wide:
        particle_wide_validate(B, J, steps_per_interval, 0, T, Tp, n)
    else:
        particle_validate(B, J, steps_per_interval, T, Tp, n)
    loglik, inc, ess = np.empty(B), np.empty((B, Tp)), np.empty((B, Tp))
    final = np.empty((B, J, 11, n)) if want_final else None
    err = C.create_string_buffer(512)
    lib = load_library()
    extra = ()
    if dispersion is None:
        call = lib.host_particle_wide_from_values if wide else lib.host_particle_from_values
    else:
        particle_nb_validate(dispersion)
        disp = _dispersion(dispersion)
        extra = (disp.ctypes.data,)
        call = lib.host_particle_wide_nb_from_values if wide else lib.host_particle_nb_from_values
    rc = call(n, T, be.size, ke.size, tm.ctypes.data, Nv.ctypes.data, Mm.ctypes.data, be.ctypes.data if be.size else None, ke.ctypes.data,
              ob[0].shape[0], ob[0].ctypes.data, ob[1].ctypes.data, ob[2].ctypes.data, mv.ctypes.data, st.ctypes.data, B, J, int(steps_per_interval),
              int(seed) & 0xFFFFFFFFFFFFFFFF, *extra, loglik.ctypes.data, inc.ctypes.data, ess.ctypes.data, None if final is None else final.ctypes.data,
              err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())
    out = {"loglik": loglik, "increments": inc, "ess": ess, "n_valid": int(np.sum(st == 0))}
    if final is not None:
        out["final_state"] = final
    return out


def particle_states_validate(B: int, J: int, steps_per_interval: int, theta_chunk: int, n_times: int, T_pos: int, n_age: int, probs=()) -> None:
    """sepaihrd_particle_states_validate (host only): ValueError with its message for arguments particle_filter_states refuses
    (probs None: a NULL pointer with n_probs = 1)"""
    err = C.create_string_buffer(512)
    pr = None if probs is None else np.ascontiguousarray(probs, dtype=np.float64).ravel()
    n_probs = 1 if pr is None else pr.size
    if hipabi.load_library().sepaihrd_particle_states_validate(int(B), int(J), int(steps_per_interval), int(theta_chunk), int(n_times), int(T_pos),
                                                               int(n_age), pr.ctypes.data if n_probs and pr is not None else None, n_probs, err,
                                                               len(err)) != 0:
        raise ValueError(err.value.decode())


def particle_states_from_values(model_values, status, times, N, M, kappa_end_times, obs_H, obs_ICU, obs_D, J: int, steps_per_interval: int,
                                seed: int, probs=(), beta_end_times=(), want_quantiles: bool = True, dispersion=None) -> dict:
    """The twin of HipObjective.particle_filter_states after the decoding: particle_wide_from_values' walk with the per-row summaries
    of csrc/sepaihrd_particle_states.inc.  loglik [B], increments [B][T_pos], ess [B][T_pos] (those of particle_wide_from_values),
    state_mean [B][T][11][n + 1] and, where probs is not empty and want_quantiles, state_quantiles [B][T][11][n + 1][len(probs)],
    bit for bit."""
    mv = np.ascontiguousarray(np.atleast_2d(model_values), dtype=np.float64)
    st = np.ascontiguousarray(status, dtype=np.int32).ravel()
    tm = np.ascontiguousarray(times, dtype=np.float64).ravel()
    Nv = np.ascontiguousarray(N, dtype=np.float64).ravel()
    n = Nv.size
    Mm = np.ascontiguousarray(M, dtype=np.float64)
    be = np.ascontiguousarray(beta_end_times, dtype=np.float64).ravel()
    ke = np.ascontiguousarray(kappa_end_times, dtype=np.float64).ravel()
    ob = [np.ascontiguousarray(np.asarray(o, dtype=np.float64).reshape(-1, n)) for o in (obs_H, obs_ICU, obs_D)]
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    B, T, J = mv.shape[0], tm.size, int(J)
    Tp = int(np.sum(tm >= 0.0))
    if Mm.shape != (n, n) or st.shape != (B,) or mv.shape[1] != stochastic_values_width(n, be.size, ke.size):
        raise ValueError("model_values [B][W], status [B], N [n], M [n][n]")
    if not (ob[0].shape == ob[1].shape == ob[2].shape):
        raise ValueError("obs_H, obs_ICU and obs_D must have the same shape [n_obs][n]")
    particle_states_validate(B, J, steps_per_interval, 0, T, Tp, n, pr)
    disp = None
    if dispersion is not None:
        particle_nb_validate(dispersion)
        disp = _dispersion(dispersion)
    loglik, inc, ess = np.empty(B), np.empty((B, Tp)), np.empty((B, Tp))
    mean = np.empty((B, T, 11, n + 1))
    quant = np.empty((B, T, 11, n + 1, pr.size)) if (want_quantiles and pr.size) else None
    err = C.create_string_buffer(512)
    rc = load_library().host_particle_states_from_values(
        n, T, be.size, ke.size, tm.ctypes.data, Nv.ctypes.data, Mm.ctypes.data, be.ctypes.data if be.size else None, ke.ctypes.data, ob[0].shape[0],
        ob[0].ctypes.data, ob[1].ctypes.data, ob[2].ctypes.data, mv.ctypes.data, st.ctypes.data, B, J, int(steps_per_interval),
        int(seed) & 0xFFFFFFFFFFFFFFFF, None if disp is None else disp.ctypes.data, pr.ctypes.data if pr.size else None, pr.size, loglik.ctypes.data,
        inc.ctypes.data, ess.ctypes.data, mean.ctypes.data, None if quant is None else quant.ctypes.data, err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())
    out = {"loglik": loglik, "increments": inc, "ess": ess, "n_valid": int(np.sum(st == 0)), "state_mean": mean}
    if quant is not None:
        out["state_quantiles"] = quant
    return out
