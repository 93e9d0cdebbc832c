"""ctypes view of the C ABI in include/sepaihrd_hip.h (test / bench plumbing).

The reference-side binding a C++ maintainer would add is the adapter in ``host/``
(see INTEGRATION.md); this module is what tests/ and bench.py use to drive the same
entry points from Python.  No compute happens here and there is no fallback: if
``libsepaihrd_hip.so`` is missing or no HIP device is present the constructors raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .problem import CONSTRAINT_CLAMP, SEPAIHRDProblem, SIRProblem, StochasticSIRProblem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsepaihrd_hip.so")
ABI_VERSION = 3
LOWEST = -np.finfo(np.float64).max

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint8)


class sepaihrd_problem(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_age", C.c_int32), ("n_times", C.c_int32), ("n_obs", C.c_int32),
        ("n_beta", C.c_int32), ("n_kappa", C.c_int32), ("n_params", C.c_int32), ("solver", C.c_int32),
        ("constraint_mode", C.c_int32), ("arith", C.c_int32), ("max_attempts", C.c_int32),
        ("precision", C.c_int32),
        ("times", _dp), ("N", _dp), ("M", _dp),
        ("a", _dp), ("h_infec", _dp), ("p", _dp), ("h", _dp), ("icu", _dp), ("d_H", _dp), ("d_ICU", _dp),
        ("d_community", _dp),
        ("beta_end_times", _dp), ("beta_values", _dp), ("kappa_end_times", _dp), ("kappa_values", _dp),
        ("initial_state", _dp), ("obs_H", _dp), ("obs_ICU", _dp), ("obs_D", _dp),
        ("param_field", _ip), ("param_index", _ip), ("lower", _dp), ("upper", _dp), ("has_bounds", _up),
        ("beta", C.c_double), ("theta", C.c_double), ("sigma", C.c_double), ("gamma_p", C.c_double),
        ("gamma_A", C.c_double), ("gamma_I", C.c_double), ("gamma_H", C.c_double), ("gamma_ICU", C.c_double),
        ("multipliers", C.c_double * 8), ("runup_days", C.c_double), ("seed_exposed", C.c_double),
        ("abs_err", C.c_double), ("rel_err", C.c_double), ("dt_hint", C.c_double),
    ]


class sepaihrd_kernel_info(C.Structure):
    _fields_ = [
        ("lanes_per_chain", C.c_int32), ("chains_per_wave", C.c_int32), ("block_threads", C.c_int32),
        ("vgprs", C.c_int32), ("sgprs", C.c_int32), ("lds_bytes", C.c_int32), ("scratch_bytes", C.c_int32),
        ("max_blocks_per_cu", C.c_int32), ("num_cus", C.c_int32), ("likelihood_form", C.c_int32),
        ("phase_pass_applied", C.c_int32),
        ("kernel_name", C.c_char * 128), ("device_name", C.c_char * 128),
    ]


class sepaihrd_sir_problem(C.Structure):
    """include/sepaihrd_hip.h: struct sepaihrd_sir_problem"""
    _fields_ = [
        ("abi_version", C.c_int32), ("n_age", C.c_int32), ("n_times", C.c_int32), ("n_params", C.c_int32),
        ("solver", C.c_int32), ("arith", C.c_int32), ("max_attempts", C.c_int32), ("reserved", C.c_int32),
        ("times", _dp), ("N", _dp), ("C", _dp), ("gamma", _dp), ("initial_state", _dp), ("obs", _dp),
        ("param_field", _ip), ("param_index", _ip),
        ("q", C.c_double), ("scale_C_total", C.c_double),
        ("abs_err", C.c_double), ("rel_err", C.c_double), ("dt_hint", C.c_double),
    ]


class sepaihrd_stoch_sir_config(C.Structure):
    """include/sepaihrd_hip.h: struct sepaihrd_stoch_sir_config"""
    _fields_ = [("abi_version", C.c_int32), ("n_groups", C.c_int32), ("n_replicates", C.c_int32), ("keep", C.c_int32),
                ("t_start", C.c_double), ("t_end", C.c_double), ("h", C.c_double), ("seed", C.c_uint64),
                ("max_workspace_bytes", C.c_uint64)]


STOCH_SIR_STATS = ("mean", "median", "p05", "p95")  # the second axis of `stats`
STOCH_SIR_DEFAULT_WORKSPACE = 4 << 30                # SEPAIHRD_STOCH_SIR_DEFAULT_WORKSPACE


# every symbol include/sepaihrd_hip.h declares
class sepaihrd_mh_config(C.Structure):
    """include/sepaihrd_hip.h: struct sepaihrd_mh_config"""
    _fields_ = [("chains", C.c_int32), ("iterations", C.c_int32), ("thinning", C.c_int32),
                ("adaptation_window", C.c_int32), ("covariance_mode", C.c_int32), ("reserved", C.c_int32),
                ("reg_eps", C.c_double), ("scaling_factor", C.c_double)]


MH_COV_RUNNING, MH_COV_TWO_PASS = 0, 1
FORM_AUTO, FORM_LANE_PER_AGE, FORM_QUAD = 0, 1, 2
LL_INLINE, LL_SEPARATE_PASS, LL_CONSUMER_WAVES = 0, 1, 2
GATHER_AUTO, GATHER_RCCL, GATHER_HOST = 0, 1, 2


def mh_create(lib, ctx, chains: int, iterations: int, x0: np.ndarray, cov0: np.ndarray, reg_eps: float = 1e-6,
              scaling_factor: Optional[float] = None, thinning: int = 1, adaptation_window: int = 0,
              covariance_mode: int = MH_COV_RUNNING):
    """sepaihrd_mh_create with its config struct filled; returns the opaque sampler handle (None on failure)."""
    P = x0.shape[-1]
    cfg = sepaihrd_mh_config(chains, iterations, thinning, adaptation_window, covariance_mode, 0, reg_eps,
                             scaling_factor if scaling_factor is not None else 2.38 * 2.38 / P)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    cov0 = np.ascontiguousarray(cov0, dtype=np.float64)
    return lib.sepaihrd_mh_create(ctx, C.byref(cfg), x0.ctypes.data, cov0.ctypes.data)


MH_FORM_AUTO, MH_FORM_BLOCK_PER_CHAIN, MH_FORM_PACKED = 0, 1, 2  # sepaihrd_mh_set_kernel_form


def sir_mh_create(lib, sir_ctx, chains: int, iterations: int, x0: np.ndarray, cov0: np.ndarray, reg_eps: float = 1e-6,
                  scaling_factor: Optional[float] = None, thinning: int = 1, adaptation_window: int = 0,
                  covariance_mode: int = MH_COV_RUNNING):
    """sepaihrd_sir_mh_create: mh_create on the context of a HipSIRObjective (``sir_ctx``).  The handle is the same opaque
    sampler: every sepaihrd_mh_* entry point and mh_diagnostics take it; its errors are read with sepaihrd_sir_last_error."""
    P = x0.shape[-1]
    cfg = sepaihrd_mh_config(chains, iterations, thinning, adaptation_window, covariance_mode, 0, reg_eps,
                             scaling_factor if scaling_factor is not None else 2.38 * 2.38 / P)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    cov0 = np.ascontiguousarray(cov0, dtype=np.float64)
    return lib.sepaihrd_sir_mh_create(sir_ctx, C.byref(cfg), x0.ctypes.data, cov0.ctypes.data)


def mh_set_kernel_form(lib, mh, form: int) -> int:
    """sepaihrd_mh_set_kernel_form (MH_FORM_*); returns the code (0 ok, -1 unknown form / no sampler, -4 packed with P > 64)."""
    return int(lib.sepaihrd_mh_set_kernel_form(mh, int(form)))


def sir_constraint_bounds(lib, param_field) -> tuple:
    """(lower, upper, has_bounds) of the clamp a SIR-backed sampler applies to its proposals, for field codes SEPAIHRD_SIR_F_*."""
    f = np.ascontiguousarray(param_field, dtype=np.int32)
    lo, hi, has = np.empty(f.size), np.empty(f.size), np.empty(f.size, dtype=np.int32)
    rc = lib.sepaihrd_sir_constraint_bounds(f.ctypes.data, f.size, lo.ctypes.data, hi.ctypes.data, has.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"sepaihrd_sir_constraint_bounds failed ({rc})")
    return lo, hi, has


SIR_MAX_EVENTS = 8        # SEPAIHRD_SIR_MAX_EVENTS
SIR_EV_CONTACT = 0        # scale_C_total <- scale_C_total * value
SIR_EV_TRANSMISSION = 1   # q <- q * (1 - value)
SIR_EVENT_KINDS = {"contact": SIR_EV_CONTACT, "transmission": SIR_EV_TRANSMISSION}
SIR_SERIES = ("incidence", "prevalence", "cumulative_infections")


class sepaihrd_sir_event(C.Structure):
    """include/sepaihrd_hip.h: struct sepaihrd_sir_event"""
    _fields_ = [("time_index", C.c_int32), ("kind", C.c_int32), ("value", C.c_double)]


def sir_metric_names(n_age: int) -> list:
    """Columns of the metric table of sepaihrd_sir_scenario_ensemble, in order."""
    names = ["R0", "peak_prevalence", "time_to_peak_prevalence", "peak_incidence", "time_to_peak_incidence", "overall_attack_rate"]
    for i in range(n_age):
        names += [f"attack_rate_age_{i}", f"peak_prevalence_age_{i}"]
    return names


def sir_event_table(scenarios) -> tuple:
    """Scenarios -- each a list of (time_index, kind, value), kind a SIR_EV_* code or "contact" / "transmission" -- as the
    [K][8] table and the [K] counts the C ABI takes.  Lists longer than 8 keep their count, for the validator to refuse."""
    K = len(scenarios)
    tab = (sepaihrd_sir_event * (max(K, 1) * SIR_MAX_EVENTS))()
    counts = np.zeros(max(K, 1), dtype=np.int32)
    for k, sc in enumerate(scenarios):
        counts[k] = len(sc)
        for e, (ti, kind, value) in enumerate(list(sc)[:SIR_MAX_EVENTS]):
            ev = tab[k * SIR_MAX_EVENTS + e]
            ev.time_index, ev.kind, ev.value = int(ti), int(SIR_EVENT_KINDS.get(kind, kind)), float(value)
    return tab, counts


def sir_validate_events(lib, scenarios, n_times: int) -> tuple:
    """sepaihrd_sir_validate_events on the host (no device): (code, message)."""
    tab, counts = sir_event_table(scenarios)
    err = C.create_string_buffer(256)
    rc = lib.sepaihrd_sir_validate_events(tab, counts.ctypes.data, len(scenarios), int(n_times), err, len(err))
    return int(rc), err.value.decode()


DIAG_COLUMNS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "r_hat")  # SEPAIHRD_DIAG_COLUMNS, in order


def _diag_result(out: np.ndarray, lag: np.ndarray) -> dict:
    return {"table": out, "columns": list(DIAG_COLUMNS), "max_lag": lag}


def mh_diagnostics(lib, mh, P: int, chains: int, first_sample: int = 0, count: int = 0, with_values: bool = False) -> dict:
    """sepaihrd_mh_diagnostics over a sampler's resident samples first_sample .. (count <= 0: to the last stored):
    table [P + with_values][7], max_lag [..][4].  Raises RuntimeError (with the code) when the call is refused."""
    rows = P + (1 if with_values else 0)
    out = np.empty((rows, len(DIAG_COLUMNS)))
    lag = np.empty((rows, 4), dtype=np.int32)
    rc = lib.sepaihrd_mh_diagnostics(mh, int(first_sample), int(count), int(bool(with_values)), out.ctypes.data, lag.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"sepaihrd_mh_diagnostics failed ({rc})")
    return _diag_result(out, lag)


EXPORTED_SYMBOLS = (
    "sepaihrd_create", "sepaihrd_destroy", "sepaihrd_last_error", "sepaihrd_abi_version",
    "sepaihrd_set_constraint_mode", "sepaihrd_set_arith", "sepaihrd_set_precision", "sepaihrd_set_integrator_form", "sepaihrd_eval_batch",
    "sepaihrd_eval_batch_device", "sepaihrd_eval_batch_begin", "sepaihrd_eval_batch_end", "sepaihrd_apply_constraints", "sepaihrd_get_kernel_info", "sepaihrd_get_kernel_info_for_batch", "sepaihrd_reserve",
    "sepaihrd_set_timing", "sepaihrd_get_timing", "sepaihrd_set_initial_state_mode", "sepaihrd_fd_gradient_batch",
    "sepaihrd_ensemble_quantiles", "sepaihrd_scenario_ensemble", "sepaihrd_mh_create", "sepaihrd_mh_destroy", "sepaihrd_mh_evaluate_current",
    "sepaihrd_mh_propose", "sepaihrd_mh_fetch", "sepaihrd_mh_stage_normals", "sepaihrd_mh_staging_buffer", "sepaihrd_mh_step", "sepaihrd_mh_read_best", "sepaihrd_mh_busy", "sepaihrd_mh_set_values", "sepaihrd_mh_test_buffer",
    "sepaihrd_mh_step_tested", "sepaihrd_mh_fetch_test", "sepaihrd_mh_commit", "sepaihrd_mh_adapt", "sepaihrd_mh_read_history",
    "sepaihrd_mh_read_covariance", "sepaihrd_mh_read_proposal", "sepaihrd_mh_history_length",
    "sepaihrd_mh_sample_count", "sepaihrd_mh_read_samples", "sepaihrd_mh_read_moments", "sepaihrd_mh_summary_records",
    "sepaihrd_records_buffer", "sepaihrd_allgather_records", "sepaihrd_read_records", "sepaihrd_write_records",
    "sepaihrd_mh_seed_streams", "sepaihrd_mh_draw_first", "sepaihrd_mh_keep_scale_on_device", "sepaihrd_mh_read_run_state",
    "sepaihrd_mh_read_sample_values", "sepaihrd_mh_read_accept_trace",
    "sepaihrd_device_libm_check", "sepaihrd_mh_read_failure_counts", "sepaihrd_mh_snapshot_begin", "sepaihrd_mh_snapshot_end",
    "sepaihrd_device_log_values", "sepaihrd_chain_diagnostics", "sepaihrd_mh_diagnostics",
    "sepaihrd_sir_create", "sepaihrd_sir_destroy", "sepaihrd_sir_last_error", "sepaihrd_sir_eval_batch", "sepaihrd_sir_eval_batch_device",
    "sepaihrd_sir_reserve", "sepaihrd_sir_apply_constraints", "sepaihrd_sir_set_arith",
    "sepaihrd_sir_mh_create", "sepaihrd_sir_device_libm_check", "sepaihrd_sir_constraint_bounds",
    "sepaihrd_mh_set_kernel_form", "sepaihrd_mh_get_kernel_form",
    "sepaihrd_sir_validate_events", "sepaihrd_sir_scenario_ensemble", "sepaihrd_sir_ensemble_quantiles", "sepaihrd_sir_ensemble_timing",
    "sepaihrd_stoch_sir_num_steps", "sepaihrd_stoch_sir_validate", "sepaihrd_stoch_sir_run", "sepaihrd_stoch_sir_binomial_device",
    "sepaihrd_ensemble_predictive", "sepaihrd_predictive_validate", "sepaihrd_predictive_timing", "sepaihrd_poisson_device",
    "sepaihrd_ensemble_predictive_nb", "sepaihrd_gamma_device", "sepaihrd_nb_draw_device",
    "sepaihrd_ensemble_predictive_scores", "sepaihrd_predictive_scores_validate",
    "sepaihrd_ensemble_predictive_targets", "sepaihrd_predictive_targets_validate",
    "sepaihrd_ensemble_stochastic", "sepaihrd_stochastic_validate", "sepaihrd_stochastic_values_width", "sepaihrd_stochastic_timing",
    "sepaihrd_particle_loglik", "sepaihrd_particle_validate", "sepaihrd_particle_max_particles", "sepaihrd_particle_timing",
    "sepaihrd_particle_resample_device",
    "sepaihrd_particle_loglik_wide", "sepaihrd_particle_wide_validate", "sepaihrd_particle_wide_max_particles", "sepaihrd_particle_wide_timing",
    "sepaihrd_particle_wide_resample_device",
    "sepaihrd_particle_loglik_nb", "sepaihrd_particle_loglik_wide_nb", "sepaihrd_particle_nb_validate", "sepaihrd_particle_nb_row_constants",
    "sepaihrd_particle_nb_term_device",
    "sepaihrd_particle_filter_states", "sepaihrd_particle_states_validate", "sepaihrd_particle_states_timing",
    "sepaihrd_set_dispersion", "sepaihrd_get_dispersion", "sepaihrd_dispersion_validate", "sepaihrd_nb_objective_host",
    "sepaihrd_lgamma_host", "sepaihrd_lgamma_device",
)

SCORE_SERIES = ("hospitalizations", "icu_admissions", "deaths")


def score_views(cell_scores, summary, observed, levels) -> dict:
    """Named views of cell_scores [3][T_pos][n][5 + 4 L] and summary [3][n + 1][4 + 2 L] as sepaihrd_ensemble_predictive_scores
    lays them out -- mean, variance, median, crps, wis [3][T_pos][n]; lower, upper, interval_score, covered [L][3][T_pos][n];
    summary_count, summary_crps, summary_wis, summary_abs_err_median [3][n + 1]; summary_coverage, summary_interval_score
    [L][3][n + 1] -- and dawid_sebastiani [3][T_pos][n]: (y - mean)^2 / variance + log(variance) against `observed`, formed here
    from the mean and the variance (it is not part of the ABI), NaN where the variance is 0 or the cell is not usable, with
    summary_dawid_sebastiani [3][n + 1] its mean over the cells where it is finite."""
    cs, sm = np.asarray(cell_scores), np.asarray(summary)
    L = np.asarray(levels).size
    out = {name: cs[..., f] for f, name in enumerate(("mean", "variance", "median", "crps", "wis"))}
    for f, name in enumerate(("lower", "upper", "interval_score", "covered")):
        out[name] = np.moveaxis(cs[..., 5 + f::4], -1, 0) if L else np.empty((0,) + cs.shape[:3])
    for f, name in enumerate(("summary_count", "summary_crps", "summary_wis", "summary_abs_err_median")):
        out[name] = sm[..., f]
    out["summary_coverage"] = np.moveaxis(sm[..., 4::2], -1, 0) if L else np.empty((0,) + sm.shape[:2])
    out["summary_interval_score"] = np.moveaxis(sm[..., 5::2], -1, 0) if L else np.empty((0,) + sm.shape[:2])
    y = np.asarray(observed, dtype=np.float64)
    var = np.where(out["variance"] > 0.0, out["variance"], np.nan)
    usable = np.isfinite(y) & (y >= 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ds = np.where(usable, (y - out["mean"]) ** 2 / var + np.log(var), np.nan)
    out["dawid_sebastiani"] = ds
    pooled = np.empty(sm.shape[:2])
    for k in range(ds.shape[0]):
        for a in range(ds.shape[2] + 1):
            v = ds[k, :, a] if a < ds.shape[2] else ds[k].ravel()
            v = v[np.isfinite(v)]
            pooled[k, a] = v.mean() if v.size else np.nan
    out["summary_dawid_sebastiani"] = pooled
    return out


TARGET_SERIES = SCORE_SERIES + tuple("cumulative_" + name for name in SCORE_SERIES)


def target_views(target_scores, summary, target_obs, levels) -> dict:
    """score_views over the targets of sepaihrd_ensemble_predictive_targets: target_scores [6][W][G][5 + 4 L], summary
    [6][G + 1][4 + 2 L] and target_obs [6][W][G] take the places of cell_scores, summary and observed -- mean, variance, median,
    crps, wis [6][W][G]; lower, upper, interval_score, covered [L][6][W][G]; the summary_* entries [6][G + 1] and [L][6][G + 1];
    series in the order of TARGET_SERIES."""
    return score_views(target_scores, summary, target_obs, levels)


def predictive_targets_validate(S: int, R: int, T_pos: int, n_age: int, age_group, window: int, origin: int, probs, levels) -> tuple:
    """sepaihrd_predictive_targets_validate (host only): (W, G) of the grouping and the windows, or ValueError with its message"""
    ag = np.ascontiguousarray(age_group, dtype=np.int32).ravel()
    pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    if ag.size != int(n_age):
        raise ValueError("age_group must hold n_age = %d entries, not %d" % (int(n_age), ag.size))
    W, G = C.c_int(0), C.c_int(0)
    err = C.create_string_buffer(512)
    if load_library().sepaihrd_predictive_targets_validate(int(S), int(R), int(T_pos), int(n_age), ag.ctypes.data, int(window), int(origin),
                                                           pr.ctypes.data, pr.size, lv.ctypes.data, lv.size, C.byref(W), C.byref(G), err,
                                                           len(err)) != 0:
        raise ValueError(err.value.decode())
    return W.value, G.value


F_DISPERSION = 28  # enum sepaihrd_field SEPAIHRD_F_DISPERSION: param_index 0, 1, 2 = the dispersion of the H, ICU, D series

_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen the HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SEPAIHRD_HIP_LIB") or LIB_PATH  # env override: experiment builds only
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 /
    # libhsa-runtime64 and a second copy (the system ROCm the library was linked against) cannot
    # open the device once the first has.  Importing torch FIRST makes the dynamic linker resolve
    # our NEEDED libamdhip64.so.7 to the already-loaded copy (same SONAME), so torch tensors,
    # torch streams and these kernels share one runtime.  Without torch (C++ hosts) the system
    # runtime from the library's RUNPATH is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); "
            "the HIP path has no CPU fallback")
    lib = C.CDLL(p)
    vp = C.c_void_p
    lib.sepaihrd_create.restype = vp
    lib.sepaihrd_create.argtypes = [C.POINTER(sepaihrd_problem), C.c_int, C.c_char_p, C.c_int]
    lib.sepaihrd_destroy.restype = None
    lib.sepaihrd_destroy.argtypes = [vp]
    lib.sepaihrd_last_error.restype = C.c_char_p
    lib.sepaihrd_last_error.argtypes = [vp]
    lib.sepaihrd_abi_version.restype = C.c_int
    lib.sepaihrd_set_constraint_mode.argtypes = [vp, C.c_int]
    lib.sepaihrd_set_arith.argtypes = [vp, C.c_int]
    lib.sepaihrd_set_precision.argtypes = [vp, C.c_int]
    lib.sepaihrd_set_integrator_form.argtypes = [vp, C.c_int]
    lib.sepaihrd_eval_batch.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_eval_batch_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_apply_constraints.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    lib.sepaihrd_get_kernel_info.argtypes = [vp, C.POINTER(sepaihrd_kernel_info)]
    lib.sepaihrd_get_kernel_info_for_batch.argtypes = [vp, C.c_int32, C.POINTER(sepaihrd_kernel_info)]
    lib.sepaihrd_reserve.argtypes = [vp, C.c_int]
    lib.sepaihrd_set_timing.argtypes = [vp, C.c_int]
    lib.sepaihrd_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.sepaihrd_mh_create.restype = vp
    lib.sepaihrd_mh_create.argtypes = [vp, C.POINTER(sepaihrd_mh_config), vp, vp]
    lib.sepaihrd_mh_sample_count.argtypes = [vp]
    lib.sepaihrd_mh_read_samples.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.sepaihrd_mh_read_moments.argtypes = [vp, vp, vp]
    lib.sepaihrd_mh_summary_records.argtypes = [vp, C.c_int, vp, vp]
    lib.sepaihrd_records_buffer.restype = vp
    lib.sepaihrd_records_buffer.argtypes = [vp, C.c_int, C.c_size_t]
    lib.sepaihrd_allgather_records.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.sepaihrd_read_records.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.sepaihrd_write_records.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.sepaihrd_mh_set_values.argtypes = [vp, vp]
    # every entry point a Python caller may reach takes its pointers as pointers (a bare int would be cut to 32 bits)
    lib.sepaihrd_abi_version.argtypes = []
    lib.sepaihrd_eval_batch_begin.argtypes = [vp, vp, C.c_int]
    lib.sepaihrd_eval_batch_end.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_fd_gradient_batch.argtypes = [vp, vp, vp, vp, C.c_int, C.c_double, vp, vp, vp, vp]
    lib.sepaihrd_mh_stage_normals.argtypes = [vp, vp]
    lib.sepaihrd_mh_staging_buffer.restype = vp
    lib.sepaihrd_mh_staging_buffer.argtypes = [vp]
    lib.sepaihrd_mh_step.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_int]
    lib.sepaihrd_mh_test_buffer.restype = vp
    lib.sepaihrd_mh_test_buffer.argtypes = [vp]
    lib.sepaihrd_mh_step_tested.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    lib.sepaihrd_mh_fetch_test.argtypes = [vp, vp, vp]
    lib.sepaihrd_mh_read_best.argtypes = [vp, vp]
    lib.sepaihrd_mh_busy.argtypes = [vp]
    lib.sepaihrd_mh_seed_streams.argtypes = [vp, C.c_uint32]
    lib.sepaihrd_mh_draw_first.argtypes = [vp]
    lib.sepaihrd_mh_keep_scale_on_device.argtypes = [vp, C.c_int, C.c_double, C.c_int]
    lib.sepaihrd_mh_read_run_state.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_mh_read_sample_values.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.sepaihrd_mh_read_accept_trace.argtypes = [vp, vp]
    lib.sepaihrd_device_libm_check.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.sepaihrd_device_log_values.argtypes = [vp, vp, C.c_int32, vp]
    lib.sepaihrd_mh_read_failure_counts.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.sepaihrd_mh_snapshot_begin.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    lib.sepaihrd_mh_snapshot_end.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.sepaihrd_mh_destroy.restype = None
    lib.sepaihrd_mh_destroy.argtypes = [vp]
    lib.sepaihrd_mh_evaluate_current.argtypes = [vp, vp, vp]
    lib.sepaihrd_mh_propose.argtypes = [vp, vp, vp, vp, vp]
    lib.sepaihrd_mh_fetch.argtypes = [vp, vp, vp]
    lib.sepaihrd_mh_commit.argtypes = [vp, vp]
    lib.sepaihrd_mh_adapt.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    lib.sepaihrd_mh_read_history.argtypes = [vp, vp, C.c_int, vp]
    lib.sepaihrd_mh_read_covariance.argtypes = [vp, vp]
    lib.sepaihrd_mh_read_proposal.argtypes = [vp, vp]
    lib.sepaihrd_mh_history_length.argtypes = [vp]
    lib.sepaihrd_set_initial_state_mode.argtypes = [vp, C.c_int]
    lib.sepaihrd_ensemble_quantiles.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_scenario_ensemble.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_chain_diagnostics.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.sepaihrd_mh_diagnostics.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.sepaihrd_sir_create.restype = vp
    lib.sepaihrd_sir_create.argtypes = [C.POINTER(sepaihrd_sir_problem), C.c_int, C.c_char_p, C.c_int]
    lib.sepaihrd_sir_destroy.restype = None
    lib.sepaihrd_sir_destroy.argtypes = [vp]
    lib.sepaihrd_sir_last_error.restype = C.c_char_p
    lib.sepaihrd_sir_last_error.argtypes = [vp]
    lib.sepaihrd_sir_eval_batch.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.sepaihrd_sir_eval_batch_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_sir_reserve.argtypes = [vp, C.c_int]
    lib.sepaihrd_sir_apply_constraints.argtypes = [vp, vp, C.c_int, vp]
    lib.sepaihrd_sir_set_arith.argtypes = [vp, C.c_int]
    lib.sepaihrd_sir_mh_create.restype = vp
    lib.sepaihrd_sir_mh_create.argtypes = [vp, C.POINTER(sepaihrd_mh_config), vp, vp]
    lib.sepaihrd_sir_device_libm_check.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.sepaihrd_sir_constraint_bounds.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.sepaihrd_sir_validate_events.argtypes = [vp, vp, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.sepaihrd_sir_scenario_ensemble.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_sir_ensemble_quantiles.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.sepaihrd_sir_ensemble_timing.argtypes = [vp, C.POINTER(C.c_int64), vp]
    lib.sepaihrd_mh_set_kernel_form.argtypes = [vp, C.c_int]
    lib.sepaihrd_stoch_sir_num_steps.restype = C.c_int64
    lib.sepaihrd_stoch_sir_num_steps.argtypes = [C.c_double, C.c_double, C.c_double]
    lib.sepaihrd_stoch_sir_validate.argtypes = [C.POINTER(sepaihrd_stoch_sir_config), vp, C.c_char_p, C.c_int]
    lib.sepaihrd_stoch_sir_run.argtypes = [C.c_int, C.POINTER(sepaihrd_stoch_sir_config), vp, vp, vp, vp, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_stoch_sir_binomial_device.argtypes = [C.c_int, C.c_uint64, vp, vp, C.c_int, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_mh_get_kernel_form.argtypes = [vp]
    lib.sepaihrd_ensemble_predictive.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_predictive_validate.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_char_p, C.c_int]
    lib.sepaihrd_predictive_timing.argtypes = [vp, vp]
    lib.sepaihrd_ensemble_stochastic.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int, C.c_int] + [vp] * 7
    lib.sepaihrd_stochastic_validate.argtypes = [C.c_int] * 7 + [vp, C.c_int, C.c_char_p, C.c_int]
    lib.sepaihrd_stochastic_values_width.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.sepaihrd_stochastic_timing.argtypes = [vp, vp]
    lib.sepaihrd_poisson_device.argtypes = [C.c_int, C.c_uint64, vp, C.c_int, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_ensemble_predictive_nb.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_ensemble_predictive_scores.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, C.c_int, vp, C.c_int,
                                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.sepaihrd_predictive_scores_validate.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_char_p, C.c_int]
    lib.sepaihrd_ensemble_predictive_targets.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp,
                                                         C.c_int] + [vp] * 12
    lib.sepaihrd_predictive_targets_validate.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int,
                                                         vp, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_gamma_device.argtypes = [C.c_int, C.c_uint64, vp, C.c_int, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_nb_draw_device.argtypes = [C.c_int, C.c_uint64, vp, vp, C.c_int, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_particle_loglik.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64] + [vp] * 7
    lib.sepaihrd_particle_validate.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_int]
    lib.sepaihrd_particle_max_particles.argtypes = [C.c_int]
    lib.sepaihrd_particle_timing.argtypes = [vp, vp]
    lib.sepaihrd_particle_resample_device.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_int, vp, C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.c_char_p, C.c_int]
    lib.sepaihrd_particle_loglik_wide.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int] + [vp] * 7
    lib.sepaihrd_particle_wide_validate.argtypes = [C.c_int] * 7 + [C.c_char_p, C.c_int]
    lib.sepaihrd_particle_wide_max_particles.argtypes = []
    lib.sepaihrd_particle_wide_timing.argtypes = [vp, vp]
    lib.sepaihrd_particle_wide_resample_device.argtypes = lib.sepaihrd_particle_resample_device.argtypes
    lib.sepaihrd_particle_loglik_nb.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp] + [vp] * 7
    lib.sepaihrd_particle_loglik_wide_nb.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_int] + [vp] * 7
    lib.sepaihrd_particle_nb_validate.argtypes = [vp, C.c_char_p, C.c_int]
    lib.sepaihrd_particle_nb_row_constants.argtypes = [vp, vp, vp]
    lib.sepaihrd_particle_nb_term_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_double, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_particle_filter_states.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, vp, vp, C.c_int] + [vp] * 8
    lib.sepaihrd_particle_states_validate.argtypes = [C.c_int] * 7 + [vp, C.c_int, C.c_char_p, C.c_int]
    lib.sepaihrd_particle_states_timing.argtypes = [vp, vp]
    lib.sepaihrd_set_dispersion.argtypes = [vp, vp]
    lib.sepaihrd_get_dispersion.argtypes = [vp, vp]
    lib.sepaihrd_dispersion_validate.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, C.c_char_p, C.c_int]
    lib.sepaihrd_nb_objective_host.argtypes = [vp] * 5 + [C.c_int] * 3 + [vp] * 3
    lib.sepaihrd_lgamma_host.restype = C.c_double
    lib.sepaihrd_lgamma_host.argtypes = [C.c_double]
    lib.sepaihrd_lgamma_device.argtypes = [C.c_int, vp, C.c_int, vp, C.c_char_p, C.c_int]
    if path is None:
        _lib = lib
    return lib


def _ptr(a: np.ndarray, typ):
    return a.ctypes.data_as(typ)


def build_problem_struct(pb: SEPAIHRDProblem, keep: list) -> sepaihrd_problem:
    """Fill the C struct; ``keep`` receives the arrays that must outlive the call."""
    n = pb.n
    s = sepaihrd_problem()
    s.abi_version = ABI_VERSION
    s.n_age, s.n_times, s.n_obs = n, pb.n_times, pb.n_obs
    s.n_beta, s.n_kappa, s.n_params = len(pb.beta_values), len(pb.kappa_values), pb.n_params
    s.solver, s.constraint_mode, s.arith = pb.solver, pb.constraint_mode, pb.arith
    s.max_attempts = int(getattr(pb, "max_attempts", 0))
    s.precision = int(getattr(pb, "precision", 0))

    def dbl(x):
        a = np.ascontiguousarray(x, dtype=np.float64)
        if a.size == 0:
            a = np.zeros(1)
        keep.append(a)
        return _ptr(a, _dp)

    s.times, s.N = dbl(pb.times), dbl(pb.N)
    s.M = dbl(np.asfortranarray(pb.M).ravel(order="F"))  # column-major like Eigen
    for name in ("a", "h_infec", "p", "h", "icu", "d_H", "d_ICU", "d_community", "beta_end_times",
                 "beta_values", "kappa_end_times", "kappa_values", "initial_state"):
        setattr(s, name, dbl(getattr(pb, name)))
    s.obs_H, s.obs_ICU, s.obs_D = dbl(pb.obs_H), dbl(pb.obs_ICU), dbl(pb.obs_D)
    codes, idxs = pb.field_map()
    lo, hi, has = pb.bounds_arrays()
    keep.extend([codes, idxs, has])
    s.param_field, s.param_index = _ptr(codes, _ip), _ptr(idxs, _ip)
    s.lower, s.upper, s.has_bounds = dbl(lo), dbl(hi), _ptr(has, _up)
    s.beta, s.theta, s.sigma, s.gamma_p = pb.beta, pb.theta, pb.sigma, pb.gamma_p
    s.gamma_A, s.gamma_I, s.gamma_H, s.gamma_ICU = pb.gamma_A, pb.gamma_I, pb.gamma_H, pb.gamma_ICU
    for i in range(8):
        s.multipliers[i] = float(pb.multipliers[i])
    s.runup_days, s.seed_exposed = pb.runup_days, pb.seed_exposed
    s.abs_err, s.rel_err, s.dt_hint = pb.abs_err, pb.rel_err, pb.dt_hint
    return s


class HipObjective:
    """Batched SEPAIHRD objective on one MI355X; mirrors IObjectiveFunction for B thetas."""

    def __init__(self, pb: SEPAIHRDProblem, device: int = -1):
        self.lib = load_library()
        self.pb = pb
        keep: list = []
        st = build_problem_struct(pb, keep)
        err = C.create_string_buffer(512)
        self.ctx = self.lib.sepaihrd_create(C.byref(st), device, err, len(err))
        if not self.ctx:
            raise RuntimeError("sepaihrd_create failed: " + err.value.decode())
        self.P, self.n, self.T = pb.n_params, pb.n, pb.n_times
        self._device = device
        self._fd_perturbed = None
        if getattr(pb, "dispersion", None) is not None:
            self.set_dispersion(pb.dispersion)

    def close(self):
        if getattr(self, "_fd_perturbed", None) is not None:
            self._fd_perturbed.close()
            self._fd_perturbed = None
        if getattr(self, "ctx", None):
            self.lib.sepaihrd_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): " + self.lib.sepaihrd_last_error(self.ctx).decode())

    def getParameterNames(self):
        return list(self.pb.param_names)

    def set_constraint_mode(self, mode: int):
        self._check(self.lib.sepaihrd_set_constraint_mode(self.ctx, mode), "set_constraint_mode")

    def set_arith(self, arith: int):
        self._check(self.lib.sepaihrd_set_arith(self.ctx, arith), "set_arith")

    def set_precision(self, precision: int):
        """PRECISION_F64 (reference arithmetic) or PRECISION_F32 (fp32 state, fp64 likelihood: BASELINE configs[4])."""
        self._check(self.lib.sepaihrd_set_precision(self.ctx, int(precision)), "set_precision")

    def set_integrator_form(self, form: int):
        """FORM_AUTO (by batch size), FORM_LANE_PER_AGE or FORM_QUAD (sixteen lanes per chain): same bits either way."""
        self._check(self.lib.sepaihrd_set_integrator_form(self.ctx, int(form)), "set_integrator_form")

    def set_dispersion(self, k):
        """sepaihrd_set_dispersion: k [3] = the fixed negative-binomial dispersions of the H, ICU, D series (+inf: Poisson; a series
        that theta calibrates, dispersion_H / _ICU / _D, ignores its entry).  ValueError with the validator's message for a k the
        library refuses.  The finite-difference objective's perturbed context, if it exists already, follows."""
        kk = np.ascontiguousarray(k, dtype=np.float64)
        if kk.shape != (3,):
            raise ValueError("dispersion must have three entries: k_H, k_ICU, k_D")
        if self.lib.sepaihrd_set_dispersion(self.ctx, kk.ctypes.data) != 0:
            raise ValueError(self.lib.sepaihrd_last_error(self.ctx).decode())
        if getattr(self, "_fd_perturbed", None) is not None:
            self._fd_perturbed.set_dispersion(kk)

    def get_dispersion(self) -> np.ndarray:
        """sepaihrd_get_dispersion: the fixed dispersions [3], NaN for a series that theta calibrates"""
        k = np.empty(3)
        self._check(self.lib.sepaihrd_get_dispersion(self.ctx, k.ctypes.data), "sepaihrd_get_dispersion")
        return k

    def lgamma_device(self, x) -> np.ndarray:
        """Probe of the device's lgamma_pos (sepaihrd_lgamma_device) on the arguments x > 0"""
        xs = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.empty(xs.size)
        err = C.create_string_buffer(256)
        rc = self.lib.sepaihrd_lgamma_device(getattr(self, "_device", -1), xs.ctypes.data, xs.size, out.ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"sepaihrd_lgamma_device failed ({rc}): " + err.value.decode())
        return out.reshape(np.shape(x))

    def calculate(self, theta) -> float:
        return float(self.eval_batch(np.asarray(theta, dtype=np.float64)[None, :])["loglik"][0])

    def eval_batch(self, theta, want_traj: bool = False) -> dict:
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != self.P:
            raise ValueError(f"theta must be B x {self.P}")
        B = th.shape[0]
        out = {
            "loglik": np.empty(B), "status": np.empty(B, dtype=np.int32),
            "n_accept": np.empty(B, dtype=np.int32), "n_reject": np.empty(B, dtype=np.int32),
            "ll_parts": np.empty((B, 3)),
        }
        traj = np.empty((B, self.T, 11 * self.n)) if want_traj else None
        rc = self.lib.sepaihrd_eval_batch(
            self.ctx, th.ctypes.data, B, out["loglik"].ctypes.data, out["status"].ctypes.data,
            out["n_accept"].ctypes.data, out["n_reject"].ctypes.data, out["ll_parts"].ctypes.data,
            traj.ctypes.data if want_traj else None)
        self._check(rc, "sepaihrd_eval_batch")
        if want_traj:
            out["traj"] = traj
        return out

    def eval_batch_device(self, d_theta, d_loglik, d_status=None, d_n_accept=None, d_n_reject=None,
                          d_ll_parts=None, d_traj=None, stream: int = 0, B: Optional[int] = None):
        """Arguments are torch CUDA tensors (or raw device addresses); async on ``stream``."""
        def addr(t):
            if t is None:
                return None
            return t if isinstance(t, int) else t.data_ptr()
        if B is None:
            B = int(d_theta.shape[0])
        rc = self.lib.sepaihrd_eval_batch_device(self.ctx, addr(d_theta), B, addr(d_loglik), addr(d_status),
                                                 addr(d_n_accept), addr(d_n_reject), addr(d_ll_parts),
                                                 addr(d_traj), stream if stream else None)
        self._check(rc, "sepaihrd_eval_batch_device")

    def fd_perturbed_objective(self) -> "HipObjective":
        """The second context of the finite-difference objective for this problem (kept with this object): the perturbed
        runs' rules -- clamp mode, the calibrated initial-state multipliers unbounded, the others 1.0, x(t0) always scaled
        by the multipliers (SEPAIHRD_INIT_MULTIPLIERS) -- in this context's arithmetic."""
        if getattr(self, "_fd_perturbed", None) is None:
            pb = self.pb
            codes, _ = pb.field_map()
            bounds = dict(pb.bounds)
            for nm, c in zip(pb.param_names, codes):
                if 8 <= c <= 15:
                    bounds[nm] = (-np.inf, np.inf)
            other = HipObjective(pb.with_(bounds=bounds, constraint_mode=CONSTRAINT_CLAMP, multipliers=np.ones(8)),
                                 device=getattr(self, "_device", -1))
            other.set_initial_state_mode(2)
            other.set_dispersion(np.where(np.isnan(self.get_dispersion()), np.inf, self.get_dispersion()))  # the same observation model
            self._fd_perturbed = other
        return self._fd_perturbed

    def fd_gradient_batch(self, theta, want_grad=None, fd_epsilon: float = 1e-4, grad=None) -> dict:
        """sepaihrd_fd_gradient_batch: forward-difference gradients of the C rows of theta in one pass, this context
        evaluating the centres and fd_perturbed_objective() the C x P perturbed vectors.  want_grad [C] (None = all):
        rows with 0 get their value only and their rows of `grad` (an optional array to fill, NaN otherwise) stay
        untouched.  Row for row what HostObjective.evaluate_with_gradient returns; status [C] is the largest
        per-evaluation status of each row."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != self.P:
            raise ValueError(f"theta must be C x {self.P}")
        Cn = th.shape[0]
        codes, _ = self.pb.field_map()
        mult = np.full(8, -1, dtype=np.int32)
        for k, c in enumerate(codes):
            if 8 <= c <= 15 and mult[c - 8] < 0:
                mult[c - 8] = k
        want = None if want_grad is None else np.ascontiguousarray(want_grad, dtype=np.uint8)
        if want is not None and want.shape != (Cn,):
            raise ValueError("want_grad must have one entry per row")
        value, status = np.empty(Cn), np.empty(Cn, dtype=np.int32)
        if grad is None:
            grad = np.full((Cn, self.P), np.nan)
        if grad.shape != (Cn, self.P) or grad.dtype != np.float64 or not grad.flags.c_contiguous:
            raise ValueError("grad must be a C-contiguous float64 array of theta's shape")
        other = self.fd_perturbed_objective()
        rc = self.lib.sepaihrd_fd_gradient_batch(self.ctx, other.ctx, th.ctypes.data, None if want is None else want.ctypes.data, Cn,
                                                 float(fd_epsilon), mult.ctypes.data, value.ctypes.data, grad.ctypes.data,
                                                 status.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"sepaihrd_fd_gradient_batch failed ({rc}): " + self.lib.sepaihrd_last_error(other.ctx).decode())
        return {"value": value, "grad": grad, "status": status}

    def set_timing(self, enable):
        """True / 1: events around every launch; k > 1: around every k-th launch; False / 0: off."""
        self._check(self.lib.sepaihrd_set_timing(self.ctx, int(enable)), "sepaihrd_set_timing")

    def get_timing(self) -> dict:
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        self._check(self.lib.sepaihrd_get_timing(self.ctx, C.byref(a), C.byref(b), C.byref(n)), "sepaihrd_get_timing")
        return {"integrator_ms": a.value, "likelihood_ms": b.value, "launches": n.value}

    def set_initial_state_mode(self, mode: int):
        """0: x(t0) derived from theta (objective); 1: problem.initial_state as given (ensemble runs)."""
        self._check(self.lib.sepaihrd_set_initial_state_mode(self.ctx, int(mode)), "set_initial_state_mode")

    def ensemble_quantiles(self, theta, probs, want_sero: bool = True, want_rt: bool = False,
                           want_metrics: bool = False) -> dict:
        """Posterior-ensemble summaries (ResultAggregator.cpp:297-345, MetricsCalculator.cpp:199-226):
        ppc [6][n_probs][T_pos][n], sero [n_probs][T], status [S], n_valid."""
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        S, npb = th.shape[0], pr.size
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        ppc = np.empty((6, npb, Tp, self.pb.n))
        sero = np.empty((npb, self.pb.n_times)) if want_sero else None
        rt = np.empty((npb, self.pb.n_times)) if want_rt else None
        met = np.empty((S, 12 + 4 * self.pb.n)) if want_metrics else None
        status = np.empty(S, dtype=np.int32)
        nv = C.c_int32(0)
        self._check(self.lib.sepaihrd_ensemble_quantiles(
            self.ctx, th.ctypes.data, S, pr.ctypes.data, npb, ppc.ctypes.data,
            sero.ctypes.data if want_sero else None, rt.ctypes.data if want_rt else None,
            met.ctypes.data if want_metrics else None, status.ctypes.data, C.byref(nv)), "ensemble_quantiles")
        out = {"ppc": ppc, "status": status, "n_valid": nv.value}
        if want_sero:
            out["sero"] = sero
        if want_rt:
            out["rt"] = rt
        if want_metrics:
            out["metrics"] = met
        return out

    CONTEXT_DISPERSION = "context"  # ensemble_predictive(dispersion=...): the context's own, per sample

    def ensemble_predictive(self, theta, R: int, seed: int, probs, want_pit: bool = True, want_means: bool = False,
                            want_draws: bool = False, dispersion=None) -> dict:
        """Posterior predictive draws with Poisson noise (sepaihrd_ensemble_predictive): R replicates y ~ Poisson(mean) per
        sample.  pred [6][n_probs][T_pos][n] (quantiles over the draws of the valid samples), pit [3][T_pos][n] (mid-PIT of
        the usable observations, NaN elsewhere), means [S][3][T_pos][n], draws [S][R][3][T_pos][n], status [S], n_valid,
        phase_ms (integrator; draws and PIT counts; sorts and quantiles).
        dispersion (None: the call above, whatever the context's dispersion): negative-binomial noise through
        sepaihrd_ensemble_predictive_nb.  HipObjective.CONTEXT_DISPERSION ("context"): each sample's k as eval_batch would take it
        (the constrained theta entry of a calibrated series, the fixed value of set_dispersion otherwise); (k_H, k_ICU, k_D): these
        for every sample, each +inf or finite in [1e-3, 1e6] (ValueError otherwise).  The result gains k_used [S][3]."""
        if dispersion is not None:
            return self._ensemble_predictive_nb(theta, R, seed, probs, want_pit, want_means, want_draws, dispersion)
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        S, npb, n, R = th.shape[0], pr.size, self.pb.n, int(R)
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        pred = np.empty((6, npb, Tp, n))
        pit = np.empty((3, Tp, n)) if want_pit else None
        means = np.empty((S, 3, Tp, n)) if want_means else None
        draws = np.empty((S, max(R, 0), 3, Tp, n)) if want_draws else None
        status = np.empty(S, dtype=np.int32)
        nv = C.c_int32(0)
        self._check(self.lib.sepaihrd_ensemble_predictive(
            self.ctx, th.ctypes.data, S, R, int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, npb, pred.ctypes.data,
            pit.ctypes.data if want_pit else None, means.ctypes.data if want_means else None,
            draws.ctypes.data if want_draws else None, status.ctypes.data, C.byref(nv)), "ensemble_predictive")
        ms = np.zeros(3)
        self._check(self.lib.sepaihrd_predictive_timing(self.ctx, ms.ctypes.data), "predictive_timing")
        out = {"pred": pred, "status": status, "n_valid": nv.value, "phase_ms": ms}
        if want_pit:
            out["pit"] = pit
        if want_means:
            out["means"] = means
        if want_draws:
            out["draws"] = draws
        return out

    def _ensemble_predictive_nb(self, theta, R, seed, probs, want_pit, want_means, want_draws, dispersion) -> dict:
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        S, npb, n, R = th.shape[0], pr.size, self.pb.n, int(R)
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        disp = None
        if not (isinstance(dispersion, str) and dispersion == self.CONTEXT_DISPERSION):
            disp = np.ascontiguousarray(dispersion, dtype=np.float64).ravel()
            if disp.size != 3:
                raise ValueError("dispersion must hold three entries: k_H, k_ICU, k_D")
        pred = np.empty((6, npb, Tp, n))
        pit = np.empty((3, Tp, n)) if want_pit else None
        means = np.empty((S, 3, Tp, n)) if want_means else None
        draws = np.empty((S, max(R, 0), 3, Tp, n)) if want_draws else None
        k_used = np.empty((S, 3))
        status = np.empty(S, dtype=np.int32)
        nv = C.c_int32(0)
        rc = self.lib.sepaihrd_ensemble_predictive_nb(
            self.ctx, th.ctypes.data, S, R, int(seed) & 0xFFFFFFFFFFFFFFFF, None if disp is None else disp.ctypes.data, pr.ctypes.data, npb,
            pred.ctypes.data, pit.ctypes.data if want_pit else None, means.ctypes.data if want_means else None,
            draws.ctypes.data if want_draws else None, k_used.ctypes.data, status.ctypes.data, C.byref(nv))
        if rc == -1 and disp is not None and not np.all(np.isposinf(disp) | ((disp >= 1e-3) & (disp <= 1e6))):
            raise ValueError(self.lib.sepaihrd_last_error(self.ctx).decode())  # sepaihrd_particle_nb_validate's message
        self._check(rc, "ensemble_predictive_nb")
        ms = np.zeros(3)
        self._check(self.lib.sepaihrd_predictive_timing(self.ctx, ms.ctypes.data), "predictive_timing")
        out = {"pred": pred, "status": status, "n_valid": nv.value, "phase_ms": ms, "k_used": k_used}
        if want_pit:
            out["pit"] = pit
        if want_means:
            out["means"] = means
        if want_draws:
            out["draws"] = draws
        return out

    def ensemble_predictive_scores(self, theta, R: int, seed: int, probs, levels, observed=None, dispersion="context",
                                   want_means: bool = False, want_draws: bool = False) -> dict:
        """The posterior predictive draws scored against data on the device (sepaihrd_ensemble_predictive_scores): the dict of
        ensemble_predictive(..., dispersion=dispersion) -- pred, pit, status, n_valid, phase_ms, k_used, means and draws on
        request, the same bits -- plus cell_scores [3][T_pos][n][5 + 4 L], summary [3][n + 1][4 + 2 L] (entry n pools the ages),
        exact (the sums were exact: the host twin gives the same bits), levels, observed (the table scored against) and the named
        views of score_views.  observed [3][T_pos][n] (None: the context's observations) is what the scores and the PIT are taken
        against: a cell is usable when finite and >= 0.  levels: up to 8 central coverage levels inside (0, 1).  phase_ms: integrator;
        draws and counts; sorts, quantiles and scores.  ValueError for an argument sepaihrd_predictive_scores_validate refuses."""
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
        S, npb, n, R, L = th.shape[0], pr.size, self.pb.n, int(R), lv.size
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        ob = None
        if observed is not None:
            ob = np.ascontiguousarray(observed, dtype=np.float64)
            if ob.shape != (3, Tp, n):
                raise ValueError("observed must be [3][T_pos][n]: (3, %d, %d), not %s" % (Tp, n, ob.shape))
        disp = None
        if not (isinstance(dispersion, str) and dispersion == self.CONTEXT_DISPERSION):
            disp = np.ascontiguousarray(dispersion, dtype=np.float64).ravel()
            if disp.size != 3:
                raise ValueError("dispersion must hold three entries: k_H, k_ICU, k_D")
        err = C.create_string_buffer(512)
        if S > 0 and R > 0 and self.lib.sepaihrd_predictive_validate(S, R, Tp, n, pr.ctypes.data, npb, None, 0) == 0 and \
                self.lib.sepaihrd_predictive_scores_validate(S, R, Tp, n, pr.ctypes.data, npb, lv.ctypes.data, L, err, len(err)) != 0:
            raise ValueError(err.value.decode())  # the levels: the arguments of the predictive call keep its own errors
        pred, pit = np.empty((6, npb, Tp, n)), np.empty((3, Tp, n))
        cell_scores, summary = np.empty((3, Tp, n, 5 + 4 * L)), np.empty((3, n + 1, 4 + 2 * L))
        means = np.empty((S, 3, Tp, n)) if want_means else None
        draws = np.empty((S, max(R, 0), 3, Tp, n)) if want_draws else None
        k_used = np.empty((S, 3))
        status = np.empty(S, dtype=np.int32)
        nv, exact = C.c_int32(0), C.c_int32(0)
        rc = self.lib.sepaihrd_ensemble_predictive_scores(
            self.ctx, th.ctypes.data, S, R, int(seed) & 0xFFFFFFFFFFFFFFFF, None if disp is None else disp.ctypes.data,
            None if ob is None else ob.ctypes.data, pr.ctypes.data, npb, lv.ctypes.data, L, pred.ctypes.data, pit.ctypes.data,
            cell_scores.ctypes.data, summary.ctypes.data, means.ctypes.data if want_means else None,
            draws.ctypes.data if want_draws else None, k_used.ctypes.data, status.ctypes.data, C.byref(nv), C.byref(exact))
        if rc == -1 and disp is not None and not np.all(np.isposinf(disp) | ((disp >= 1e-3) & (disp <= 1e6))):
            raise ValueError(self.lib.sepaihrd_last_error(self.ctx).decode())  # sepaihrd_particle_nb_validate's message
        self._check(rc, "ensemble_predictive_scores")
        ms = np.zeros(3)
        self._check(self.lib.sepaihrd_predictive_timing(self.ctx, ms.ctypes.data), "predictive_timing")
        if ob is None:
            from . import hostabi
            ob = hostabi.observed_table(self.pb)
        out = {"pred": pred, "pit": pit, "status": status, "n_valid": nv.value, "phase_ms": ms, "k_used": k_used,
               "cell_scores": cell_scores, "summary": summary, "exact": bool(exact.value), "levels": lv, "observed": ob}
        if want_means:
            out["means"] = means
        if want_draws:
            out["draws"] = draws
        out.update(score_views(cell_scores, summary, ob, lv))
        return out

    def ensemble_predictive_targets(self, theta, R: int, seed: int, probs, levels, age_group, window: int, origin: int = 0, observed=None,
                                    dispersion="context", want_means: bool = False, want_draws: bool = False,
                                    want_target_draws: bool = False) -> dict:
        """The posterior predictive draws scored on window and age-group totals on the device
        (sepaihrd_ensemble_predictive_targets): the draws of ensemble_predictive_scores(..., dispersion=dispersion) summed into
        targets -- age_group [n] (-1: left out, else a group id 0 .. G - 1) x windows of `window` output rows from row `origin`,
        W = (T_pos - origin) // window of them, and the running sums of those totals.  target_quantiles [6][n_probs][W][G], pit,
        target_obs [6][W][G], target_scores [6][W][G][5 + 4 L], summary [6][G + 1][4 + 2 L] (entry G pools the groups), exact,
        W, G, window_first_row [W], levels, age_group, the named views of target_views, and status, n_valid, k_used, phase_ms
        (means, the daily draws and target_draws [S][R][3][W][G] on request) as the scored call gives them.  observed
        [3][T_pos][n] (None: the context's observations) is the daily table the observed targets are summed from.  ValueError for
        an argument sepaihrd_predictive_targets_validate refuses."""
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
        ag = np.ascontiguousarray(age_group, dtype=np.int32).ravel()
        S, npb, n, R, L = th.shape[0], pr.size, self.pb.n, int(R), lv.size
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        ob = None
        if observed is not None:
            ob = np.ascontiguousarray(observed, dtype=np.float64)
            if ob.shape != (3, Tp, n):
                raise ValueError("observed must be [3][T_pos][n]: (3, %d, %d), not %s" % (Tp, n, ob.shape))
        disp = None
        if not (isinstance(dispersion, str) and dispersion == self.CONTEXT_DISPERSION):
            disp = np.ascontiguousarray(dispersion, dtype=np.float64).ravel()
            if disp.size != 3:
                raise ValueError("dispersion must hold three entries: k_H, k_ICU, k_D")
        W, G = 1, 1  # where the scored call's own rules fail, the call below refuses with their message before either is read
        if S > 0 and R > 0 and self.lib.sepaihrd_predictive_validate(S, R, Tp, n, pr.ctypes.data, npb, None, 0) == 0:
            W, G = predictive_targets_validate(S, R, Tp, n, ag, window, origin, pr, lv)
        tq, pit, tobs = np.empty((6, npb, W, G)), np.empty((6, W, G)), np.empty((6, W, G))
        tscores, summary = np.empty((6, W, G, 5 + 4 * L)), np.empty((6, G + 1, 4 + 2 * L))
        means = np.empty((S, 3, Tp, n)) if want_means else None
        draws = np.empty((S, max(R, 0), 3, Tp, n)) if want_draws else None
        tdraws = np.empty((S, max(R, 0), 3, W, G)) if want_target_draws else None
        k_used = np.empty((S, 3))
        status = np.empty(S, dtype=np.int32)
        nv, exact = C.c_int32(0), C.c_int32(0)
        rc = self.lib.sepaihrd_ensemble_predictive_targets(
            self.ctx, th.ctypes.data, S, R, int(seed) & 0xFFFFFFFFFFFFFFFF, None if disp is None else disp.ctypes.data,
            None if ob is None else ob.ctypes.data, ag.ctypes.data, int(window), int(origin), pr.ctypes.data, npb, lv.ctypes.data, L,
            tq.ctypes.data, pit.ctypes.data, tscores.ctypes.data, summary.ctypes.data, tobs.ctypes.data,
            None if tdraws is None else tdraws.ctypes.data, means.ctypes.data if want_means else None,
            draws.ctypes.data if want_draws else None, k_used.ctypes.data, status.ctypes.data, C.byref(nv), C.byref(exact))
        if rc == -1 and disp is not None and not np.all(np.isposinf(disp) | ((disp >= 1e-3) & (disp <= 1e6))):
            raise ValueError(self.lib.sepaihrd_last_error(self.ctx).decode())  # sepaihrd_particle_nb_validate's message
        self._check(rc, "ensemble_predictive_targets")
        ms = np.zeros(3)
        self._check(self.lib.sepaihrd_predictive_timing(self.ctx, ms.ctypes.data), "predictive_timing")
        out = {"target_quantiles": tq, "pit": pit, "target_obs": tobs, "target_scores": tscores, "summary": summary,
               "exact": bool(exact.value), "W": W, "G": G, "window": int(window), "origin": int(origin),
               "window_first_row": int(origin) + int(window) * np.arange(W), "levels": lv, "age_group": ag, "status": status,
               "n_valid": nv.value, "phase_ms": ms, "k_used": k_used}
        if want_means:
            out["means"] = means
        if want_draws:
            out["draws"] = draws
        if want_target_draws:
            out["target_draws"] = tdraws
        out.update(target_views(tscores, summary, tobs, lv))
        return out

    def ensemble_stochastic(self, theta, R: int, steps_per_interval: int, seed: int, probs, keep: int = 0, want_extinct: bool = True,
                            want_values: bool = False, want_final: bool = False) -> dict:
        """Stochastic chain-binomial SEPAIHRD replicates of every sample (sepaihrd_ensemble_stochastic): R replicates per row
        of theta, steps_per_interval binomial steps per output interval.  quantiles [6][n_probs][T_pos][n] (daily
        hospitalisations, ICU admissions, deaths and their running sums over the replicates of the valid samples), extinct [S],
        model_values [S][W], traj [S][keep][T][11][n], final_state [S][R][11][n], status [S], n_valid, phase_ms (step kernel;
        sorts and quantiles)."""
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        S, npb, n, R, keep = th.shape[0], pr.size, self.pb.n, int(R), int(keep)
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        W = self.lib.sepaihrd_stochastic_values_width(n, len(self.pb.beta_end_times), len(self.pb.kappa_end_times))
        q = np.empty((6, npb, Tp, n))
        extinct = np.empty(S) if want_extinct else None
        values = np.empty((S, W)) if want_values else None
        traj = np.empty((S, keep, self.pb.n_times, 11, n)) if 0 < keep <= max(R, 0) else None
        final = np.empty((S, max(R, 0), 11, n)) if want_final else None
        status = np.empty(S, dtype=np.int32)
        nv = C.c_int32(0)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._check(self.lib.sepaihrd_ensemble_stochastic(
            self.ctx, th.ctypes.data, S, R, int(steps_per_interval), int(seed) & 0xFFFFFFFFFFFFFFFF, pr.ctypes.data, npb, keep, q.ctypes.data,
            ptr(extinct), ptr(values), ptr(traj), ptr(final), status.ctypes.data, C.byref(nv)), "ensemble_stochastic")
        ms = np.zeros(2)
        self._check(self.lib.sepaihrd_stochastic_timing(self.ctx, ms.ctypes.data), "stochastic_timing")
        out = {"quantiles": q, "status": status, "n_valid": nv.value, "phase_ms": ms}
        for key, arr in (("extinct", extinct), ("model_values", values), ("traj", traj), ("final_state", final)):
            if arr is not None:
                out[key] = arr
        return out

    def particle_max_particles(self) -> int:
        """sepaihrd_particle_max_particles for this problem's age classes: the largest J particle_loglik takes"""
        return int(self.lib.sepaihrd_particle_max_particles(self.pb.n))

    def particle_loglik(self, theta, J: int, steps_per_interval: int, seed: int, want_increments: bool = True, want_ess: bool = True,
                        want_final: bool = False, want_values: bool = False, dispersion=None) -> dict:
        """The bootstrap particle filter of the stochastic SEPAIHRD model (sepaihrd_particle_loglik): J particles per row of theta,
        steps_per_interval binomial steps per output interval, systematic resampling at every observed row.  loglik [B] (the
        estimate of log p(y | theta); -DBL_MAX for an invalid theta), increments [B][T_pos], ess [B][T_pos], final_state
        [B][J][11][n], model_values [B][W], status [B], n_valid.  dispersion = (k_H, k_ICU, k_D), each +inf or finite in
        [1e-3, 1e6]: the negative-binomial observation model through sepaihrd_particle_loglik_nb (None: the Poisson call)."""
        if dispersion is not None:
            return self._particle_call("particle_loglik_nb", self.lib.sepaihrd_particle_loglik_nb, (), theta, J, steps_per_interval, seed,
                                       want_increments, want_ess, want_final, want_values, dispersion)
        return self._particle_call("particle_loglik", self.lib.sepaihrd_particle_loglik, (), theta, J, steps_per_interval, seed, want_increments,
                                   want_ess, want_final, want_values)

    def particle_loglik_wide(self, theta, J: int, steps_per_interval: int, seed: int, theta_chunk: int = 0, want_increments: bool = True,
                             want_ess: bool = True, want_final: bool = False, want_values: bool = False, dispersion=None) -> dict:
        """The wide form of particle_loglik (sepaihrd_particle_loglik_wide): the particles in device memory, J up to 65 536, the
        thetas theta_chunk at a time (0: chosen by the call).  The same outputs, bit for bit where particle_loglik takes J.
        dispersion as in particle_loglik, through sepaihrd_particle_loglik_wide_nb."""
        if dispersion is not None:
            return self._particle_call("particle_loglik_wide_nb", self.lib.sepaihrd_particle_loglik_wide_nb, (int(theta_chunk),), theta, J,
                                       steps_per_interval, seed, want_increments, want_ess, want_final, want_values, dispersion)
        return self._particle_call("particle_loglik_wide", self.lib.sepaihrd_particle_loglik_wide, (int(theta_chunk),), theta, J, steps_per_interval,
                                   seed, want_increments, want_ess, want_final, want_values)

    def _particle_call(self, who, fn, extra, theta, J, steps_per_interval, seed, want_increments, want_ess, want_final, want_values,
                       dispersion=None) -> dict:
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        B, n, J = th.shape[0], self.pb.n, int(J)
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        W = self.lib.sepaihrd_stochastic_values_width(n, len(self.pb.beta_end_times), len(self.pb.kappa_end_times))
        loglik = np.empty(B)
        inc = np.empty((B, Tp)) if want_increments else None
        ess = np.empty((B, Tp)) if want_ess else None
        final = np.empty((B, max(J, 0), 11, n)) if want_final else None
        values = np.empty((B, W)) if want_values else None
        status = np.empty(B, dtype=np.int32)
        nv = C.c_int32(0)
        ptr = lambda a: None if a is None else a.ctypes.data
        if dispersion is not None:  # the _nb calls take it after the seed
            disp = np.ascontiguousarray(dispersion, dtype=np.float64).ravel()
            if disp.size != 3:
                raise ValueError("dispersion must hold three entries: k_H, k_ICU, k_D")
            extra = (disp.ctypes.data,) + tuple(extra)
        self._check(fn(self.ctx, th.ctypes.data, B, J, int(steps_per_interval), int(seed) & 0xFFFFFFFFFFFFFFFF, *extra, loglik.ctypes.data, ptr(inc),
                       ptr(ess), ptr(final), ptr(values), status.ctypes.data, C.byref(nv)), who)
        out = {"loglik": loglik, "status": status, "n_valid": nv.value}
        for key, arr in (("increments", inc), ("ess", ess), ("final_state", final), ("model_values", values)):
            if arr is not None:
                out[key] = arr
        return out

    def particle_filter_states(self, theta, J: int, steps_per_interval: int, seed: int, probs=(), dispersion=None, theta_chunk: int = 0,
                               want_increments: bool = True, want_ess: bool = True, want_quantiles: bool = True,
                               want_values: bool = False) -> dict:
        """The filtered state means and quantile bands of every output row (sepaihrd_particle_filter_states): the wide form of
        the filter, J up to 65 536, summarised after every row over the J particles the next interval starts from.  state_mean
        [B][T][11][n + 1] (index n: the age total), state_quantiles [B][T][11][n + 1][len(probs)] (where probs is not empty and
        want_quantiles), and loglik, increments, ess, status, n_valid, model_values as particle_loglik_wide gives them, bit for
        bit.  dispersion as in particle_loglik."""
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        B, n, T = th.shape[0], self.pb.n, len(self.pb.times)
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        W = self.lib.sepaihrd_stochastic_values_width(n, len(self.pb.beta_end_times), len(self.pb.kappa_end_times))
        disp = None
        if dispersion is not None:
            disp = np.ascontiguousarray(dispersion, dtype=np.float64).ravel()
            if disp.size != 3:
                raise ValueError("dispersion must hold three entries: k_H, k_ICU, k_D")
        loglik = np.empty(B)
        inc = np.empty((B, Tp)) if want_increments else None
        ess = np.empty((B, Tp)) if want_ess else None
        mean = np.empty((B, T, 11, n + 1))
        quant = np.empty((B, T, 11, n + 1, pr.size)) if (want_quantiles and pr.size) else None
        values = np.empty((B, W)) if want_values else None
        status = np.empty(B, dtype=np.int32)
        nv = C.c_int32(0)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._check(self.lib.sepaihrd_particle_filter_states(self.ctx, th.ctypes.data, B, int(J), int(steps_per_interval),
                                                             int(seed) & 0xFFFFFFFFFFFFFFFF, int(theta_chunk), ptr(disp),
                                                             pr.ctypes.data if pr.size else None, pr.size, loglik.ctypes.data, ptr(inc), ptr(ess),
                                                             mean.ctypes.data, ptr(quant), ptr(values), status.ctypes.data, C.byref(nv)),
                    "particle_filter_states")
        out = {"loglik": loglik, "status": status, "n_valid": nv.value, "state_mean": mean}
        for key, arr in (("increments", inc), ("ess", ess), ("state_quantiles", quant), ("model_values", values)):
            if arr is not None:
                out[key] = arr
        return out

    def particle_states_timing(self) -> np.ndarray:
        """Device time of the last particle_filter_states call in ms: decode; all launches; of these the summaries of the first
        chunk of thetas, the whole share where the call has one chunk (sepaihrd_particle_states_timing)"""
        ms = np.zeros(3)
        self._check(self.lib.sepaihrd_particle_states_timing(self.ctx, ms.ctypes.data), "particle_states_timing")
        return ms

    def particle_nb_row_constants(self, dispersion) -> np.ndarray:
        """sepaihrd_particle_nb_row_constants (host only): G [T_pos], the row constants a call with this dispersion uploads"""
        disp = np.ascontiguousarray(dispersion, dtype=np.float64).ravel()
        if disp.size != 3:
            raise ValueError("dispersion must hold three entries: k_H, k_ICU, k_D")
        G = np.empty(int(np.sum(np.asarray(self.pb.times) >= 0.0)))
        if self.lib.sepaihrd_particle_nb_row_constants(self.ctx, disp.ctypes.data, G.ctypes.data) != 0:
            raise ValueError("sepaihrd_particle_nb_row_constants refused the dispersion")
        return G

    def particle_nb_term_device(self, obs, inc, k: float) -> np.ndarray:
        """Probe of the device's negative-binomial term (sepaihrd_particle_nb_term_device): out[i] for the observation obs[i] and
        the increment inc[i] (int32) under the dispersion k"""
        ob = np.ascontiguousarray(obs, dtype=np.float64).ravel()
        ic = np.ascontiguousarray(inc, dtype=np.int32).ravel()
        if ob.size != ic.size:
            raise ValueError("obs and inc must have the same number of cells")
        out = np.empty(ob.size)
        err = C.create_string_buffer(512)
        rc = self.lib.sepaihrd_particle_nb_term_device(getattr(self, "_device", -1), ob.ctypes.data, ic.ctypes.data, ob.size, float(k),
                                                       out.ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"sepaihrd_particle_nb_term_device failed ({rc}): " + err.value.decode())
        return out

    def particle_timing(self) -> np.ndarray:
        """Device time of the last particle_loglik call (with or without a dispersion) in ms: decode; filter kernel
        (sepaihrd_particle_timing)"""
        ms = np.zeros(2)
        self._check(self.lib.sepaihrd_particle_timing(self.ctx, ms.ctypes.data), "particle_timing")
        return ms

    def particle_wide_timing(self) -> np.ndarray:
        """Device time of the last particle_loglik_wide call (with or without a dispersion) in ms: decode; all filter launches
        (sepaihrd_particle_wide_timing)"""
        ms = np.zeros(2)
        self._check(self.lib.sepaihrd_particle_wide_timing(self.ctx, ms.ctypes.data), "particle_wide_timing")
        return ms

    def particle_resample_device(self, logw, seed: int, b: int = 0, row: int = 0) -> dict:
        """Probe of the device's normalisation, scans and ancestor search (sepaihrd_particle_resample_device): one weighted row
        with log-weights logw [J] at the resampling coordinates (seed, b, row).  ancestors [J], increment, ess."""
        return self._resample_probe("sepaihrd_particle_resample_device", logw, seed, b, row)

    def particle_wide_resample_device(self, logw, seed: int, b: int = 0, row: int = 0) -> dict:
        """The same probe through the wide form's normalise-and-resample kernel (sepaihrd_particle_wide_resample_device): J up to
        65 536."""
        return self._resample_probe("sepaihrd_particle_wide_resample_device", logw, seed, b, row)

    def _resample_probe(self, name, logw, seed, b, row) -> dict:
        lw = np.ascontiguousarray(logw, dtype=np.float64).ravel()
        anc = np.empty(lw.size, dtype=np.int32)
        inc, ess = C.c_double(0.0), C.c_double(0.0)
        err = C.create_string_buffer(512)
        rc = getattr(self.lib, name)(getattr(self, "_device", -1), int(seed) & 0xFFFFFFFFFFFFFFFF, int(b), int(row), lw.ctypes.data, lw.size,
                                     anc.ctypes.data, C.byref(inc), C.byref(ess), err, len(err))
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc}): " + err.value.decode())
        return {"ancestors": anc, "increment": inc.value, "ess": ess.value}

    def poisson(self, lam, seed: int) -> np.ndarray:
        """Probe of the device's Poisson sampler (sepaihrd_poisson_device): out[i] at (seed, c0 = i, c1 = c2 = 0)."""
        lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
        out = np.empty(lam.size)
        err = C.create_string_buffer(512)
        rc = self.lib.sepaihrd_poisson_device(getattr(self, "_device", -1), int(seed) & 0xFFFFFFFFFFFFFFFF, lam.ctypes.data, lam.size,
                                              out.ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"sepaihrd_poisson_device failed ({rc}): " + err.value.decode())
        return out

    def gamma_device(self, shape, seed: int) -> np.ndarray:
        """Probe of the device's gamma sampler (sepaihrd_gamma_device): out[i] ~ Gamma(shape[i], 1) at (seed, c0 = i, c1 = c2 = 0);
        every shape finite in [1e-3, 1e6]."""
        shape = np.ascontiguousarray(shape, dtype=np.float64).ravel()
        out = np.empty(shape.size)
        err = C.create_string_buffer(512)
        rc = self.lib.sepaihrd_gamma_device(getattr(self, "_device", -1), int(seed) & 0xFFFFFFFFFFFFFFFF, shape.ctypes.data, shape.size,
                                            out.ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"sepaihrd_gamma_device failed ({rc}): " + err.value.decode())
        return out

    def nb_draw_device(self, mu, k, seed: int) -> np.ndarray:
        """Probe of the device's negative-binomial sampler (sepaihrd_nb_draw_device): out[i] ~ NB(mean mu[i], dispersion k[i]) at
        (seed, c0 = i, c1 = c2 = 0); every k +inf (Poisson) or finite in [1e-3, 1e6]."""
        mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.float64), mu.shape), dtype=np.float64).ravel()
        out = np.empty(mu.size)
        err = C.create_string_buffer(512)
        rc = self.lib.sepaihrd_nb_draw_device(getattr(self, "_device", -1), int(seed) & 0xFFFFFFFFFFFFFFFF, mu.ctypes.data, k.ctypes.data,
                                              mu.size, out.ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"sepaihrd_nb_draw_device failed ({rc}): " + err.value.decode())
        return out

    def scenario_ensemble(self, theta, kappa_mult, probs, want_sero: bool = False, want_rt: bool = False) -> dict:
        """NPI scenario analysis (sepaihrd_scenario_ensemble): every sample of theta under every row k of kappa_mult
        ([K][n_kappa], applied to kappa after the constraints) in one launch.  ppc [K][6][n_probs][T_pos][n],
        metrics [K][S][12 + 4 n], summary [K][12 + 4 n][2 + n_probs] (mean, std_dev, quantiles), diff [K][12 + 4 n][n_probs]
        (quantiles of metric[k][s] - metric[0][s]), status [K][S], n_valid [K]; sero / rt [K][n_probs][T] on request."""
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        km = np.ascontiguousarray(np.atleast_2d(kappa_mult), dtype=np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        S, K, npb, n = th.shape[0], km.shape[0], pr.size, self.pb.n
        W = 12 + 4 * n
        Tp = int(np.sum(np.asarray(self.pb.times) >= 0.0))
        ppc = np.empty((K, 6, npb, Tp, n))
        sero = np.empty((K, npb, self.pb.n_times)) if want_sero else None
        rt = np.empty((K, npb, self.pb.n_times)) if want_rt else None
        met = np.empty((K, S, W))
        summ = np.empty((K, W, 2 + npb))
        diff = np.empty((K, W, npb))
        status = np.empty((K, S), dtype=np.int32)
        nv = np.empty(K, dtype=np.int32)
        self._check(self.lib.sepaihrd_scenario_ensemble(
            self.ctx, th.ctypes.data, S, km.ctypes.data, K, km.shape[1], pr.ctypes.data, npb, ppc.ctypes.data,
            sero.ctypes.data if want_sero else None, rt.ctypes.data if want_rt else None, met.ctypes.data,
            summ.ctypes.data, diff.ctypes.data, status.ctypes.data, nv.ctypes.data), "scenario_ensemble")
        out = {"ppc": ppc, "metrics": met, "summary": summ, "diff": diff, "status": status, "n_valid": nv}
        if want_sero:
            out["sero"] = sero
        if want_rt:
            out["rt"] = rt
        return out

    def chain_diagnostics(self, samples, values=None) -> dict:
        """Convergence diagnostics on the device (sepaihrd_chain_diagnostics): samples [C][N][P], values [C][N] or None ->
        table [P + (values given)][7] (columns DIAG_COLUMNS; the values row last), max_lag [..][4] (Geyer's max_t of the raw,
        z, I[x <= q05] and I[x <= q95] series, -1 where that ESS is NaN)."""
        s = np.ascontiguousarray(samples, dtype=np.float64)
        if s.ndim != 3:
            raise ValueError("samples must be [C][N][P]")
        Cn, N, P = s.shape
        v = None if values is None else np.ascontiguousarray(np.reshape(values, (Cn, N)), dtype=np.float64)
        rows = P + (0 if v is None else 1)
        out = np.empty((rows, len(DIAG_COLUMNS)))
        lag = np.empty((rows, 4), dtype=np.int32)
        self._check(self.lib.sepaihrd_chain_diagnostics(self.ctx, s.ctypes.data, None if v is None else v.ctypes.data, Cn, N, P,
                                                        out.ctypes.data, lag.ctypes.data), "chain_diagnostics")
        return _diag_result(out, lag)

    def reserve(self, max_B: int):
        self._check(self.lib.sepaihrd_reserve(self.ctx, int(max_B)), "sepaihrd_reserve")

    def apply_constraints(self, theta, mode: int) -> np.ndarray:
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        out = np.empty_like(th)
        self._check(self.lib.sepaihrd_apply_constraints(self.ctx, mode, th.ctypes.data, th.shape[0],
                                                        out.ctypes.data), "apply_constraints")
        return out

    def device_libm_check(self):
        """(n_log_diff, n_exp_diff): arguments of the run-time self-check on which the device's log / exp restatements
        differ from this process's libm (0, 0 = the device may draw the chains' streams)."""
        a, b = C.c_int32(-1), C.c_int32(-1)
        self._check(self.lib.sepaihrd_device_libm_check(self.ctx, C.byref(a), C.byref(b)), "device_libm_check")
        return a.value, b.value

    def device_log_values(self, x) -> np.ndarray:
        """The Poisson term's log as the device evaluates it (csrc/sepaihrd_dev_common.inc log_pos), on positive normal x."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.empty_like(x)
        self._check(self.lib.sepaihrd_device_log_values(self.ctx, x.ctypes.data, x.size, out.ctypes.data), "device_log_values")
        return out

    def kernel_info(self, batch: int = 0) -> dict:
        """Resource report of the integrator kernel a launch of `batch` chains uses (0: the large-batch kernel)."""
        info = sepaihrd_kernel_info()
        self._check(self.lib.sepaihrd_get_kernel_info_for_batch(self.ctx, int(batch), C.byref(info)), "get_kernel_info")
        d = {k: getattr(info, k) for k, _ in info._fields_}
        d["kernel_name"] = info.kernel_name.decode()
        d["device_name"] = info.device_name.decode()
        return d


def build_sir_problem_struct(pb: SIRProblem, keep: list) -> sepaihrd_sir_problem:
    """Fill the C struct of the age-structured SIR objective; ``keep`` receives the arrays that must outlive the call."""
    s = sepaihrd_sir_problem()
    s.abi_version = ABI_VERSION
    s.n_age, s.n_times, s.n_params = pb.n, pb.n_times, pb.n_params
    s.solver, s.arith, s.max_attempts, s.reserved = pb.solver, pb.arith, int(pb.max_attempts), 0

    def dbl(x):
        a = np.ascontiguousarray(x, dtype=np.float64)
        keep.append(a)
        return _ptr(a, _dp)

    s.times, s.N, s.C, s.gamma = dbl(pb.times), dbl(pb.N), dbl(pb.C), dbl(pb.gamma)  # C row-major
    s.initial_state, s.obs = dbl(pb.initial_state), dbl(pb.obs)
    codes, idxs = pb.field_map()
    keep.extend([codes, idxs])
    s.param_field, s.param_index = _ptr(codes, _ip), _ptr(idxs, _ip)
    s.q, s.scale_C_total = float(pb.q), float(pb.scale_C_total)
    s.abs_err, s.rel_err, s.dt_hint = pb.abs_err, pb.rel_err, pb.dt_hint
    return s


class HipSIRObjective:
    """Batched PoissonLikelihoodObjective of the age-structured SIR model on one MI355X.  A failed chain is -inf with its
    status set (1 non-finite, 2 step failure, 3 step budget); nothing raises for a chain."""

    def __init__(self, pb: SIRProblem, device: int = -1):
        self.lib = load_library()
        self.pb = pb
        self._keep: list = []
        st = build_sir_problem_struct(pb, self._keep)
        err = C.create_string_buffer(512)
        self.ctx = self.lib.sepaihrd_sir_create(C.byref(st), device, err, len(err))
        if not self.ctx:
            raise RuntimeError("sepaihrd_sir_create failed: " + err.value.decode())
        self.P, self.n, self.T = pb.n_params, pb.n, pb.n_times

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.sepaihrd_sir_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): " + self.lib.sepaihrd_sir_last_error(self.ctx).decode())

    def getParameterNames(self):
        return list(self.pb.param_names)

    def set_arith(self, arith: int):
        self._check(self.lib.sepaihrd_sir_set_arith(self.ctx, int(arith)), "sepaihrd_sir_set_arith")

    def reserve(self, max_B: int):
        self._check(self.lib.sepaihrd_sir_reserve(self.ctx, int(max_B)), "sepaihrd_sir_reserve")

    def calculate(self, theta) -> float:
        return float(self.eval_batch(np.asarray(theta, dtype=np.float64)[None, :])["loglik"][0])

    def eval_batch(self, theta, want_traj: bool = False) -> dict:
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != self.P:
            raise ValueError(f"theta must be B x {self.P}")
        B = th.shape[0]
        out = {"loglik": np.empty(B), "status": np.empty(B, dtype=np.int32),
               "n_accept": np.empty(B, dtype=np.int32), "n_reject": np.empty(B, dtype=np.int32)}
        traj = np.empty((B, self.T, 3 * self.n)) if want_traj else None
        rc = self.lib.sepaihrd_sir_eval_batch(self.ctx, th.ctypes.data, B, out["loglik"].ctypes.data, out["status"].ctypes.data,
                                              out["n_accept"].ctypes.data, out["n_reject"].ctypes.data,
                                              traj.ctypes.data if want_traj else None)
        self._check(rc, "sepaihrd_sir_eval_batch")
        if want_traj:
            out["traj"] = traj
        return out

    def eval_batch_device(self, d_theta, d_loglik, d_status=None, d_n_accept=None, d_n_reject=None, d_traj=None,
                          stream: int = 0, B: Optional[int] = None):
        """Arguments are torch CUDA tensors (or raw device addresses); async on ``stream``."""
        def addr(t):
            if t is None:
                return None
            return t if isinstance(t, int) else t.data_ptr()
        if B is None:
            B = int(d_theta.shape[0])
        rc = self.lib.sepaihrd_sir_eval_batch_device(self.ctx, addr(d_theta), B, addr(d_loglik), addr(d_status), addr(d_n_accept),
                                                     addr(d_n_reject), addr(d_traj), stream if stream else None)
        self._check(rc, "sepaihrd_sir_eval_batch_device")

    def device_libm_check(self):
        """(n_log_diff, n_exp_diff) of the libm self-check, as HipObjective.device_libm_check."""
        a, b = C.c_int32(-1), C.c_int32(-1)
        self._check(self.lib.sepaihrd_sir_device_libm_check(self.ctx, C.byref(a), C.byref(b)), "sir_device_libm_check")
        return a.value, b.value

    def apply_constraints(self, theta) -> np.ndarray:
        th = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        out = np.empty_like(th)
        self._check(self.lib.sepaihrd_sir_apply_constraints(self.ctx, th.ctypes.data, th.shape[0], out.ctypes.data),
                    "sepaihrd_sir_apply_constraints")
        return out.reshape(np.shape(theta))

    # ---- posterior ensemble and intervention scenarios ----
    def scenario_ensemble(self, theta, scenarios, probs, want=("quantiles", "metrics", "metric_summary", "diff_quantiles", "status",
                                                               "n_accept", "n_reject", "n_valid")) -> dict:
        """sepaihrd_sir_scenario_ensemble: the S samples ``theta`` under the K ``scenarios`` (lists of (time_index, kind,
        value), see sir_event_table) in one integrator launch.  Returns the outputs named in ``want``:
        quantiles [K][3][n_probs][T][n + 1], metrics [K][S][6 + 2 n], metric_summary [K][W][2 + n_probs], diff_quantiles
        [K][W][n_probs], status / n_accept / n_reject [K][S], n_valid [K].  A failed sample is a NaN metric row with its
        status set; a refused event table raises ValueError before the device is touched."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != self.P:
            raise ValueError(f"theta must be S x {self.P}")
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        S, K, n_probs, W = th.shape[0], len(scenarios), pr.size, 6 + 2 * self.n
        tab, counts = sir_event_table(scenarios)
        shapes = {"quantiles": ((K, 3, n_probs, self.T, self.n + 1), np.float64), "metrics": ((K, S, W), np.float64),
                  "metric_summary": ((K, W, 2 + n_probs), np.float64), "diff_quantiles": ((K, W, n_probs), np.float64),
                  "status": ((K, S), np.int32), "n_accept": ((K, S), np.int32), "n_reject": ((K, S), np.int32),
                  "n_valid": ((K,), np.int32)}
        unknown = set(want) - set(shapes)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        out = {k: np.empty(shapes[k][0], dtype=shapes[k][1]) for k in shapes if k in want}
        ptr = [out[k].ctypes.data if k in out else None for k in shapes]
        rc = self.lib.sepaihrd_sir_scenario_ensemble(self.ctx, th.ctypes.data, S, tab, counts.ctypes.data, K, pr.ctypes.data, n_probs, *ptr)
        if rc == -1:
            raise ValueError(self.lib.sepaihrd_sir_last_error(self.ctx).decode())
        self._check(rc, "sepaihrd_sir_scenario_ensemble")
        return out

    def ensemble_quantiles(self, theta, probs) -> dict:
        """sepaihrd_sir_ensemble_quantiles: one scenario without events.  quantiles [3][n_probs][T][n + 1], metrics [S][W],
        metric_summary [W][2 + n_probs], status [S], n_valid."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != self.P:
            raise ValueError(f"theta must be S x {self.P}")
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        S, n_probs, W = th.shape[0], pr.size, 6 + 2 * self.n
        out = {"quantiles": np.empty((3, n_probs, self.T, self.n + 1)), "metrics": np.empty((S, W)),
               "metric_summary": np.empty((W, 2 + n_probs)), "status": np.empty(S, dtype=np.int32), "n_valid": np.empty(1, dtype=np.int32)}
        rc = self.lib.sepaihrd_sir_ensemble_quantiles(self.ctx, th.ctypes.data, S, pr.ctypes.data, n_probs, out["quantiles"].ctypes.data,
                                                      out["metrics"].ctypes.data, out["metric_summary"].ctypes.data,
                                                      out["status"].ctypes.data, out["n_valid"].ctypes.data)
        if rc == -1:
            raise ValueError(self.lib.sepaihrd_sir_last_error(self.ctx).decode())
        self._check(rc, "sepaihrd_sir_ensemble_quantiles")
        out["n_valid"] = int(out["n_valid"][0])
        return out

    def ensemble_timing(self) -> dict:
        """Calls of the two entry points above that reached the device, and the last one's device time by phase (ms)."""
        calls = C.c_int64(0)
        ms = np.zeros(3)
        self._check(self.lib.sepaihrd_sir_ensemble_timing(self.ctx, C.byref(calls), ms.ctypes.data), "sepaihrd_sir_ensemble_timing")
        return {"calls": calls.value, "integrator_ms": ms[0], "metrics_ms": ms[1], "sort_ms": ms[2]}


def stoch_sir_config(pb: StochasticSIRProblem, replicates: int, seed: int, keep: int = 0, max_workspace_bytes: Optional[int] = None,
                     abi_version: int = ABI_VERSION) -> sepaihrd_stoch_sir_config:
    return sepaihrd_stoch_sir_config(abi_version, pb.n_groups, int(replicates), int(keep), pb.t_start, pb.t_end, pb.h,
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_workspace_bytes or 0))


def stoch_sir_num_steps(t_start: float, t_end: float, h: float) -> int:
    """sepaihrd_stoch_sir_num_steps: the number of rows, or a negative code"""
    return int(load_library().sepaihrd_stoch_sir_num_steps(float(t_start), float(t_end), float(h)))


def stoch_sir_validate(pb: StochasticSIRProblem, replicates: int, keep: int = 0, abi_version: int = ABI_VERSION) -> tuple:
    """sepaihrd_stoch_sir_validate on the host (no device): (code, message)."""
    cfg = stoch_sir_config(pb, replicates, 0, keep, abi_version=abi_version)
    tab = pb.group_table()
    err = C.create_string_buffer(256)
    rc = load_library().sepaihrd_stoch_sir_validate(C.byref(cfg), tab.ctypes.data, err, len(err))
    return int(rc), err.value.decode()


def stoch_sir_outputs(pb: StochasticSIRProblem, steps: int, replicates: int, keep: int, want_final: bool) -> dict:
    G = pb.n_groups
    return {"stats": np.empty((G, 4, 3, steps)), "traj": np.empty((G, keep, 3, steps)) if keep > 0 else None,
            "final_state": np.empty((G, replicates, 3)) if want_final else None,
            "times": pb.t_start + np.arange(steps) * pb.h}


class HipStochasticSIR:
    """Chain-binomial SIR ensembles of the reference's StochasticSIRModel on one MI355X (sepaihrd_stoch_sir_run)."""

    def __init__(self, pb: StochasticSIRProblem, device: int = -1):
        self.lib = load_library()
        self.pb = pb
        self.device = int(device)
        self.phase_ms = None

    def run(self, replicates: int, seed: int, keep: int = 0, want_final: bool = False, max_workspace_bytes: Optional[int] = None) -> dict:
        """stats [G][4][3][steps] (STOCH_SIR_STATS), traj [G][keep][3][steps] or None, final_state [G][R][3] or None, times
        [steps].  Refused arguments raise ValueError before the device is touched; the device time of the call by phase
        (step kernels, sorts, summaries; ms) is left in ``phase_ms``."""
        cfg = stoch_sir_config(self.pb, replicates, seed, keep, max_workspace_bytes)
        tab = self.pb.group_table()
        err = C.create_string_buffer(512)
        if self.lib.sepaihrd_stoch_sir_validate(C.byref(cfg), tab.ctypes.data, err, len(err)) != 0:
            raise ValueError(err.value.decode())
        steps = stoch_sir_num_steps(self.pb.t_start, self.pb.t_end, self.pb.h)
        out = stoch_sir_outputs(self.pb, steps, int(replicates), int(keep), want_final)
        ms = np.zeros(3)
        rc = self.lib.sepaihrd_stoch_sir_run(self.device, C.byref(cfg), tab.ctypes.data, out["stats"].ctypes.data,
                                             None if out["traj"] is None else out["traj"].ctypes.data,
                                             None if out["final_state"] is None else out["final_state"].ctypes.data,
                                             ms.ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"sepaihrd_stoch_sir_run failed ({rc}): " + err.value.decode())
        self.phase_ms = {"step": ms[0], "sort": ms[1], "summary": ms[2]}
        return out

    def binomial(self, n, p, seed: int) -> np.ndarray:
        """sepaihrd_stoch_sir_binomial_device: out[i] ~ Binomial(n[i], p[i]) drawn by the device's sampler."""
        n = np.ascontiguousarray(n, dtype=np.int32).ravel()
        p = np.ascontiguousarray(p, dtype=np.float64).ravel()
        if n.shape != p.shape:
            raise ValueError("n and p must have one entry per draw")
        out = np.empty(n.size, dtype=np.int32)
        err = C.create_string_buffer(512)
        rc = self.lib.sepaihrd_stoch_sir_binomial_device(self.device, int(seed) & 0xFFFFFFFFFFFFFFFF, n.ctypes.data, p.ctypes.data, n.size,
                                                         out.ctypes.data, err, len(err))
        if rc != 0:
            raise RuntimeError(f"sepaihrd_stoch_sir_binomial_device failed ({rc}): " + err.value.decode())
        return out
