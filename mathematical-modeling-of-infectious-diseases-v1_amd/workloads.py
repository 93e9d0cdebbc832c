"""BASELINE.json workloads as problem builders (host plumbing for bench.py and the full-size tests).

  c1  SEPAIHRD n=4, Dopri5, 400 days (t=-20..380), 4 096 chains / GPU          (configs[1], bench default)
  c2  same model, Cash-Karp, 65 536 chains / GPU                                (configs[2])
  c3  same model, Dopri5, 32 768 chains / GPU (262 144 over 8 GPUs)             (configs[3])
  c5  n=16 synthetic (bands split 4 ways, M16 = M4/4), Dopri5, 1 000 days, 32 768 chains / GPU   (configs[4])

Observations of c5 are drawn once from the base-theta trajectory computed by the HIP path itself
(trajectory mode) with numpy's RandomState(12345), i.e. SURVEY.md 8(d)'s recipe without touching the oracle.
"""
from __future__ import annotations

import os

import numpy as np

from .problem import SEPAIHRDProblem, StochasticSIRProblem, widen_age_classes, SOLVER_DOPRI5, SOLVER_CASH_KARP54

DEFAULT_CHAINS = {"c1": 4096, "c2": 65536, "c3": 32768, "c5": 32768}


def _incidence(traj: np.ndarray, n: int, comp: int, runup_offset: int) -> np.ndarray:
    cum = traj[:, comp * n:(comp + 1) * n]
    inc = np.maximum(np.diff(cum, axis=0, prepend=cum[:1]), 0.0)
    return inc[runup_offset:]


def with_synthetic_observations(pb: SEPAIHRDProblem, hip_factory, seed: int = 12345) -> SEPAIHRDProblem:
    """obs = Poisson(model incidence at base theta); the trajectory comes from the device."""
    T_obs = pb.n_times - pb.runup_offset
    blank = pb.with_(obs_H=np.zeros((T_obs, pb.n)), obs_ICU=np.zeros((T_obs, pb.n)), obs_D=np.zeros((T_obs, pb.n)))
    blank.base_theta = pb.base_theta
    hip = hip_factory(blank)
    traj = hip.eval_batch(pb.base_theta[None, :], want_traj=True)["traj"][0]
    hip.close()
    rs = np.random.RandomState(seed)
    obs = {name: rs.poisson(_incidence(traj, pb.n, comp, pb.runup_offset)).astype(np.float64)
           for name, comp in (("obs_H", 9), ("obs_ICU", 10), ("obs_D", 8))}
    out = blank.with_(**obs)
    out.base_theta = pb.base_theta
    return out


def build(name: str, golden_dir: str, hip_factory=None) -> SEPAIHRDProblem:
    if name in ("c1", "c2", "c3"):
        pb = SEPAIHRDProblem.load(os.path.join(golden_dir, "synth_400d_n4.json"))
        pb.solver = SOLVER_CASH_KARP54 if name == "c2" else SOLVER_DOPRI5
        return pb
    if name == "c5":
        base = SEPAIHRDProblem.load(os.path.join(golden_dir, "shipped_problem.json"))
        wide = widen_age_classes(base, 4)
        wide = wide.with_(times=np.arange(-20, 981, dtype=np.float64))
        wide.base_theta = widen_age_classes(base, 4).base_theta
        wide.solver = SOLVER_DOPRI5
        if hip_factory is None:
            raise ValueError("workload c5 needs a device to draw its synthetic observations")
        return with_synthetic_observations(wide, hip_factory)
    raise ValueError(f"unknown workload {name}")


# ---------------------------------------------------------------------------------------------------------------
# Age-structured SIR: BASELINE configs[0]'s problem with synthetic observations
# ---------------------------------------------------------------------------------------------------------------
SIR_TRUE_THETA = (0.03, 1.0, 0.2, 0.2, 0.15)  # q, scale_C_total, gamma_0..2
SIR_ALL_NAMES = ("q", "scale_C_total", "gamma_0", "gamma_1", "gamma_2")


def sir_incidence(pb, traj, values=None) -> np.ndarray:
    """SimulationResultProcessor::getIncidenceData on a trajectory [T][3n]: max(q ((C scale) (I / N)), 0) * S."""
    v = values or {"q": pb.q, "scale_C_total": pb.scale_C_total}
    n = pb.n
    ion = np.where(pb.N > 1e-9, traj[:, n:2 * n] / np.where(pb.N > 1e-9, pb.N, 1.0), 0.0)
    lam = np.maximum(v["q"] * (ion @ (pb.C * v["scale_C_total"]).T), 0.0)
    return lam * traj[:, :n]


def sir_config0(simulate, param_names=SIR_ALL_NAMES, seed: int = 20240229, **kw):
    """configs[0]'s three-age SIR problem (N, C, gamma, q = 0.03, I0 = 10 / 20 / 5, days 0..200) with observations drawn
    once, with a fixed seed, as Poisson counts of the true incidence.  ``simulate(N, C, gamma, q, scale, init, times)``
    returns {"traj": [T][3n]} of the true parameters (the tests pass the CPU oracle's sir_simulate; tools pass a device
    evaluation): the package itself holds no integrator."""
    from .problem import SIRProblem
    N = np.array([5.0e5, 1.2e6, 3.0e5])
    Cm = np.array([[8.0, 3.0, 1.0], [3.0, 6.0, 2.0], [1.0, 2.0, 3.0]])
    gamma = np.array([0.2, 0.2, 0.15])
    I0 = np.array([10.0, 20.0, 5.0])
    init = np.concatenate([N - I0, I0, np.zeros(3)])
    times = np.arange(0.0, 201.0)
    pb = SIRProblem(N=N, C=Cm, gamma=gamma, q=0.03, scale_C_total=1.0, initial_state=init, times=times,
                    obs=np.zeros((len(times), 3)), param_names=list(param_names), **kw)
    traj = np.asarray(simulate(N, Cm, gamma, 0.03, 1.0, init, times)["traj"]).reshape(len(times), 9)
    rng = np.random.default_rng(seed)
    return pb.with_(obs=rng.poisson(sir_incidence(pb, traj)).astype(np.float64))


def sir_scenario_reference(simulate, pb, theta, scenarios, probs) -> dict:
    """The semantics of sepaihrd_sir_scenario_ensemble restated in numpy around a caller-supplied
    ``simulate(N, C, gamma, q, scale, init, times, abs_err, rel_err)`` -> {"traj": [T'][3n], "n_accept", "n_reject"} that
    raises when a run fails (the package holds no integrator).  ``scenarios``: lists of (time_index, kind, value), kind 0 /
    "contact" (scale <- scale * value) or 1 / "transmission" (q <- q * (1 - value)), sorted by time_index.

    An event at grid index k splits the run: the segment before it ends at times[k], whose row (state and incidence)
    is formed with the old parameters; the next segment is a fresh ``simulate`` call on times[k:] from that state with the
    new ones, C_current = C * scale_now.  Events at index 0 precede the first observation.  Step counts are summed over
    the segments; a sample whose summed attempts exceed pb.max_attempts (0: 1 000 000) has status 3, as a chain that is still
    running after that many attempts has on the device.  Quantiles: np.quantile(method="linear") over the samples valid in that scenario, NaN when there is none;
    R0 = max |eigvals| of K_ij = q scale C_ij N_i / (N_j gamma_j), columns with N_j <= 1e-9 dropped, gamma_j = 0: +inf.
    Returns the outputs of HipSIRObjective.scenario_ensemble plus "series" [K][S][3][T][n + 1]."""
    kinds = {"contact": 0, "transmission": 1}
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    probs = np.asarray(probs, dtype=np.float64)
    K, S, n, T = len(scenarios), theta.shape[0], pb.n, pb.n_times
    W = 6 + 2 * n
    series = np.full((K, S, 3, T, n + 1), np.nan)
    metrics = np.full((K, S, W), np.nan)
    status = np.zeros((K, S), dtype=np.int32)
    n_acc = np.zeros((K, S), dtype=np.int32)
    n_rej = np.zeros((K, S), dtype=np.int32)
    S0 = pb.initial_state[:n]
    has_pop = pb.N > 1e-9

    def incidence(rows, q, scale):
        ion = np.where(has_pop, rows[:, n:2 * n] / np.where(has_pop, pb.N, 1.0), 0.0)
        return np.maximum(q * (ion @ (pb.C * scale).T), 0.0) * rows[:, :n]

    def total(a):  # ages added in ascending order
        tot = np.zeros(a.shape[:-1])
        for i in range(a.shape[-1]):
            tot = tot + a[..., i]
        return tot

    for s in range(S):
        v = pb.model_values(theta[s])
        # R0 from the sample's own parameters, before any event
        if np.any(has_pop & (v["gamma"] == 0.0)):
            r0 = np.inf
        else:
            col = np.where(has_pop, 1.0 / np.where(has_pop, pb.N * v["gamma"], 1.0), 0.0)
            r0 = float(np.max(np.abs(np.linalg.eigvals(v["q"] * v["scale_C_total"] * pb.C * pb.N[:, None] * col[None, :]))))
        for k, sc in enumerate(scenarios):
            events = [(int(ti), int(kinds.get(kind, kind)), float(val)) for ti, kind, val in sc]
            q, scale = v["q"], v["scale_C_total"]

            def apply(at, q, scale):
                for ti, kind, val in events:
                    if ti == at:
                        if kind == 0:
                            scale = scale * val
                        else:
                            q = q * (1.0 - val)
                return q, scale

            q, scale = apply(0, q, scale)
            cuts = sorted({ti for ti, _, _ in events if 0 < ti < T - 1}) + [T - 1]
            traj = np.empty((T, 3 * n))
            inc = np.empty((T, n))
            x, k0 = pb.initial_state, 0
            try:
                for k1 in cuts:
                    r = simulate(pb.N, pb.C, v["gamma"], q, scale, x, pb.times[k0:k1 + 1], pb.abs_err, pb.rel_err)
                    seg = np.asarray(r["traj"]).reshape(k1 - k0 + 1, 3 * n)
                    first = 0 if k0 == 0 else 1  # row k0 was formed by the segment that ended there
                    traj[k0 + first:k1 + 1] = seg[first:]
                    inc[k0 + first:k1 + 1] = incidence(seg[first:], q, scale)
                    n_acc[k, s] += r.get("n_accept", 0)
                    n_rej[k, s] += r.get("n_reject", 0)
                    x, k0 = seg[-1], k1
                    q, scale = apply(k1, q, scale)
                if T == 1:
                    traj[0] = pb.initial_state
                    inc[0] = incidence(traj[:1], q, scale)[0]
            except RuntimeError:
                status[k, s] = 2
                continue
            if int(n_acc[k, s]) + int(n_rej[k, s]) > (pb.max_attempts if pb.max_attempts > 0 else 1000000):
                status[k, s] = 3
                continue
            if not np.all(np.isfinite(inc)):
                status[k, s] = 1
                continue
            for ser, a in enumerate((inc, traj[:, n:2 * n], S0[None, :] - traj[:, :n])):
                series[k, s, ser, :, :n] = a
                series[k, s, ser, :, n] = total(a)
            tp, ti_ = series[k, s, 1, :, n], series[k, s, 0, :, n]
            m = metrics[k, s]
            m[0] = r0
            m[1], m[2] = tp.max(), pb.times[int(np.argmax(tp))]
            m[3], m[4] = ti_.max(), pb.times[int(np.argmax(ti_))]
            tot_pop = 0.0
            for i in range(n):
                tot_pop = tot_pop + pb.N[i]
            m[5] = series[k, s, 2, T - 1, n] / tot_pop
            last = series[k, s, 2, T - 1, :n]
            m[6::2] = np.where(pb.N > 0, last / np.where(pb.N > 0, pb.N, 1.0), 0.0)
            m[7::2] = series[k, s, 1, :, :n].max(axis=0)

    def q_of(a):  # a [n_valid][...] -> [n_probs][...]
        if a.shape[0] == 0:
            return np.full((len(probs),) + a.shape[1:], np.nan)
        return np.quantile(a, probs, axis=0, method="linear")

    quantiles = np.empty((K, 3, len(probs), T, n + 1))
    summary = np.empty((K, W, 2 + len(probs)))
    diff = np.empty((K, W, len(probs)))
    n_valid = np.zeros(K, dtype=np.int32)
    for k in range(K):
        ok = status[k] == 0
        n_valid[k] = ok.sum()
        quantiles[k] = np.moveaxis(q_of(series[k, ok]), 0, 1)  # [n_probs][3][T][n+1] -> [3][n_probs][T][n+1]
        mv = metrics[k, ok]
        if mv.shape[0]:  # (an infinite R0 gives an infinite mean and NaN below it, as on the device)
            mean = mv.sum(axis=0) / mv.shape[0]
            summary[k, :, 0] = mean
            summary[k, :, 1] = np.sqrt(((mv - mean) ** 2).sum(axis=0) / mv.shape[0])
        else:
            summary[k, :, :2] = np.nan
        summary[k, :, 2:] = q_of(mv).T
        both = ok & (status[0] == 0)
        diff[k] = q_of(metrics[k, both] - metrics[0, both]).T
    return {"quantiles": quantiles, "metrics": metrics, "metric_summary": summary, "diff_quantiles": diff, "status": status,
            "n_accept": n_acc, "n_reject": n_rej, "n_valid": n_valid, "series": series}


def stochastic_sir_reference(golden_dir: str = None, **kw):
    """The workload of the reference's stochastic SIR driver (tests/golden/stochastic_sir_reference_input.json: its
    input_parameters.txt with h = 1/24): (problem, fixture dict).  Keyword arguments replace fields of the problem."""
    import json
    if golden_dir is None:
        golden_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    with open(os.path.join(golden_dir, "stochastic_sir_reference_input.json")) as fh:
        fx = json.load(fh)
    fields = {k: fx[k] for k in ("N", "beta", "gamma", "S0", "I0", "R0", "t_start", "t_end", "h")}
    fields.update(kw)
    return StochasticSIRProblem(**fields), fx
