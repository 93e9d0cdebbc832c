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

from .problem import SEPAIHRDProblem, widen_age_classes, SOLVER_DOPRI5, SOLVER_CASH_KARP54

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
