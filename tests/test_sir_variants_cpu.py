"""Every instantiation of the age-structured SIR kernel (sepaihrd_sir_eval_kernel<LPC, SOLVER, ARITH> and its ensemble
build), the parts that need no GPU: the problems and parameter batches of tests/test_gpu_sir_variants.py, their
step-for-step reference, and the conditions on those inputs that make the GPU comparison mean something.

Reference: Dopri5 is the oracle's own run (oracle_py.sir_simulate); Cash-Karp 5(4) and Fehlberg 7(8) are
tests/test_gpu_fehlberg78.py's plain-float restatement of integrate_times over a controlled generic explicit RK
(integrate_times, CASH_KARP, FEHLBERG78) driven by the oracle's SIR right-hand side.  The likelihood is formed from the
reference trajectory as tests/test_gpu_sir.py's oracle_eval forms it.

Checked here: (1) the driver with both tableaus converges to SciPy DOP853 on this model; (2) the inputs make the
controller grow and reject, differently per chain; (3) the GPU file's case list reaches every (LPC, SOLVER, ARITH) the
launcher can pick and both placements of the contact rows per solver; (4) what a case's reference costs."""
import functools
import os
import re
import time

import numpy as np
import pytest

from test_gpu_fehlberg78 import CASH_KARP, FEHLBERG78, integrate_times
from test_gpu_sir import oracle_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIR_SOURCE = os.path.join(ROOT, "mathematical-modeling-of-infectious-diseases-v1_amd", "csrc", "sepaihrd_sir.hip")

WAVE = 64
NS = [1, 2, 3, 7, 13, 16, 17, 33, 64]
SOLVERS = {"dopri5": 0, "cash_karp": 1, "fehlberg78": 2}  # SEPAIHRD_SOLVER_*
ARITHS = {"strict": 0, "fma": 1}                          # SEPAIHRD_ARITH_*
TABLEAUS = {"cash_karp": CASH_KARP, "fehlberg78": FEHLBERG78}
# uneven; the first interval is shorter than dt_hint; the long intervals let the controller grow and reject
GRID = np.array([0.0, 0.5, 3.0, 10.0, 25.0, 45.0, 80.0, 120.0, 121.0, 200.0])
EMPTY_AGE = 2        # n >= 3: N = 0 and S = I = R = 0 (has_pop == false, I / N forced to 0)
NEGATIVE_OBS = (3, 0)  # (row, age) of an observation below 0, clipped by max(obs, 0)
MAX_COMPARED = 12
FMA_CHAINS = 65
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
# grid indices 3 (t = 10) and 5 (t = 45): each event restarts the integrator
EVENT_SCENARIOS = [[], [(3, "contact", 0.6), (5, "transmission", 0.3)]]


def lanes_per_chain(n):
    lpc = 1
    while lpc < n:
        lpc *= 2
    return lpc


def batch_size(n):
    """two full wavefronts and a partial one, at least 9 chains"""
    return max(2 * (WAVE // lanes_per_chain(n)) + 1, 9)


def no_seed_age(n):
    """the age class that starts without infected (n >= 3)"""
    return 4 % n


@functools.lru_cache(maxsize=None)
def _base_problem(mm, oracle_py, n):
    rng = np.random.default_rng(7 + n)
    N = rng.uniform(2e5, 1.5e6, n)
    Cm = rng.uniform(0.2, 1.0, (n, n)) * 12.0 / n
    gamma = rng.uniform(0.15, 0.25, n)
    I0 = np.round(rng.uniform(5, 25, n))
    q = 0.03
    if n >= 3:
        N[EMPTY_AGE] = 0.0
        I0[EMPTY_AGE] = 0.0
        I0[no_seed_age(n)] = 0.0
    # R0 = 2: the spectral radius of K_ij = q C_ij N_i / (N_j gamma_j) over the populated classes
    pop = N > 1e-9
    K = q * Cm[np.ix_(pop, pop)] * N[pop][:, None] / (N[pop] * gamma[pop])[None, :]
    Cm = Cm * (2.0 / np.max(np.abs(np.linalg.eigvals(K))))
    init = np.concatenate([N - I0, I0, np.zeros(n)])
    names = ["q", "scale_C_total"] + [f"gamma_{i}" for i in range(n)]
    pb = mm.SIRProblem(N=N, C=Cm, gamma=gamma, q=q, scale_C_total=1.0, initial_state=init, times=GRID.copy(),
                       obs=np.zeros((len(GRID), n)), param_names=names)
    traj = oracle_py.sir_simulate(N, Cm, gamma, q, 1.0, init, GRID)["traj"]
    obs = rng.poisson(mm.workloads.sir_incidence(pb, traj)).astype(np.float64)
    obs[NEGATIVE_OBS] = -3.0
    obs[5, n - 1] = 0.0
    return pb.with_(obs=obs)


def variant_problem(mm, oracle_py, n, solver, arith, abs_err=1e-6, rel_err=1e-6):
    """n age classes on GRID, a fixed-seed contact matrix scaled to R0 = 2, Poisson observations of the true incidence with
    one negative and one zero cell; for n >= 3 age class 2 is empty and age class 4 mod n starts without infected"""
    code = SOLVERS[solver] if isinstance(solver, str) else int(solver)
    ar = ARITHS[arith] if isinstance(arith, str) else int(arith)
    return _base_problem(mm, oracle_py, n).with_(solver=code, arith=ar, abs_err=abs_err, rel_err=rel_err)


def variant_theta(pb, B):
    """B - 1 rows: current parameters x exp(N(0, 0.3)) on q and scale_C_total, x exp(N(0, 0.2)) on each gamma_i; the last
    row is the unperturbed vector"""
    rng = np.random.default_rng(1000 + pb.n)
    sd = np.where(np.arange(pb.n_params) < 2, 0.3, 0.2)
    th = pb.current_parameters() * np.exp(rng.normal(0.0, 1.0, size=(B - 1, pb.n_params)) * sd)
    return np.vstack([th, pb.current_parameters()])


def compared_chains(B, n):
    """at most 12 chains: the first and the last chain of every wavefront, the last row of theta, the rest spread evenly"""
    cpw = WAVE // lanes_per_chain(n)
    ends = {B - 1}
    for first in range(0, B, cpw):
        ends.update((first, min(first + cpw, B) - 1))
    if len(ends) > MAX_COMPARED:  # more wavefronts than chains to compare: the ends of the batch, the rest spread evenly
        ends = {0, B - 1}
    rest = [b for b in range(B) if b not in ends]
    room = min(MAX_COMPARED - len(ends), len(rest))
    if room > 0:
        ends.update(rest[int(i)] for i in np.linspace(0, len(rest) - 1, room).round())
    return np.array(sorted(ends))


def driver_simulate(oracle_py, tab, dt_hint=1.0):
    """simulate(N, C, gamma, q, scale, init, times, abs_err, rel_err) of workloads.sir_scenario_reference over the plain-float
    driver; raises when the run fails"""
    def simulate(N, Cm, gamma, q, scale, init, times, abs_err=1e-6, rel_err=1e-6):
        rows, acc, rej, status = integrate_times(tab, lambda x, t: oracle_py.sir_rhs(N, Cm, gamma, q, scale, x), init,
                                                 [float(t) for t in times], dt_hint, abs_err, rel_err)
        if status != 0:
            raise RuntimeError(f"integrate_times failed ({status})")
        return {"traj": np.array(rows), "n_accept": acc, "n_reject": rej}
    return simulate


def simulator(oracle_py, pb):
    """the reference run of pb's stepper"""
    name = {v: k for k, v in SOLVERS.items()}[pb.solver]
    return oracle_py.sir_simulate if name == "dopri5" else driver_simulate(oracle_py, TABLEAUS[name], pb.dt_hint)


def reference_eval(oracle_py, mm, pb, theta):
    """oracle_eval of tests/test_gpu_sir.py with the stepper's own reference run: per chain the trajectory, step counts,
    likelihood and sum|terms| at the constrained point"""
    out = {"traj": [], "n_accept": [], "n_reject": [], "loglik": [], "scale": []}
    obs = np.maximum(pb.obs, 0.0)
    simulate = simulator(oracle_py, pb)
    for th in theta:
        v = pb.model_values(th)
        r = simulate(pb.N, pb.C, v["gamma"], v["q"], v["scale_C_total"], pb.initial_state, pb.times, pb.abs_err, pb.rel_err)
        inc = np.maximum(mm.workloads.sir_incidence(pb, r["traj"], v), 1e-9)
        terms = obs * np.log(inc) - inc
        out["traj"].append(r["traj"]); out["n_accept"].append(r["n_accept"]); out["n_reject"].append(r["n_reject"])
        out["loglik"].append(terms.sum()); out["scale"].append(np.abs(terms).sum())
    return {k: np.array(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case_reference(mm, oracle_py, n, solver, B, tol=1e-6):
    """(problem, theta [B], compared chain indices, their reference), computed once per session; arithmetic plays no part in
    the reference"""
    pb = variant_problem(mm, oracle_py, n, solver, "strict", tol, tol)
    theta = variant_theta(pb, B)
    idx = compared_chains(B, n)
    return pb, theta, idx, reference_eval(oracle_py, mm, pb, theta[idx])


@functools.lru_cache(maxsize=None)
def scenario_reference(mm, oracle_py, n, solver):
    """(problem, samples, workloads.sir_scenario_reference of EVENT_SCENARIOS over the plain-float driver)"""
    pb = variant_problem(mm, oracle_py, n, solver, "strict")
    theta = variant_theta(pb, batch_size(n))
    return pb, theta, mm.workloads.sir_scenario_reference(simulator(oracle_py, pb), pb, theta, EVENT_SCENARIOS, PROBS)


# ---------------------------------------------------------------- the helpers themselves
@pytest.mark.parametrize("n", NS)
def test_the_problem_has_the_edges_it_promises(mm, oracle_py, n):
    pb = variant_problem(mm, oracle_py, n, "fehlberg78", "fma", 1e-9, 1e-9)
    assert (pb.solver, pb.arith, pb.abs_err, pb.rel_err, pb.dt_hint) == (mm.SOLVER_FEHLBERG78, mm.ARITH_FMA, 1e-9, 1e-9, 1.0)
    assert np.array_equal(pb.times, GRID) and pb.times[1] - pb.times[0] < pb.dt_hint
    if n >= 3:
        assert pb.N[EMPTY_AGE] == 0.0 and np.all(pb.initial_state[EMPTY_AGE::n] == 0.0)
        assert pb.initial_state[n + no_seed_age(n)] == 0.0 and pb.N[no_seed_age(n)] > 0
    assert pb.obs[NEGATIVE_OBS] < 0 and pb.obs[5, n - 1] == 0.0 and np.all(np.isfinite(pb.obs))
    assert np.maximum(pb.obs, 0.0).max() > 100  # an epidemic, not noise
    B = batch_size(n)
    cpw = WAVE // lanes_per_chain(n)
    assert B >= 9 and B >= 2 * cpw + 1 and (cpw == 1 or B % cpw != 0)  # two full wavefronts and a partial one
    theta = variant_theta(pb, B)
    assert theta.shape == (B, n + 2) and np.array_equal(theta[-1], pb.current_parameters())
    assert np.array_equal(pb.apply_constraints(theta), theta)  # positive: the constrained point is the point
    for size in (B, FMA_CHAINS):
        idx = compared_chains(size, n)
        assert len(idx) <= MAX_COMPARED and len(set(idx.tolist())) == len(idx) and size - 1 in idx and 0 in idx
        assert idx.min() >= 0 and idx.max() < size
        if (size + cpw - 1) // cpw * 2 <= MAX_COMPARED:  # every wavefront's two ends fit
            for first in range(0, size, cpw):
                assert first in idx and min(first + cpw, size) - 1 in idx


def test_dopri5_reference_is_oracle_eval(mm, oracle_py):
    pb, theta, idx, ref = case_reference(mm, oracle_py, 7, "dopri5", batch_size(7))
    want = oracle_eval(oracle_py, mm, pb, theta[idx])
    for k in want:
        assert np.array_equal(ref[k], want[k]), k
    assert np.all(np.isfinite(ref["traj"])) and np.all(np.isfinite(ref["loglik"]))
    assert np.all(ref["traj"][:, :, EMPTY_AGE::7] == 0.0)


# ---------------------------------------------------------------- 1. the driver on this model
@pytest.mark.parametrize("n", [3, 17, 64])
def test_driver_converges_to_the_independent_answer(mm, oracle_py, n):
    """Both tableaus at abs = rel = 1e-11 against SciPy DOP853 (rtol 1e-12, atol 1e-9, interval by interval over the grid),
    within ten times the error of the oracle's Dopri5 run at 1e-11 against the same answer (the rule of
    tests/test_gpu_sir.py: the three methods' error constants differ, their controller is the same)."""
    from scipy.integrate import solve_ivp
    pb = variant_problem(mm, oracle_py, n, "dopri5", "strict", 1e-11, 1e-11)
    args = (pb.N, pb.C, pb.gamma, pb.q, pb.scale_C_total)
    ans = [pb.initial_state.copy()]
    for k in range(1, len(GRID)):
        sol = solve_ivp(lambda t, x: oracle_py.sir_rhs(*args, x), (GRID[k - 1], GRID[k]), ans[-1], method="DOP853", rtol=1e-12, atol=1e-9)
        assert sol.success
        ans.append(sol.y[:, -1])
    ans = np.array(ans)

    def err(traj):
        return float(np.max(np.abs(traj - ans) / np.maximum(np.abs(ans), 1.0)))
    oracle_tight = err(oracle_py.sir_simulate(*args, pb.initial_state, GRID, 1e-11, 1e-11)["traj"])
    assert oracle_tight < 1e-8
    for name, tab in TABLEAUS.items():
        r = driver_simulate(oracle_py, tab, pb.dt_hint)(*args, pb.initial_state, GRID, 1e-11, 1e-11)
        e = err(r["traj"])
        print(f"n = {n} {name}: error {e:.3g} (bar {10.0 * oracle_tight:.3g}; oracle Dopri5 at 1e-11: {oracle_tight:.3g}), "
              f"steps {r['n_accept']} + {r['n_reject']}")
        assert e < 10.0 * oracle_tight, (n, name, e, oracle_tight)


# ---------------------------------------------------------------- 2. the inputs exercise the controller
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("n", NS)
def test_compared_chains_take_different_paths_through_the_controller(mm, oracle_py, n, solver):
    """A condition on the inputs, checked without the kernel: a batch whose chains all take the same steps would let a
    controller that is wrong for the others pass."""
    pb, theta, idx, ref = case_reference(mm, oracle_py, n, solver, batch_size(n))
    pairs = set(zip(ref["n_accept"].tolist(), ref["n_reject"].tolist()))
    print(f"n = {n} {solver}: accepted {ref['n_accept'].min()}..{ref['n_accept'].max()}, rejected "
          f"{ref['n_reject'].min()}..{ref['n_reject'].max()}, {len(pairs)} distinct pairs over {len(idx)} chains")
    assert np.all(np.isfinite(ref["traj"])) and np.all(np.isfinite(ref["loglik"]))
    assert len(pairs) >= 3
    assert ref["n_reject"].max() >= 1
    assert ref["n_accept"].min() > len(GRID) - 1  # more than one step per interval somewhere: the controller, not the grid


@pytest.mark.parametrize("solver", ["cash_karp", "fehlberg78"])
@pytest.mark.parametrize("n", [17, 64])
def test_the_event_scenario_runs_and_hides_no_argmax_ties(mm, oracle_py, n, solver):
    """The GPU test holds peak TIMES equal to the reference's, which means something only if no sample's largest row is
    within the state bar of its runner-up (tests/test_sir_ensemble_cpu.py has the argument)."""
    from test_sir_ensemble_cpu import peak_gaps
    pb, theta, ref = scenario_reference(mm, oracle_py, n, solver)
    assert np.all(ref["status"] == 0) and np.all(np.isfinite(ref["quantiles"]))
    assert np.any(ref["n_accept"][1] != ref["n_accept"][0])
    assert np.all(ref["metrics"][1, :, 5] < ref["metrics"][0, :, 5])  # the events lower every sample's attack rate
    gaps = peak_gaps(ref["series"])
    print(f"n = {n} {solver}: smallest relative gap between the peak row and its runner-up {gaps.min():.3g}")
    assert gaps.min() >= 1e-6


# ---------------------------------------------------------------- 3. the parameter grid is complete
def _switch_labels(text, head):
    """the case labels of the first `switch (head) { ... }` after each occurrence of its head; all occurrences must agree"""
    found = []
    for m in re.finditer(r"switch \(%s\) \{(.*?)\n\s*default:" % re.escape(head), text, re.S):
        found.append(sorted(int(c) for c in re.findall(r"case (\d+):", m.group(1))))
    assert found and all(f == found[0] for f in found), (head, found)
    return found[0]


def _rows_in_lds_rule(text):
    """sir_rows_in_lds(lpc, solver) of the source as a Python function of (lpc, solver, arith_fma)"""
    m = re.search(r"constexpr bool sir_rows_in_lds\(int lpc, int solver\) \{ return (.*?); \}", text)
    assert m, "sir_rows_in_lds has changed its form: restate it here"
    expr = m.group(1).replace("||", " or ").replace("&&", " and ").replace("SEPAIHRD_ARITH_FMA", "arith")
    assert re.fullmatch(r"[\w\s()<>=]+", expr), expr
    return lambda lpc, solver, arith: bool(eval(expr, {"__builtins__": {}}, {"lpc": lpc, "solver": solver, "arith": arith}))


def test_the_gpu_cases_reach_every_instantiation_and_both_row_placements():
    import test_gpu_sir_variants as gpu
    text = open(SIR_SOURCE).read()
    lpcs = _switch_labels(text, "pb.lpc")
    solvers = _switch_labels(text, "solver")
    # one translation unit per arithmetic, each with its own entry point
    ariths = sorted(ARITHS[a] for a in set(re.findall(r"^int launch_sir_eval_(\w+)\(", text, re.M)))
    assert ariths == [0, 1] and ariths == sorted(ARITHS[a] for a in set(re.findall(r"^int launch_sir_ens_(\w+)\(", text, re.M)))
    want = {(l, s, a) for l in lpcs for s in solvers for a in ariths}
    assert len(want) == 42, (lpcs, solvers, ariths)
    rows_in_lds = _rows_in_lds_rule(text)

    def triples(cases):
        return {(lanes_per_chain(n), SOLVERS[solver], ARITHS[arith]) for n, solver, arith in cases}
    for name in ("EVAL_CASES", "ENSEMBLE_CASES"):  # the evaluation kernels and the ensemble build: 42 each
        got = triples(getattr(gpu, name))
        assert want - got == set(), (name, sorted(want - got))
        for s in solvers:
            placements = {rows_in_lds(l, s2, a) for l, s2, a in got if s2 == s}
            assert placements == {False, True}, (name, s, placements)
    # the special case at sixteen lanes: strict Fehlberg alone
    assert [t for t in sorted(want) if t[0] == 16 and rows_in_lds(*t)] == [(16, SOLVERS["fehlberg78"], ARITHS["strict"])]
    assert rows_in_lds(*gpu.LDS_ROW_SHAPES_CASE_TRIPLE) and gpu.LDS_ROW_SHAPES_CASE_TRIPLE[0] == 16


# ---------------------------------------------------------------- 4. what the reference costs
def test_reference_of_one_case_is_cheap(mm, oracle_py):
    """about 12 chains x 10 rows; printed, not asserted"""
    for n, solver in ((2, "cash_karp"), (17, "fehlberg78"), (64, "fehlberg78")):
        pb = variant_problem(mm, oracle_py, n, solver, "strict")
        theta = variant_theta(pb, FMA_CHAINS)
        idx = compared_chains(FMA_CHAINS, n)
        t0 = time.perf_counter()
        ref = reference_eval(oracle_py, mm, pb, theta[idx])
        print(f"n = {n} {solver}: reference of {len(idx)} chains in {time.perf_counter() - t0:.2f} s")
        assert ref["traj"].shape == (len(idx), len(GRID), 3 * n)
