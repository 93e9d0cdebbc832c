"""Every instantiation of the age-structured SIR kernel against a step-for-step reference: the seven lane widths, the three
steppers and both arithmetics of sepaihrd_sir_eval_kernel<LPC, SOLVER, ARITH>, and the same 42 of the ensemble build.

Problems, parameter batches and the reference come from tests/test_sir_variants_cpu.py (variant_problem, variant_theta,
compared_chains, case_reference): n in {1, 2, 3, 7, 13, 16, 17, 33, 64} covers every LPC with padded and exact age counts,
n = 16 with strict Fehlberg 7(8) is the sixteen-lane kernel whose contact rows sit in LDS, the uneven output grid makes the
controller grow and reject, one age class is empty (N = 0) and one starts without infected.  Dopri5 is held to the oracle's own
run, Cash-Karp and Fehlberg to the plain-float integrate_times driver of tests/test_gpu_fehlberg78.py over the oracle's
right-hand side.  That file's CPU tests show that the driver converges on this model, that the compared chains take different
paths through the controller, and that EVAL_CASES / ENSEMBLE_CASES below reach every instantiation.

Bars: strict -- tests/test_gpu_sir.py's check_strict (status 0, step counts identical, states within 1e-9 of max(|ref|, 1),
log-likelihood within 1e-10 sum|terms|); fma -- test_fma_within_north_star_tolerance's (states 1e-6, likelihood 1e-7
sum|terms|, step counts equal on more than 0.9 of the compared chains); the ensemble build -- bit for bit against eval_batch
without events, tests/test_gpu_sir_ensemble.py's check_strict with events.  At most 12 chains per case meet the reference;
every other chain is held to them by evaluating the batch in reversed order and demanding the same bits per point."""
import numpy as np
import pytest

from test_gpu_sir import REL_STATE_BAR, check_strict
from test_gpu_sir_ensemble import check_strict as check_strict_ensemble
from test_sir_variants_cpu import (ARITHS, EMPTY_AGE, EVENT_SCENARIOS, FMA_CHAINS, NS, PROBS, SOLVERS, batch_size, case_reference,
                                   lanes_per_chain, scenario_reference, variant_problem, variant_theta)

pytestmark = pytest.mark.gpu

# (n, solver, arith) of the evaluation kernels (sections 1 and 2) and of the ensemble build (section 4);
# tests/test_sir_variants_cpu.py asserts that each list reaches all 42 (LPC, SOLVER, ARITH) and both row placements per solver
EVAL_CASES = [(n, solver, arith) for n in NS for solver in SOLVERS for arith in ARITHS]
ENSEMBLE_CASES = list(EVAL_CASES)
TIGHT_CASES = [(n, solver) for n in (2, 17, 64) for solver in SOLVERS]
EVENT_CASES = [(n, solver) for n in (17, 64) for solver in ("cash_karp", "fehlberg78")]
LDS_ROW_SHAPES_CASE = (16, "fehlberg78", "strict")
LDS_ROW_SHAPES_CASE_TRIPLE = (lanes_per_chain(16), SOLVERS["fehlberg78"], ARITHS["strict"])


def _of(cases, arith):
    return [(n, solver) for n, solver, a in cases if a == arith]


def pick(got, idx):
    return {k: v[idx] for k, v in got.items()}


def strict_against_the_reference(mm, oracle_py, n, solver, tol):
    B = batch_size(n)
    pb, theta, idx, ref = case_reference(mm, oracle_py, n, solver, B, tol)
    hip = mm.HipSIRObjective(pb)
    got = hip.eval_batch(theta, want_traj=True)
    assert np.all(got["status"] == 0), np.flatnonzero(got["status"])
    check_strict(pick(got, idx), ref, f"n = {n} {solver} strict tol {tol:g}, {len(idx)} of {B} chains")
    if n > EMPTY_AGE:
        assert np.all(got["traj"][:, :, EMPTY_AGE::n] == 0.0)  # the empty age class: every row exactly 0
    assert np.array_equal(hip.eval_batch(theta)["loglik"], got["loglik"])  # the likelihood-only launch
    rev = hip.eval_batch(theta[::-1], want_traj=True)  # every chain in another lane group, wavefront and partial wavefront
    for k in ("loglik", "status", "n_accept", "n_reject", "traj"):
        assert np.array_equal(rev[k][::-1], got[k]), k
    hip.close()
    return got


# ---------------------------------------------------------------- 1. strict against the reference
@pytest.mark.parametrize("n, solver", _of(EVAL_CASES, "strict"))
def test_strict_against_the_reference(mm, oracle_py, n, solver):
    strict_against_the_reference(mm, oracle_py, n, solver, 1e-6)


# ---------------------------------------------------------------- 2. fma, the same cases, at 65 chains
@pytest.mark.parametrize("n, solver", _of(EVAL_CASES, "fma"))
def test_fma_within_north_star_tolerance(mm, oracle_py, n, solver):
    pb, theta, idx, ref = case_reference(mm, oracle_py, n, solver, FMA_CHAINS)
    hip = mm.HipSIRObjective(pb.with_(arith=mm.ARITH_FMA))
    full = hip.eval_batch(theta, want_traj=True)
    assert np.all(full["status"] == 0)
    got = pick(full, idx)
    rel = np.abs(got["traj"] - ref["traj"]) / np.maximum(np.abs(ref["traj"]), 1.0)
    ll_err = np.abs(got["loglik"] - ref["loglik"]) / ref["scale"]
    same = np.mean((got["n_accept"] == ref["n_accept"]) & (got["n_reject"] == ref["n_reject"]))
    print(f"n = {n} {solver} fma: max rel state err {rel.max():.3g}, max |dll| / sum|terms| {ll_err.max():.3g}, "
          f"same step counts {same:.3f} of {len(idx)} chains")
    assert rel.max() < REL_STATE_BAR and ll_err.max() < 1e-7 and same > 0.9, (rel.max(), ll_err.max(), same)
    if n > EMPTY_AGE:
        assert np.all(full["traj"][:, :, EMPTY_AGE::n] == 0.0)
    rev = hip.eval_batch(theta[::-1])
    for k in ("loglik", "status", "n_accept", "n_reject"):
        assert np.array_equal(rev[k][::-1], full[k]), k
    # set_arith switches the same context: the strict kernel's bits, and its bars, on the batch of section 1
    pb1, theta1, idx1, ref1 = case_reference(mm, oracle_py, n, solver, batch_size(n))
    hip.set_arith(mm.ARITH_STRICT)
    back = hip.eval_batch(theta1, want_traj=True)
    hip.close()
    check_strict(pick(back, idx1), ref1, f"n = {n} {solver} set_arith(strict)")
    fresh = mm.HipSIRObjective(pb1)
    want = fresh.eval_batch(theta1, want_traj=True)
    fresh.close()
    for k in ("loglik", "status", "n_accept", "n_reject", "traj"):
        assert np.array_equal(back[k], want[k]), k


# ---------------------------------------------------------------- 3. tight tolerance
@pytest.mark.parametrize("n, solver", TIGHT_CASES)
def test_strict_at_tight_tolerance(mm, oracle_py, n, solver):
    """abs = rel = 1e-9: three to four times the steps, the decrease exponent and the floors act more often"""
    strict_against_the_reference(mm, oracle_py, n, solver, 1e-9)


# ---------------------------------------------------------------- 4. the ensemble build
@pytest.mark.parametrize("n, solver, arith", ENSEMBLE_CASES)
def test_empty_scenario_is_eval_batch_bit_for_bit(mm, oracle_py, n, solver, arith):
    """Series 1 (a copy of I) and 2 (S(t0) - S(t), one subtraction) of one scenario without events against eval_batch's
    trajectories, as tests/test_gpu_sir_ensemble.py's test of that name: step counts, the extremes over the samples
    (probabilities 0 and 1 pick single order statistics), every value of three single-sample calls, every sample's per-age
    peak prevalence."""
    pb = variant_problem(mm, oracle_py, n, solver, arith)
    theta = variant_theta(pb, batch_size(n))
    hip = mm.HipSIRObjective(pb)
    ev = hip.eval_batch(theta, want_traj=True)
    assert np.all(ev["status"] == 0)
    S_, I_ = ev["traj"][:, :, 0:n], ev["traj"][:, :, n:2 * n]
    cum = pb.initial_state[None, None, 0:n] - S_
    got = hip.scenario_ensemble(theta, [[]], [0.0, 1.0])
    assert np.all(got["status"] == 0)
    assert np.array_equal(got["n_accept"][0], ev["n_accept"]) and np.array_equal(got["n_reject"][0], ev["n_reject"])
    q = got["quantiles"][0]
    assert np.array_equal(q[1, 0, :, :n], I_.min(axis=0)) and np.array_equal(q[1, 1, :, :n], I_.max(axis=0))
    assert np.array_equal(q[2, 0, :, :n], cum.min(axis=0)) and np.array_equal(q[2, 1, :, :n], cum.max(axis=0))
    assert np.array_equal(got["metrics"][0][:, 7::2], I_.max(axis=1))
    for s in (0, len(theta) // 2, len(theta) - 1):
        one = hip.scenario_ensemble(theta[s:s + 1], [[]], [0.5], want=("quantiles",))["quantiles"][0]
        assert np.array_equal(one[1, 0, :, :n], I_[s]) and np.array_equal(one[2, 0, :, :n], cum[s])
    hip.close()


@pytest.mark.parametrize("n, solver", EVENT_CASES)
def test_events_restart_the_integrator_inside_an_lds_row_kernel(mm, oracle_py, n, solver):
    """A contact event and a transmission event against workloads.sir_scenario_reference driven by the plain-float driver:
    each event re-forms the rows in LDS and restarts the integrator with dt = dt_hint."""
    pb, theta, ref = scenario_reference(mm, oracle_py, n, solver)
    assert np.all(ref["status"] == 0)
    hip = mm.HipSIRObjective(pb)
    got = hip.scenario_ensemble(theta, EVENT_SCENARIOS, PROBS)
    hip.close()
    check_strict_ensemble(got, ref, f"n = {n} {solver}, {len(theta)} samples x {len(EVENT_SCENARIOS)} scenarios")
    assert np.any(got["n_accept"][1] != got["n_accept"][0])  # the events do something


# ---------------------------------------------------------------- 5. batch shapes of one LDS-row case
@pytest.mark.parametrize("B", [1, 5, 4099])
def test_lds_row_kernel_batch_shapes_give_bit_identical_values_per_repeated_point(mm, oracle_py, B):
    n, solver, arith = LDS_ROW_SHAPES_CASE
    pb = variant_problem(mm, oracle_py, n, solver, arith)
    base = variant_theta(pb, batch_size(n))
    hip = mm.HipSIRObjective(pb)
    ref = hip.eval_batch(base)
    idx = np.arange(B) % len(base)
    got = hip.eval_batch(base[idx])
    hip.close()
    assert np.all(got["status"] == 0)
    assert np.array_equal(got["loglik"], ref["loglik"][idx])
    assert np.array_equal(got["n_accept"], ref["n_accept"][idx]) and np.array_equal(got["n_reject"], ref["n_reject"][idx])
