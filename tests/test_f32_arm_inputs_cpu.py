"""Can the inputs of tests/test_gpu_f32_arm.py see what they are meant to see?  Oracle only, no GPU.

The fp32 arm (csrc/sepaihrd_kernels_f32.hip) has no bit contract, so its GPU tests rest on bars.  A bar only means something
if the fault it is meant to catch moves the answer by much more than the bar: each test here applies such a fault to the
PROBLEM (two columns of the contact matrix swapped = a contact sum reading the wrong lane; every schedule breakpoint moved
to the next one = a schedule cache one refresh late) and requires the oracle's trajectory to move by at least 10 x the
state bar used on the device.  The rest pins the conditions the edge cases of the GPU file rely on (attempt budgets on the
right side of the oracle's counts, expected statuses, mates that do what their names say).
"""
import itertools

import numpy as np
import pytest

import f32_arm_cases as fc


def _traj(oracle_py, pb, theta):
    return oracle_py.Oracle(pb).eval_batch(theta, want_traj=True)


@pytest.mark.parametrize("n", fc.LANE_COUNTS)
def test_every_column_transposition_moves_the_trajectory(mm, oracle_py, n):
    """A: minimum over all transpositions (a, b) of two columns of M of the largest state error over the batch, against
    10 x the state bar.  Measured with this recipe: n = 5: 0.67, 8: 8.1e-2, 9: 0.27, 15: 3.6e-2, 16: 2.2e-2."""
    pb = fc.lane_problem(mm, n)
    theta = fc.lane_batch(mm, pb)
    assert theta.shape[0] % (64 // fc.lanes_per_chain(n)) != 0          # ragged last wave
    ref = _traj(oracle_py, pb, theta)
    assert np.all(ref["status"] == 0)
    assert len({tuple(col) for col in pb.M.T}) == n                     # column-distinct
    worst = np.inf
    for a, b in itertools.combinations(range(n), 2):
        moved = _traj(oracle_py, fc.swap_columns(pb, a, b), theta)
        worst = min(worst, fc.rel_state_err(moved["traj"], ref["traj"]).max())
    print(f"n={n} minimum over transpositions {worst:.3g}")
    assert worst >= 10 * fc.STATE_BAR, worst


@pytest.mark.parametrize("f", [2, 4])
def test_replicated_age_classes_hide_a_column_swap(mm, oracle_py, f):
    """Why A exists: on widen_age_classes alone, swapping two columns inside a replicated block changes nothing at all."""
    from mmid_amd import draws
    pb = mm.widen_age_classes(fc.load(mm, "shipped_problem.json"), f)
    pb = fc.cut_grid(pb, pb.times[:40])
    theta = draws.jitter_draws(pb, 3, 3)
    ref = _traj(oracle_py, pb, theta)
    for a, b in ((0, 1), (f, f + 1)):
        assert np.array_equal(_traj(oracle_py, fc.swap_columns(pb, a, b), theta)["traj"], ref["traj"])


@pytest.mark.parametrize("lpc", [4, 8, 16])
def test_big_batch_shape(mm, oracle_py, lpc):
    """B: 1025 workgroups, the last one with one chain; the 64 distinct chains all run; a swapped column is still seen on
    the short grid."""
    pb = fc.big_problem(mm, lpc)
    tile, B = fc.big_batch(mm, pb)
    cpw = 64 // lpc
    assert pb.n == lpc and pb.n_times == 12 and pb.n_obs == pb.n_times - pb.runup_offset == 5
    assert (B + cpw - 1) // cpw == 1025 and B % cpw == 1 and B % 64 == 1
    assert len({tuple(t) for t in tile}) == 64
    ref = _traj(oracle_py, pb, tile)
    assert np.all(ref["status"] == 0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("lpc", [4, 8, 16])
def test_company_is_what_it_says(mm, oracle_py, lpc, mode):
    """C: the mates fail at once / reject more / are moved by the constraint rule, and the target sits first, mid-wave and
    last in a ragged wave."""
    pb = fc.company_problem(mm, lpc, mode)
    target, batch, pos = fc.company_batch(mm, pb)
    cpw = 64 // lpc
    assert pos[0] % cpw == 0 and 0 < pos[1] % cpw < cpw - 1 + (cpw == 4) and pos[2] == len(batch) - 1 and len(batch) % cpw != 0
    assert all(np.array_equal(batch[p], target) for p in pos)
    ref = oracle_py.Oracle(pb).eval_batch(batch)
    alone = oracle_py.Oracle(pb).eval_batch(target[None, :])
    others = [b for b in range(len(batch)) if b not in pos]
    assert alone["status"][0] == 0
    assert (ref["status"][others] == 1).any() and (ref["status"][others] == 0).sum() >= 4
    assert ref["n_reject"][others].max() > alone["n_reject"][0]
    lo, hi, _ = pb.bounds_arrays()
    assert ((batch[others] < lo) | (batch[others] > hi)).any(axis=1).sum() >= 2
    steps = ref["n_accept"][others] + ref["n_reject"][others]
    assert len(set(steps[ref["status"][others] == 0].tolist())) >= 3     # the mates' step sequences differ


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("n", [4, 16])
def test_late_schedule_moves_the_trajectory(mm, oracle_py, n, solver):
    """D: 65 segments of beta kappa (the largest schedule the C ABI takes), breakpoints on and between grid times, two inside
    the first step, one factor jumping by 2 x at each; every breakpoint moved to the next one moves the trajectory by at least
    10 x the state bar."""
    pb = fc.schedule_problem(mm, n).with_(solver=solver)
    ends = fc.merged_end_times(pb)
    assert len(ends) == len(pb.beta_end_times) + len(pb.kappa_end_times) == 64           # 65 segments, none shared
    assert np.sum(ends < pb.dt_hint) == 2
    on_grid = np.isin(ends, pb.times)
    assert on_grid.sum() >= 4 and (~on_grid).sum() >= 55
    for vals in (pb.beta_values, pb.kappa_values):
        ratio = vals[1:] / vals[:-1]
        assert np.all(np.maximum(ratio, 1 / ratio) >= 2.0)
    theta = fc.schedule_batch(pb)
    ref = _traj(oracle_py, pb, theta)
    assert np.all(ref["status"] == 0)
    late = _traj(oracle_py, fc.shift_breakpoints(pb), theta)
    moved = fc.rel_state_err(late["traj"], ref["traj"]).max(axis=(1, 2))
    print(f"n={n} solver={solver} late schedule moves the states by {moved.min():.3g} .. {moved.max():.3g}")
    assert moved.min() >= 10 * fc.STATE_BAR, moved


def test_no_schedule_problem_runs(mm, oracle_py):
    pb = fc.no_schedule_problem(mm)
    ref = oracle_py.Oracle(pb).eval_batch(fc.NO_SCHEDULE_THETA)
    assert np.all(ref["status"] == 0) and np.ptp(ref["loglik"]) > 0


def test_sentinel_cases_have_the_oracles_statuses(mm, oracle_py):
    for name, (pb, theta, want) in fc.sentinel_cases(mm).items():
        ref = oracle_py.Oracle(pb).eval_batch(theta)
        assert ref["status"].tolist() == want, name
        assert np.all(ref["loglik"][np.array(want) == 1] == -np.finfo(np.float64).max), name


@pytest.mark.parametrize("solver", [0, 1])
def test_attempt_budgets_are_far_from_the_oracles_counts(mm, oracle_py, solver):
    """E: the short budget is at most half the smallest attempt count, the ample one at least twice the largest: the fp32
    step counts differ from these by a few, never by a factor of two."""
    pb = fc.budget_problem(mm).with_(solver=solver)
    ref = oracle_py.Oracle(pb).eval_batch(fc.budget_batch(pb))
    attempts = ref["n_accept"] + ref["n_reject"]
    assert np.all(ref["status"] == 0)
    assert 2 * fc.BUDGET_SHORT <= attempts.min() and fc.BUDGET_AMPLE >= 2 * attempts.max(), (attempts.min(), attempts.max())
    orc = oracle_py.Oracle(pb)
    orc.set_max_attempts(fc.BUDGET_SHORT)
    assert np.all(orc.eval_batch(fc.budget_batch(pb))["status"] == 3)


def test_observation_problem_skips_what_it_should(mm, oracle_py):
    pb = fc.observation_problem(mm)
    theta = fc.fixture_batch(pb, 9, 71)
    ref = oracle_py.Oracle(pb).eval_batch(theta)
    assert np.all(ref["status"] == 0) and np.all(np.isfinite(ref["loglik"]))
    assert np.all(ref["ll_parts"][:, 2] == 0.0) and np.all(ref["ll_parts"][:, :2] != 0.0)


def test_negative_increments_reach_every_stream(mm, oracle_py):
    """E: the oracle runs the chains that start below zero, and every stream sees negative daily increments (which it clamps)."""
    pb, theta = fc.negative_increment_case(mm)
    ref = _traj(oracle_py, pb, theta)
    assert np.all(ref["status"] == 0) and np.all(np.isfinite(ref["loglik"]))
    n = pb.n
    negative = [(np.diff(ref["traj"][1:, :, c * n:(c + 1) * n], axis=1) < -0.01).sum() for c in (8, 9, 10)]
    assert min(negative) >= 5, negative
    assert not (np.diff(ref["traj"][0, :, 8 * n:], axis=0) < 0).any()
    # the reference's own error at this tolerance: small on chains 0-2, 4.3e-4 on the chain with I and H both below zero -- a
    # bar on the distance from THIS reference cannot be tighter than that for chain 3 (the GPU file's group "E-")
    fine = _traj(oracle_py, pb.with_(abs_err=1e-12, rel_err=1e-12), theta)
    own = fc.rel_state_err(ref["traj"], fine["traj"]).max(axis=(1, 2))
    print("oracle at 1e-6 against itself at 1e-12:", own)
    assert own[:3].max() < 1e-4 and 2e-4 < own[3] < 1e-3


def test_init_modes_are_three_different_runs(mm):
    """E: the three initial-state modes must be told apart by the test: the problem's stored state, that state times the
    multipliers, and the seeded state differ."""
    pb = fc.init_mode_problem(mm)
    n = pb.n
    x = pb.initial_state.reshape(11, n)
    assert pb.runup_days > 0 and pb.seed_exposed > 0
    assert np.abs(x[1:9]).sum() > 0 and not np.allclose(pb.multipliers, 1.0)


@pytest.mark.parametrize("scale", [1e-3, 40.0])
def test_extreme_beta_runs_in_the_oracle(mm, oracle_py, scale):
    pb, theta = fc.extreme_beta_case(mm, scale)
    ref = _traj(oracle_py, pb, theta)
    assert ref["status"][0] == 0
    n = pb.n
    if scale > 1:
        assert ref["traj"][0, -1, :n].min() < 0.05 * pb.N.min()            # S runs out
