"""Lock-step No-U-Turn chains on the device: sepaihrd_fd_gradient_batch against the one-vector finite-difference
objective, MultiChainNUTSSampler against HipNUTSSampler chain by chain and against the oracle, and its output as the
input of the convergence diagnostics.  Fixture: the reference test fixture plus two calibrated initial-state multipliers
(n = 4, 30 output days, P = 7), as in tests/test_gpu_host_mirror.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NUTS_KW = dict(iterations=10, adaptation_window=4, max_tree_depth=3)
PER_CHAIN = ("samples", "sample_values", "epsilon_trace", "depth_trace", "best", "best_value", "gradient_calls")


def _multiplier_fixture(mm):
    """reference test fixture + calibrated E0 / I0 multipliers (the finite-difference objective reads them)."""
    pb = mm.SEPAIHRDProblem.load(os.path.join(GOLDEN, "reference_test_fixture.json"))
    names = list(pb.param_names) + ["E0_multiplier", "I0_multiplier"]
    sig = dict(pb.sigmas); sig.update(E0_multiplier=0.05, I0_multiplier=0.05)
    bnd = dict(pb.bounds); bnd.update(E0_multiplier=(0.5, 1.2), I0_multiplier=(0.1, 3.0))
    theta = np.concatenate([np.asarray(pb.base_theta), [1.2, 0.8]])  # E0 multiplier AT its upper bound
    return pb.with_(param_names=names, sigmas=sig, bounds=bnd, base_theta=theta, arith=mm.ARITH_STRICT, constraint_mode=0)


def _inside_start(pb):
    """the existing NUTS test's starting point: the fixture's theta with the E0 multiplier inside its bounds"""
    th = np.asarray(pb.base_theta).copy()
    th[-2] = 1.0
    return th


def _jittered(base, count, seed):
    """starts one percent around `base`, well inside every bound of the fixture"""
    rng = np.random.default_rng(seed)
    return base * (1.0 + 0.01 * rng.standard_normal((count, base.size)))


def _arith(mm, name):
    return mm.ARITH_STRICT if name == "strict" else mm.ARITH_FMA


@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_fd_gradient_batch_equals_the_single_vector_objective(mm, oracle_py, arith):
    pb = _multiplier_fixture(mm).with_(arith=_arith(mm, arith))
    inside = _inside_start(pb)
    rows = np.vstack([inside, _jittered(inside, 3, 1), np.asarray(pb.base_theta)])  # last row: E0 + eps leaves its bound
    assert rows.shape == (5, 7) and rows[4, 5] == pb.bounds["E0_multiplier"][1]
    hip = mm.HipObjective(pb)
    got = hip.fd_gradient_batch(rows)
    host = mm.HostObjective(pb)
    for c in range(5):
        v, g = host.evaluate_with_gradient(rows[c])
        print(arith, "row", c, "value", got["value"][c], v, "max |grad diff|", np.abs(got["grad"][c] - g).max())
        assert got["value"][c] == v and np.array_equal(got["grad"][c], g), c
    assert np.all(got["status"] <= 1) and np.all(np.isfinite(got["grad"])) and np.count_nonzero(got["grad"]) >= 20
    if arith == "strict":  # tolerances of test_finite_difference_gradient_objective
        orc = oracle_py.Oracle(pb)
        for c in range(5):
            ref_v, ref_g = orc.evaluate_with_gradient(rows[c])
            np.testing.assert_allclose(got["value"][c], ref_v, rtol=1e-11)
            scale = np.abs(ref_v) * 1e-10 / (1e-4 * np.maximum(np.abs(rows[c]), 1e-4))
            assert np.all(np.abs(got["grad"][c] - ref_g) <= np.maximum(1e-6 * np.abs(ref_g), scale)), (c, got["grad"][c], ref_g)
    # a mask: the same values, the unwanted rows of the gradient left as they were
    mask = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    kept = np.full((5, 7), 123.0)
    part = hip.fd_gradient_batch(rows, want_grad=mask, grad=kept)
    assert np.array_equal(part["value"], got["value"])
    assert np.array_equal(kept[mask == 1], got["grad"][mask == 1]) and np.all(kept[mask == 0] == 123.0)
    none = hip.fd_gradient_batch(rows, want_grad=np.zeros(5, dtype=np.uint8))
    assert np.array_equal(none["value"], got["value"]) and np.all(np.isnan(none["grad"]))


@pytest.mark.parametrize("arith", ["strict", "fma"])
def test_lock_step_chains_equal_solo_runs_and_the_oracle(mm, oracle_py, arith):
    """forms of one arithmetic are bit-identical whatever the batch -- so a chain whose gradients were
    rows of a batch takes, bit for bit, the path it takes alone."""
    pb = _multiplier_fixture(mm)
    pb = pb.with_(base_theta=_inside_start(pb), constraint_mode=1, arith=_arith(mm, arith))
    starts = _jittered(np.asarray(pb.base_theta), 5, 2)
    lock = mm.HostObjective(pb).nuts_chains(starts, 3, **NUTS_KW)
    assert np.all(lock["failure_status"] == 0) and np.all(lock["n_samples"] == 10)
    assert lock["depth_trace"].max() >= 2 and lock["rows_total"] == lock["rows_evaluated"].sum()
    assert lock["ticks"] <= 1.2 * lock["rows_evaluated"].max()
    for c in range(5):
        solo = mm.HostObjective(pb).nuts(starts[c], 3 + c, **NUTS_KW)
        for k in PER_CHAIN:
            print(arith, "chain", c, k, "equal" if np.array_equal(lock[k][c], solo[k]) else "DIFFERENT")
        for k in PER_CHAIN:
            assert np.array_equal(lock[k][c], solo[k]), (c, k)
        assert lock["rows_evaluated"][c] <= 0.45 * lock["gradient_calls"][c] + 10  # the memory serves the repeats (+ value rows)
        if arith == "strict":
            ref = oracle_py.Oracle(pb).nuts(starts[c], 3 + c, **NUTS_KW)
            assert np.array_equal(lock["depth_trace"][c], ref["depth_trace"])
            np.testing.assert_allclose(lock["epsilon_trace"][c], ref["epsilon_trace"], rtol=1e-6)
            np.testing.assert_allclose(lock["samples"][c], ref["samples"], rtol=1e-6, atol=1e-9)
            np.testing.assert_allclose(lock["sample_values"][c], ref["sample_values"], rtol=1e-6)
            assert lock["gradient_calls"][c] == ref["gradient_calls"]


def test_chains_feed_the_convergence_diagnostics(mm):
    """R-hat across chains needs more than one chain: before the lock-step sampler no NUTS output had any."""
    pb = _multiplier_fixture(mm)
    pb = pb.with_(base_theta=_inside_start(pb), constraint_mode=1)
    host = mm.HostObjective(pb)
    run = host.nuts_chains(_jittered(np.asarray(pb.base_theta), 4, 5), 11, iterations=40, adaptation_window=10, max_tree_depth=3)
    assert np.all(run["n_samples"] == 40)
    diag = host.chain_diagnostics(run["samples"], run["sample_values"])
    assert diag["table"].shape == (7 + 1, 7) and diag["max_lag"].shape == (7 + 1, 4)
    assert np.all(np.isfinite(diag["table"])), diag["table"]


def test_six_hundred_chains_cross_the_launch_form_boundary(mm):
    """600 chains x 7 parameters = 4200 perturbed rows, past the 4096 chains at which the evaluator changes its launch
    form: chains from both ends and the middle still equal their solo runs."""
    pb = _multiplier_fixture(mm)
    pb = pb.with_(base_theta=_inside_start(pb), constraint_mode=1)
    starts = _jittered(np.asarray(pb.base_theta), 600, 7)
    kw = dict(iterations=3, adaptation_window=2, max_tree_depth=2)
    lock = mm.HostObjective(pb).nuts_chains(starts, 100, **kw)
    assert np.all(lock["failure_status"] == 0) and np.all(lock["n_samples"] == 3)
    assert lock["ticks"] <= 1.2 * lock["rows_evaluated"].max()  # the first tick carries all 600 chains: 4200 perturbed rows
    for c in (0, 299, 599):
        solo = mm.HostObjective(pb).nuts(starts[c], 100 + c, **kw)
        for k in PER_CHAIN:
            assert np.array_equal(lock[k][c], solo[k]), (c, k)
