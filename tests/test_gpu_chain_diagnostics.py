"""Convergence diagnostics on the device (sepaihrd_chain_diagnostics / sepaihrd_mh_diagnostics) against the numpy
restatement of the same definitions (mmid_amd.diagnostics: posterior's split R-hat, bulk / tail ESS)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1


def _ar1(rng, C, N, phi):
    e = rng.standard_normal((C, N))
    x = np.empty((C, N))
    x[:, 0] = e[:, 0] / math.sqrt(1 - phi * phi)
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return x


def _columns(C, N, seed):
    """iid, AR(1) 0.9, heavily tied (rounded to 0.1), constant, NaN-bearing, one shifted chain; values iid."""
    rng = np.random.default_rng(seed)
    cols = [rng.standard_normal((C, N)), _ar1(rng, C, N, 0.9) * 2.0 + 5.0, np.round(rng.standard_normal((C, N)), 1),
            np.full((C, N), 0.75)]
    nan = rng.standard_normal((C, N))
    nan[C // 2, N // 3] = np.nan
    shifted = rng.standard_normal((C, N))
    if C > 1:
        shifted[C - 1] += 2.0
    else:
        shifted[0, N // 2:] += 2.0
    cols += [nan, shifted]
    return np.stack(cols, axis=2), rng.standard_normal((C, N)) - 300.0


def _assert_agrees(got, want):
    g, w = got["table"], want["table"]
    assert g.shape == w.shape
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    ok = ~np.isnan(w)
    rel = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
    assert np.all(rel[:, :2][ok[:, :2]] <= 1e-12), rel[:, :2]
    assert np.all(rel[:, 2:][ok[:, 2:]] <= 1e-9), rel[:, 2:]
    assert np.array_equal(got["max_lag"], want["max_lag"]), (got["max_lag"], want["max_lag"])


@pytest.fixture(scope="module")
def hip(mm):
    return mm.HipObjective(mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json")))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 5, 6, 101, 1000])
@pytest.mark.parametrize("C", [1, 4, 37])
def test_device_agrees_with_the_restatement(mm, hip, C, N):
    s, v = _columns(C, N, seed=100 * C + N)
    got = hip.chain_diagnostics(s, v)
    _assert_agrees(got, mm.diagnostics.chain_diagnostics(s, v))
    assert got["table"].shape == (7, 7) and np.all(np.isnan(got["table"][3])) and np.all(np.isnan(got["table"][4]))
    if N == 1000 and C > 1:
        # one chain shifted by 2 sd: flagged among 4 chains, and above iid's R-hat among 37
        assert got["table"][5, 6] > (1.1 if C == 4 else got["table"][0, 6]) and got["table"][0, 6] < 1.01


@pytest.mark.gpu
def test_a_million_draws_per_column(mm, hip):
    rng = np.random.default_rng(9)
    C, N = 1024, 1024
    s = np.stack([rng.standard_normal((C, N)), _ar1(rng, C, N, 0.9), np.round(rng.standard_normal((C, N)), 1)], axis=2)
    v = _ar1(rng, C, N, 0.5)
    _assert_agrees(hip.chain_diagnostics(s, v), mm.diagnostics.chain_diagnostics(s, v))


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(mm, hip):
    s, v = _columns(37, 1000, seed=4)
    a, b = hip.chain_diagnostics(s, v), hip.chain_diagnostics(s, v)
    assert a["table"].tobytes() == b["table"].tobytes() and np.array_equal(a["max_lag"], b["max_lag"])
    # without the values column the parameter rows are unchanged
    c = hip.chain_diagnostics(s)
    assert c["table"].tobytes() == a["table"][:-1].tobytes()


@pytest.mark.gpu
def test_resident_path_equals_the_read_back_samples(mm, oracle_py, shipped, hip):
    pb = shipped.with_(arith=mm.ARITH_FMA, constraint_mode=1)
    C = 8
    x0 = oracle_py.Oracle(pb).jitter_draws(pb.base_theta, 3, C, mode=1)
    kw = dict(seed=19, iterations=400, burn_in=100, adaptation_period=50, thinning=5)
    host_off = mm.HostObjective(pb)
    off = host_off.metropolis_hastings(x0, device_state=True, **kw)
    assert host_off.mh_diagnostics() is None
    host = mm.HostObjective(pb)
    host.set_mh_diagnostics(True)
    on = host.metropolis_hastings(x0, device_state=True, **kw)
    for key in ("samples", "sample_values", "accept_trace", "accepted", "best_value"):
        assert np.array_equal(on[key], off[key]), key
    table = host.mh_diagnostics()
    first = kw["burn_in"] // kw["thinning"] + 1
    ref = hip.chain_diagnostics(on["samples"][:, first:, :], on["sample_values"][:, first:])
    assert table.shape == (pb.n_params + 1, 7)
    assert table.tobytes() == ref["table"].tobytes()
    assert np.all(np.isfinite(table[:, 6]))
    # the C++ class over host draws (host_chain_diagnostics) is the same computation
    via_host = host.chain_diagnostics(on["samples"][:, first:, :], on["sample_values"][:, first:])
    assert via_host["table"].tobytes() == ref["table"].tobytes()


@pytest.mark.gpu
def test_refusals(mm, hip):
    lib, ctx = hip.lib, hip.ctx
    out = np.empty((8, 7))
    lag = np.empty((8, 4), dtype=np.int32)
    s = np.zeros(64 * 4)

    def chain(C, N, P, values=None):
        return lib.sepaihrd_chain_diagnostics(ctx, s.ctypes.data, values, C, N, P, out.ctypes.data, lag.ctypes.data)

    assert chain(0, 8, 1) == INVALID_ARG
    assert chain(2, 8, 0) == INVALID_ARG
    assert chain(2, 3, 1) == INVALID_ARG
    assert chain(1 << 16, 1 << 15, 1) == INVALID_ARG and b"2^31" in lib.sepaihrd_last_error(ctx)
    theta = np.tile(hip.pb.base_theta, (2, 1))
    assert lib.sepaihrd_eval_batch_begin(ctx, np.ascontiguousarray(theta).ctypes.data, 2) == 0
    assert chain(2, 8, 1) == INVALID_ARG and b"pending" in lib.sepaihrd_last_error(ctx)
    ll = np.empty(2)
    assert lib.sepaihrd_eval_batch_end(ctx, ll.ctypes.data, None, None, None, None) == 0
    assert chain(2, 8, 1) == 0

    P = hip.P
    x0 = np.tile(hip.pb.base_theta, (2, 1))
    cov0 = np.eye(P) * 1e-6
    out = np.empty((P + 1, 7))
    lag = np.empty((P + 1, 4), dtype=np.int32)
    mh0 = mm.hipabi.mh_create(lib, ctx, 2, 10, x0, cov0, thinning=0)
    try:
        assert lib.sepaihrd_mh_diagnostics(mh0, 0, 0, 0, out.ctypes.data, lag.ctypes.data) == INVALID_ARG
        assert b"stores no samples" in lib.sepaihrd_last_error(ctx)
    finally:
        lib.sepaihrd_mh_destroy(mh0)
    mh = mm.hipabi.mh_create(lib, ctx, 2, 10, x0, cov0, thinning=1)
    try:
        assert lib.sepaihrd_mh_diagnostics(mh, 0, 0, 1, out.ctypes.data, lag.ctypes.data) == INVALID_ARG
        assert b"no values stored" in lib.sepaihrd_last_error(ctx)
        assert lib.sepaihrd_mh_diagnostics(mh, 0, 5, 0, out.ctypes.data, lag.ctypes.data) == INVALID_ARG
        assert b"beyond" in lib.sepaihrd_last_error(ctx)
        assert lib.sepaihrd_mh_diagnostics(mh, 0, 0, 0, out.ctypes.data, lag.ctypes.data) == INVALID_ARG  # one sample: N < 4
        assert lib.sepaihrd_eval_batch_begin(ctx, np.ascontiguousarray(theta).ctypes.data, 2) == 0
        assert lib.sepaihrd_mh_diagnostics(mh, 0, 0, 0, out.ctypes.data, lag.ctypes.data) == INVALID_ARG
        assert b"pending" in lib.sepaihrd_last_error(ctx)
        assert lib.sepaihrd_eval_batch_end(ctx, ll.ctypes.data, None, None, None, None) == 0
    finally:
        lib.sepaihrd_mh_destroy(mh)


@pytest.mark.gpu
def test_calibration_driver_writes_the_diagnostics(tmp_path):
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_calibration.py"), "--out", str(out), "--chains", "4",
                        "--hc-iterations", "6", "--hc-threads", "4", "--cloud-size-multiplier", "2", "--mcmc-iterations", "200",
                        "--burn-in", "60", "--adaptation-period", "40", "--thinning", "4", "--diagnostics"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    lines = open(out / "parameter_posteriors" / "posterior_diagnostics.csv").read().splitlines()
    assert lines[0] == "parameter,mean,sd,mcse_mean,ess_mean,ess_bulk,ess_tail,r_hat"
    assert len(lines) == 1 + 62 + 1 and lines[-1].startswith("log_likelihood,")
    vals = np.array([[float(c) for c in ln.split(",")[1:]] for ln in lines[1:]])
    # every row finite except, in a run this short, ess_tail of a parameter whose upper draws repeat one value (chains that
    # rejected in a row): then I[x <= q95] is 1 everywhere, and posterior's should_return_NA makes that ESS NaN
    assert np.all(np.isfinite(np.delete(vals, 5, axis=1))) and np.all(np.isfinite(vals[-1]))
    assert np.isfinite(vals[:, 5]).sum() >= 50
    assert summary["max_r_hat"] == pytest.approx(vals[:, 6].max()) and summary["min_ess_bulk"] == pytest.approx(vals[:, 4].min())
    assert summary["min_ess_tail"] == pytest.approx(np.nanmin(vals[:, 5]))
