"""Stochastic chain-binomial SIR ensembles on the device (sepaihrd_stoch_sir_run): bit-identity with the host twin, the two
sort paths, independence of a replicate's path from everything but its coordinates, the sampler probe and the distribution
of what the device draws."""
import ctypes as C
import math

import numpy as np
import pytest

from test_stoch_sir_cpu import BINOM_N, BINOM_P, check_summaries, chi_square_against_binomial

pytestmark = pytest.mark.gpu


def six_groups(mm, steps):
    """the reference workload at h = 1; both probabilities large, the rejection regime, near the int limit; a fractional
    start; beta = 0; gamma = 0; I0 = 0"""
    return mm.StochasticSIRProblem(N=[1000.0, 2e9, 100.5, 1000.0, 1000.0, 1000.0], beta=[0.4, 3.0, 0.9, 0.0, 0.4, 0.4],
                                   gamma=[0.04, 2.0, 0.2, 0.04, 0.0, 0.04], S0=[999.0, 1.9e9, 90.25, 900.0, 999.0, 1000.0],
                                   I0=[1.0, 1e8, 10.25, 100.0, 1.0, 0.0], R0=0.0, t_start=0.0,
                                   t_end=float(steps - 1) if steps > 1 else 0.25, h=1.0)


def assert_same(got, want):
    for k in ("stats", "traj", "final_state"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("steps", [1, 25])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 200])
def test_device_equals_twin_bit_for_bit(mm, R, steps):
    pb = six_groups(mm, steps)
    got = mm.HipStochasticSIR(pb, device=0).run(R, seed=4242, keep=R, want_final=True)
    assert got["stats"].shape == (6, 4, 3, steps)
    assert_same(got, mm.HostStochasticSIR(pb).run(R, seed=4242, keep=R, want_final=True))
    if steps > 1:
        assert np.any(got["traj"][1, :, 0, 1] != 1.9e9)  # the large group moved


@pytest.mark.parametrize("R,steps", [(16384, 3), (16448, 12)])
def test_sort_path_boundary(mm, R, steps):
    """16384 replicates are the longest segment the LDS sort takes, 16448 (a multiple of 64, no power of two) goes through the
    segmented radix sort: the statistics are the explicit formulas on the returned trajectories, and the twin's."""
    pb = six_groups(mm, steps)
    got = mm.HipStochasticSIR(pb, device=0).run(R, seed=99, keep=R, want_final=True)
    check_summaries(got["stats"], got["traj"])
    assert_same(got, mm.HostStochasticSIR(pb).run(R, seed=99, keep=R, want_final=True))


def test_independence_of_company_chunking_and_seed(mm):
    pb = six_groups(mm, 25)
    hip = mm.HipStochasticSIR(pb, device=0)
    big = hip.run(256, seed=7, keep=64, want_final=True)
    small = hip.run(64, seed=7, keep=64, want_final=True)
    assert np.array_equal(big["traj"], small["traj"]) and np.array_equal(big["final_state"][:, :64], small["final_state"])
    whole = hip.run(200, seed=7, keep=200, want_final=True)
    assert np.array_equal(whole["traj"][:, :64], small["traj"])
    step_bytes = 6 * 3 * 256 * 8  # 200 replicates are padded to 256
    chunked = hip.run(200, seed=7, keep=200, want_final=True, max_workspace_bytes=8 * step_bytes)  # 8 + 8 + 8 + 1 rows
    assert_same(chunked, whole)
    assert_same(hip.run(200, seed=7, keep=200, want_final=True, max_workspace_bytes=1), whole)      # one row per chunk
    assert_same(hip.run(200, seed=7, keep=200, want_final=True), whole)
    other = hip.run(200, seed=8, keep=200, want_final=True)
    assert not np.array_equal(other["traj"], whole["traj"]) and not np.array_equal(other["stats"], whole["stats"])
    assert hip.phase_ms["step"] > 0.0


def test_probe_equals_twin_on_the_grid(mm):
    n = np.repeat(np.array(BINOM_N, dtype=np.int32), len(BINOM_P) * 4096)
    p = np.tile(np.repeat(np.array(BINOM_P), 4096), len(BINOM_N))
    pb = six_groups(mm, 1)
    got = mm.HipStochasticSIR(pb, device=0).binomial(n, p, seed=31337)
    assert np.array_equal(got, mm.hostabi.stoch_binomial_probe(n, p, seed=31337))
    assert np.all(got[p == 0.0] == 0) and np.all(got[p == 1.0] == n[p == 1.0]) and got.min() >= 0 and np.all(got <= n)


def test_transition_distributions_on_the_device(mm):
    """R = 20 000.  beta = 0: I_t ~ Binomial(I0, (1 - pR)^t) at t = 5; one step: S0 - S_1 ~ Binomial(S0, pI)."""
    R = 20000
    pb = mm.StochasticSIRProblem(N=1000.0, beta=[0.0, 0.4], gamma=0.04, S0=900.0, I0=100.0, R0=0.0, t_start=0.0, t_end=5.0, h=1.0)
    tr = mm.HipStochasticSIR(pb, device=0).run(R, seed=2718, keep=R)["traj"]
    pI, pR = mm.hostabi.stoch_probabilities(0.4, 100.0, 1.0, 1000.0, 0.04)
    for name, draws, n, p in (("I_5 at beta = 0", tr[0, :, 1, 5], 100, (1.0 - pR) ** 5), ("S0 - S_1", 900.0 - tr[1, :, 0, 1], 900, pI)):
        assert np.all(draws % 1.0 == 0.0)
        pval, z = chi_square_against_binomial(draws.astype(np.int64), n, p)
        print(f"{name}: chi-square p-value {pval:.4g}, z of the mean {z:+.3f}")
        assert pval >= 1e-6 and abs(z) <= 6.0, (name, pval, z)


def numpy_chain_binomial(R, steps, seed, N=1000.0, beta=0.4, gamma=0.04, S0=999, I0=1, h=1.0):
    """an independent simulation of the model with numpy's generator and sampler, the freeze rule included"""
    rng = np.random.default_rng(seed)
    S, I, Rc = np.full(R, S0, dtype=np.int64), np.full(R, I0, dtype=np.int64), np.zeros(R, dtype=np.int64)
    out = np.empty((R, 3, steps))
    pR = 1.0 - math.exp(-gamma * h)
    for step in range(steps):
        out[:, 0, step], out[:, 1, step], out[:, 2, step] = S, I, Rc
        live = (S > 0) & (I > 0)
        pI = 1.0 - np.exp(-(beta * I * h / N))
        I_new = np.where(live, rng.binomial(S, pI), 0)
        R_new = np.where(live, rng.binomial(I, pR), 0)
        S, I, Rc = S - I_new, I + I_new - R_new, Rc + R_new
    return out


def test_paths_agree_in_distribution_with_a_numpy_simulation(mm):
    """two-sample Kolmogorov-Smirnov, reference workload at h = 1, 20 000 replicates each, steps 1, 10, 30 and 100, all three
    compartments: p >= 1e-6 (two independent numpy runs give minimum p-values of 0.2 to 0.4)"""
    from scipy import stats
    R = 20000
    pb = mm.workloads.stochastic_sir_reference()[0].with_(h=1.0, t_end=100.0)
    tr = mm.HipStochasticSIR(pb, device=0).run(R, seed=1618, keep=R)["traj"][0]
    ref = numpy_chain_binomial(R, 101, seed=5)
    worst = 1.0
    for step in (1, 10, 30, 100):
        for c in range(3):
            pval = float(stats.ks_2samp(tr[:, c, step], ref[:, c, step]).pvalue)
            print(f"step {step} compartment {'SIR'[c]}: KS p-value {pval:.4g}")
            worst = min(worst, pval)
    assert worst >= 1e-6, worst


def test_argument_errors_return_invalid_arg(mm):
    lib = mm.load_library()
    h = mm.hipabi
    pb = six_groups(mm, 25)
    tab = pb.group_table()
    stats = np.full((6, 4, 3, 25), -7.0)
    err = C.create_string_buffer(256)

    def run(cfg, groups=tab, out=stats):
        return lib.sepaihrd_stoch_sir_run(0, C.byref(cfg), None if groups is None else groups.ctypes.data,
                                          None if out is None else out.ctypes.data, None, None, None, err, len(err))

    assert run(h.stoch_sir_config(pb, 0, 1)) == -1 and b"replicate" in err.value
    assert run(h.stoch_sir_config(pb, 8, 1, keep=9)) == -1 and b"keep" in err.value
    assert run(h.stoch_sir_config(pb, 8, 1, keep=2)) == -1 and b"traj" in err.value          # keep without a traj buffer
    assert run(h.stoch_sir_config(pb, 8, 1, abi_version=2)) == -1 and b"abi_version" in err.value
    assert run(h.stoch_sir_config(pb, 8, 1), out=None) == -1 and b"stats" in err.value
    assert run(h.stoch_sir_config(pb, 8, 1), groups=None) == -1
    assert run(h.stoch_sir_config(pb.with_(h=-1.0), 8, 1)) == -1 and b"h must be > 0" in err.value
    bad = pb.with_(S0=pb.S0 + 5.0).group_table()
    assert run(h.stoch_sir_config(pb, 8, 1), groups=bad) == -1 and b"must sum to N" in err.value
    assert np.all(stats == -7.0)  # nothing was written
    with pytest.raises(ValueError, match="must sum to N"):
        mm.HipStochasticSIR(pb.with_(S0=pb.S0 + 5.0), device=0).run(8, seed=1)
    one = np.zeros(1, dtype=np.int32)
    assert lib.sepaihrd_stoch_sir_binomial_device(0, 1, one.ctypes.data, None, 1, one.ctypes.data, err, len(err)) == -1
    assert run(h.stoch_sir_config(pb, 8, 1)) == 0 and not np.any(stats == -7.0)
