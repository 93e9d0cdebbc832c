"""Stochastic chain-binomial SIR ensembles without a device: the random stream, the binomial sampler, the step logic, the
summaries, the validator and the C++ adapter, all through the host twin (libsepaihrd_host.so), which compiles the text the
kernel compiles (csrc/sepaihrd_stoch.inc)."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MASK = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ref(mm):
    return mm.workloads.stochastic_sir_reference(GOLDEN)


def cases_problem(mm, pb_ref, t_end=25.0):
    """the reference workload at h = 1, a fractional start, beta = 0, gamma = 0 and I0 = 0 as five groups of one call"""
    return mm.StochasticSIRProblem(N=[1000.0, 100.5, 1000.0, 1000.0, 1000.0], beta=[0.4, 0.9, 0.0, 0.4, 0.4],
                                   gamma=[0.04, 0.2, 0.04, 0.0, 0.04], S0=[999.0, 90.25, 900.0, 999.0, 1000.0],
                                   I0=[1.0, 10.25, 100.0, 1.0, 0.0], R0=[0.0, 0.0, 0.0, 0.0, 0.0], t_start=0.0, t_end=t_end, h=1.0)


# ---- the stream
def philox_python(counter, key):
    """Philox-4x32-10 as Salmon et al. publish it, written independently of csrc/sepaihrd_stoch.inc"""
    c = [int(x) for x in counter]
    k = [int(x) for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + 0x9E3779B9) & MASK, (k[1] + 0xBB67AE85) & MASK]
    return c


def test_philox_known_answers_and_independent_restatement(mm, ref):
    _, fx = ref
    host = mm.hostabi
    assert len(fx["philox4x32_10"]) == 3
    for v in fx["philox4x32_10"]:
        counter, key, want = ([int(x, 16) for x in v[k]] for k in ("counter", "key", "output"))
        assert philox_python(counter, key) == want
        assert host.stoch_philox(counter, key).tolist() == want
    rs = np.random.RandomState(11)
    words = rs.randint(0, 2**32, size=(1000, 6), dtype=np.uint64)
    for w in words:
        assert host.stoch_philox(w[:4], w[4:]).tolist() == philox_python(w[:4], w[4:])


def test_uniform_rule_stays_strictly_inside_the_unit_interval(mm):
    host = mm.hostabi
    assert host.stoch_uniform(0, 0) == 2.0 ** -53
    assert host.stoch_uniform(MASK, MASK) == 1.0 - 2.0 ** -53
    assert 0.0 < host.stoch_uniform(0, 0) and host.stoch_uniform(MASK, MASK) < 1.0
    assert math.isfinite(math.log(host.stoch_uniform(0, 0))) and math.log(1.0 - host.stoch_uniform(MASK, MASK)) < 0.0
    rs = np.random.RandomState(12)
    for lo, hi in rs.randint(0, 2**32, size=(200, 2), dtype=np.uint64):
        w = (int(hi) << 32) | int(lo)
        assert host.stoch_uniform(lo, hi) == ((w >> 12) + 0.5) * 2.0 ** -52  # exact: 53 significant bits at the most


# ---- the sampler's distribution
BINOM_N = (1, 2, 10, 50, 1000, 10**6, 2**31 - 1)
BINOM_P = (0.0, 1e-9, 1e-3, 0.2, 0.5, 0.7, 1 - 1e-3, 1.0)
DRAWS = 200_000


def chi_square_against_binomial(draws, n, p):
    """(p-value, z of the sample mean): support cut at the 1e-9 tails with the tail mass folded into the end bins,
    neighbouring bins pooled left to right until the expected count is at least 10."""
    from scipy import stats
    d = stats.binom(n, p)
    lo, hi = int(d.ppf(1e-9)), int(d.isf(1e-9))
    k = np.arange(lo, hi + 1)
    prob = d.pmf(k)
    prob[0] += d.cdf(lo - 1)
    prob[-1] += d.sf(hi)
    obs = np.bincount(np.clip(draws, lo, hi) - lo, minlength=len(k)).astype(np.float64)
    exp = prob * len(draws)
    O, E, o, e = [], [], 0.0, 0.0
    for oi, ei in zip(obs, exp):
        o, e = o + oi, e + ei
        if e >= 10.0:
            O.append(o); E.append(e)
            o = e = 0.0
    if e > 0.0 or o > 0.0:  # what is left joins the last pooled bin
        if O:
            O[-1] += o; E[-1] += e
        else:
            O.append(o); E.append(e)
    O, E = np.array(O), np.array(E)
    pval = 1.0 if len(O) < 2 else float(stats.chi2.sf(np.sum((O - E) ** 2 / E), len(O) - 1))
    sd = math.sqrt(n * p * (1.0 - p) / len(draws))
    z = 0.0 if sd == 0.0 else (float(np.mean(draws, dtype=np.float64)) - n * p) / sd
    return pval, z


def chi_square_against_pmf(draws, pmf):
    """chi_square_against_binomial for a given pmf over 0 .. len(pmf) - 1 (finite support: nothing to cut): the same pooling,
    left to right until the expected count is at least 10, the remainder into the last pooled bin; (p-value, z of the sample
    mean).  A draw outside the support, or where the pmf is exactly 0, is an assertion error: no bin could hold it."""
    from scipy import stats
    draws = np.asarray(draws).astype(np.int64).ravel()
    prob = np.asarray(pmf, dtype=np.float64)
    assert abs(prob.sum() - 1.0) < 1e-9 and draws.min() >= 0 and draws.max() < len(prob)
    obs = np.bincount(draws, minlength=len(prob)).astype(np.float64)
    assert not obs[prob == 0.0].any(), "draws where the pmf is exactly 0"
    exp = prob * len(draws)
    O, E, o, e = [], [], 0.0, 0.0
    for oi, ei in zip(obs, exp):
        o, e = o + oi, e + ei
        if e >= 10.0:
            O.append(o); E.append(e)
            o = e = 0.0
    if e > 0.0 or o > 0.0:  # what is left joins the last pooled bin
        if O:
            O[-1] += o; E[-1] += e
        else:
            O.append(o); E.append(e)
    O, E = np.array(O), np.array(E)
    pval = 1.0 if len(O) < 2 else float(stats.chi2.sf(np.sum((O - E) ** 2 / E), len(O) - 1))
    k = np.arange(len(prob))
    mean = float(np.sum(k * prob))
    sd = math.sqrt(max(0.0, float(np.sum(k * k * prob)) - mean * mean) / len(draws))
    z = 0.0 if sd == 0.0 else (float(np.mean(draws, dtype=np.float64)) - mean) / sd
    return pval, z


@pytest.mark.parametrize("n", BINOM_N)
def test_binomial_sampler_distribution(mm, n):
    """56 cases, 200 000 draws each at a fixed seed: chi-square p-value >= 1e-6 and |z| of the sample mean <= 6 in every one
    (a correct sampler breaks either with probability < 1e-4 over all of them); p = 0 gives 0 and p = 1 gives n."""
    host = mm.hostabi
    for j, p in enumerate(BINOM_P):
        draws = host.stoch_binomial_probe(np.full(DRAWS, n, dtype=np.int32), np.full(DRAWS, p), seed=20240611 + 100 * BINOM_N.index(n) + j)
        assert draws.min() >= 0 and draws.max() <= n
        if p == 0.0:
            assert not draws.any()
        elif p == 1.0:
            assert np.all(draws == n)
        else:
            pval, z = chi_square_against_binomial(draws.astype(np.int64), n, p)
            print(f"n={n} p={p}: chi-square p-value {pval:.4g}, z of the mean {z:+.3f}")
            assert pval >= 1e-6, (n, p, pval)
            assert abs(z) <= 6.0, (n, p, z)


def test_binomial_edges(mm):
    host = mm.hostabi
    assert host.stoch_binomial_at(1, 0, 0, 0, 0, 0, 0.3) == 0
    assert host.stoch_binomial_at(1, 0, 0, 0, 0, 17, 0.0) == 0
    assert host.stoch_binomial_at(1, 0, 0, 0, 0, 17, 1.0) == 17
    # a variate is a function of its coordinates: each one matters, and nothing else does
    base = (5, 1, 2, 3, 0, 1000, 0.3)
    again = [host.stoch_binomial_at(*base) for _ in range(2)]
    assert again[0] == again[1]
    seen = set()
    for pos in range(4):  # seed, group, replicate, step
        vals = []
        for delta in range(1, 9):
            c = list(base)
            c[pos] += delta
            vals.append(host.stoch_binomial_at(*c))
        seen.add(tuple(vals))
        assert len(set(vals)) > 1
    assert len(seen) == 4
    by_transition = [[host.stoch_binomial_at(5, 1, r, 3, t, 1000, 0.3) for r in range(8)] for t in (host.STOCH_INFECTION, host.STOCH_RECOVERY)]
    assert by_transition[0] != by_transition[1]


def test_probabilities_follow_the_reference_expressions(mm):
    host = mm.hostabi
    for beta, I, h, N, gamma in ((0.4, 1.0, 1.0, 1000.0, 0.04), (0.4, 37.0, 1 / 24, 1000.0, 0.04), (3.0, 1e8, 1.0, 2e9, 2.0),
                                 (0.9, 10.25, 1.0, 100.5, 0.2)):
        pI, pR = host.stoch_probabilities(beta, I, h, N, gamma)
        assert pI == 1.0 - float(host.glibc_exp(np.array([-(beta * I * h / N)]))[0])  # 1 - exp, not expm1
        assert pR == 1.0 - float(host.glibc_exp(np.array([-gamma * h]))[0])
        assert pI == pytest.approx(-math.expm1(-(beta * I * h / N)), rel=1e-12)
    assert host.stoch_probabilities(0.0, 5.0, 1.0, 10.0, 0.0) == (0.0, 0.0)
    assert host.stoch_probabilities(1e6, 1e3, 1.0, 1.0, 600.0) == (1.0, 1.0)   # exp of an argument <= -512: exactly 1
    assert host.stoch_probabilities(511.0, 1.0, 1.0, 1.0, 511.0) == (1.0, 1.0)  # inside the range: 1 - tiny rounds to 1


# ---- the step logic
def c_round(x):
    f = math.floor(x)
    return int(f + 1 if x - f >= 0.5 else f)


def python_paths(host, pb, replicates, seed, steps):
    """section 1 of the issue as a Python loop; probabilities and variates from the exported helpers"""
    out = np.empty((pb.n_groups, replicates, 3, steps))
    for g in range(pb.n_groups):
        N, beta, gamma = pb.N[g], pb.beta[g], pb.gamma[g]
        for r in range(replicates):
            S, I, R = pb.S0[g], pb.I0[g], pb.R0[g]
            for step in range(steps):
                out[g, r, :, step] = (S, I, R)
                if step == steps - 1:
                    break
                S_int, I_int = max(0, c_round(S)), max(0, c_round(I))
                if I_int <= 0 or S_int <= 0:
                    continue
                pI, pR = host.stoch_probabilities(beta, I, pb.h, N, gamma)
                I_new = host.stoch_binomial_at(seed, g, r, step, host.STOCH_INFECTION, S_int, pI)
                R_new = host.stoch_binomial_at(seed, g, r, step, host.STOCH_RECOVERY, I_int, pR)
                S, I, R = max(0.0, float(S_int - I_new)), max(0.0, float(I_int + I_new - R_new)), max(0.0, R + R_new)
    return out


@pytest.fixture(scope="module")
def twin_run(mm, ref):
    pb = cases_problem(mm, ref[0], t_end=60.0)
    return pb, mm.HostStochasticSIR(pb).run(6, seed=77, keep=6, want_final=True)


def test_twin_equals_python_restatement_bit_for_bit(mm, twin_run):
    pb, got = twin_run
    steps = got["stats"].shape[-1]
    assert steps == 61 and got["traj"].shape == (5, 6, 3, 61)
    want = python_paths(mm.hostabi, pb, 6, 77, steps)
    assert np.array_equal(got["traj"], want)
    assert np.array_equal(got["final_state"], want[:, :, :, -1])
    assert np.array_equal(got["times"], np.arange(61.0))


def test_reference_workload_at_unit_step_equals_python_restatement(mm, ref):
    pb = ref[0].with_(h=1.0)
    got = mm.HostStochasticSIR(pb).run(3, seed=5, keep=3)
    assert got["traj"].shape == (1, 3, 3, 361)
    assert np.array_equal(got["traj"], python_paths(mm.hostabi, pb, 3, 5, 361))


def test_path_invariants(mm, ref):
    pb = cases_problem(mm, ref[0], t_end=100.0)
    tr = mm.HostStochasticSIR(pb).run(200, seed=3, keep=200)["traj"]
    S, I, R = tr[:, :, 0], tr[:, :, 1], tr[:, :, 2]
    assert np.all(np.diff(S[..., 1:], axis=-1) <= 0) and np.all(np.diff(R, axis=-1) >= 0) and tr.min() >= 0.0
    for g in range(pb.n_groups):
        if g == 1:  # the fractional start: row 0 as given, integers after it (S' = S_int - I_new whatever is drawn)
            assert np.all(tr[g][:, :, 0] == np.array([90.25, 10.25, 0.0])) and np.all(tr[g][:, :, 1:] % 1.0 == 0.0)
        else:
            assert np.all(tr[g] % 1.0 == 0.0)
            assert np.all(S[g] + I[g] + R[g] == pb.N[g])
    assert np.all(S[2] == 900.0) and np.all(np.diff(I[2], axis=-1) <= 0)   # beta = 0: no infections, I only recovers
    assert np.all(R[3] == 0.0) and np.all(np.diff(I[3], axis=-1) >= 0)     # gamma = 0: no recoveries
    assert np.all(tr[4] == np.array([1000.0, 0.0, 0.0])[None, :, None])    # I0 = 0: frozen from the start
    # the reference's freeze rule: once S is 0 nothing moves any more, infectives included
    frozen = (S[0, :, -2] == 0.0) & (I[0, :, -2] > 0.0)
    assert np.array_equal(tr[0, frozen, :, -1], tr[0, frozen, :, -2])


def test_replicates_do_not_depend_on_company_keep_or_chunking(mm, ref):
    pb = cases_problem(mm, ref[0])
    twin = mm.HostStochasticSIR(pb)
    a = twin.run(40, seed=9, keep=40, want_final=True)
    b = twin.run(10, seed=9, keep=4, want_final=True)
    assert np.array_equal(a["traj"][:, :4], b["traj"]) and np.array_equal(a["final_state"][:, :10], b["final_state"])
    c = twin.run(40, seed=9, keep=40, want_final=True, max_workspace_bytes=3 * 40 * 8 * 7)  # 7 steps per chunk: 4 chunks of 26 rows
    for k in ("stats", "traj", "final_state"):
        assert np.array_equal(a[k], c[k]), k
    assert not np.array_equal(a["traj"], twin.run(40, seed=10, keep=40)["traj"])


# ---- the summaries
@pytest.mark.parametrize("R", [1, 2, 7, 10, 101])
def test_summaries_equal_the_explicit_formulas(mm, ref, R):
    pb = cases_problem(mm, ref[0])
    got = mm.HostStochasticSIR(pb).run(R, seed=21, keep=R)
    check_summaries(got["stats"], got["traj"])


def check_summaries(stats, traj):
    """stats [G][4][3][steps] against the formulas of the issue on traj [G][R][3][steps]"""
    x = np.sort(traj, axis=1)
    R = x.shape[1]
    lhs, rhs = (R - 1) // 2, R // 2
    median = x[:, lhs] if lhs == rhs else (x[:, lhs] + x[:, rhs]) / 2.0
    assert np.array_equal(stats[:, 1], median)
    for col, f in ((2, 0.05), (3, 0.95)):
        pos = f * (R - 1)
        i = int(pos)
        d = pos - i
        q = (1.0 - d) * x[:, i] + d * x[:, i + 1] if i + 1 < R else x[:, i]
        assert np.array_equal(stats[:, col], q)
    mean = x.mean(axis=1)
    assert np.all(np.abs(stats[:, 0] - mean) <= 1e-12 * np.maximum(np.abs(mean), 1e-300))


# ---- validation
def test_num_steps(mm):
    h = mm.hipabi
    assert h.stoch_sir_num_steps(0.0, 360.0, 1.0 / 24.0) == 8641
    assert h.stoch_sir_num_steps(0.0, 360.0, 1.0) == 361 and h.stoch_sir_num_steps(2.0, 3.0, 10.0) == 1
    assert h.stoch_sir_num_steps(0.0, 1.0, 0.0) < 0 and h.stoch_sir_num_steps(1.0, 1.0, 0.5) < 0
    assert h.stoch_sir_num_steps(0.0, 1.0, 1e-10) < 0 and h.stoch_sir_num_steps(0.0, float("inf"), 1.0) < 0


def test_validator_messages(mm, ref):
    pb, _ = ref
    v = mm.hipabi.stoch_sir_validate
    assert v(pb, 100) == (0, "")
    for change, word in ((dict(N=0.0, S0=0.0, I0=0.0), "N must be > 0"), (dict(beta=-0.1), ">= 0"), (dict(gamma=-1.0), ">= 0"),
                         (dict(S0=-1.0), ">= 0"), (dict(h=0.0), "h must be > 0"), (dict(t_end=0.0), "t_end must be > t_start"),
                         (dict(S0=990.0), "must sum to N"), (dict(N=2.0**31, S0=2.0**31 - 1), "2^31 - 1"),
                         (dict(h=1e-9), "steps"), (dict(beta=float("nan")), "finite")):
        rc, msg = v(pb.with_(**change), 100)
        assert rc == -1 and word in msg, (change, msg)
    assert v(pb, 0)[0] == -1 and "replicate" in v(pb, 0)[1]
    assert v(pb, 10, keep=11)[0] == -1 and v(pb, 1 << 25)[0] == -1
    assert v(pb, 10, abi_version=2)[0] == -1 and "abi_version" in v(pb, 10, abi_version=2)[1]
    two = mm.StochasticSIRProblem(N=[1000.0, 1000.0], beta=0.4, gamma=0.04, S0=[999.0, 500.0], I0=1.0, R0=0.0, t_end=5.0)
    rc, msg = v(two, 5)
    assert rc == -1 and msg.startswith("stoch_sir: group 1")
    with pytest.raises(ValueError, match="must sum to N"):
        mm.HostStochasticSIR(two).run(5, seed=1)


def test_adapter_throws_where_the_reference_does(mm, ref):
    pb, fx = ref
    a = dict(N=fx["N"], beta=fx["beta"], gamma=fx["gamma"], S0=fx["S0"], I0=fx["I0"], R0=fx["R0"], t_start=0.0, t_end=10.0, h=1.0,
             num_simulations=4)
    model = mm.hostabi.stoch_sir_model
    assert model(**a, run=False) == {"steps": 11}
    for change in (dict(N=0.0), dict(beta=-1.0), dict(gamma=-1.0), dict(S0=-1.0), dict(I0=-1.0), dict(R0=-1.0), dict(h=0.0),
                   dict(t_end=0.0), dict(num_simulations=0)):
        with pytest.raises(ValueError, match="Invalid parameters for StochasticSIRModel constructor."):
            model(**{**a, **change}, run=False)
    with pytest.raises(ValueError, match=re.escape("Initial compartments S0+I0+R0 must sum to N.")):
        model(**{**a, "S0": 900.0}, run=False)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        model(**{**a, "N": 2.0**32, "S0": 2.0**32 - 1}, run=False)


# ---- exported surface and adapter
def test_header_version_and_new_symbols(mm):
    header = open(os.path.join(ROOT, "include", "sepaihrd_hip.h")).read()
    assert re.search(r"#define SEPAIHRD_ABI_VERSION 3\b", header) and mm.hipabi.ABI_VERSION == 3
    lib = mm.load_library()
    for name in ("sepaihrd_stoch_sir_num_steps", "sepaihrd_stoch_sir_validate", "sepaihrd_stoch_sir_run", "sepaihrd_stoch_sir_binomial_device"):
        assert name in mm.hipabi.EXPORTED_SYMBOLS and re.search(r"\b" + name + r"\s*\(", header)
        assert getattr(lib, name) is not None
    assert not re.search(r"sepaihrd_stoch[a-z_]*\d", header)
    import ctypes
    assert ctypes.sizeof(mm.hipabi.sepaihrd_stoch_sir_config) == 56


def test_adapter_csv_files_match_the_reference_layout(mm, ref, tmp_path):
    pb, fx = ref
    out = mm.hostabi.stoch_sir_model(fx["N"], fx["beta"], fx["gamma"], fx["S0"], fx["I0"], fx["R0"], fx["t_start"], fx["t_end"], fx["h"],
                                     fx["numSimulations"], seed=2024, out_dir=str(tmp_path))
    assert out["steps"] == fx["num_steps"] == 8641
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["stochastic_sir_stats.csv"] + [f"stochastic_sir_sim_{i}.csv" for i in range(100)])
    lines = open(tmp_path / "stochastic_sir_stats.csv").read().split("\n")
    assert lines[0] == fx["stats_header"] and lines[1] == "0,999,999,999,999,1,1,1,1,0,0,0,0"
    assert lines[2].startswith("0.0416667,") and len(lines) == 8641 + 2 and lines[-1] == ""
    assert lines[8641].startswith("360,")
    for i in (0, 99):
        sim = open(tmp_path / f"stochastic_sir_sim_{i}.csv").read().split("\n")
        assert sim[0] == fx["sim_header"] and sim[1] == "0,999,1,0" and len(sim) == 8641 + 2
        last = np.array([float(v) for v in sim[8641].split(",")])
        assert np.array_equal(last[1:], out["results"][i, :, -1]) and last[1:].sum() == 1000.0
    # the adapter is the twin of the flat call: same seed, same numbers
    direct = mm.HostStochasticSIR(pb).run(100, seed=2024, keep=100)
    assert np.array_equal(direct["stats"][0], out["stats"]) and np.array_equal(direct["traj"][0], out["results"])
    # one simulation: no statistics file
    single = tmp_path / "single"
    single.mkdir()
    mm.hostabi.stoch_sir_model(1000.0, 0.4, 0.04, 999.0, 1.0, 0.0, 0.0, 5.0, 1.0, 1, seed=1, out_dir=str(single))
    assert os.listdir(single) == ["stochastic_sir_sim_0.csv"]
