"""The stochastic chain-binomial SEPAIHRD model on the host twin (hostStochasticSEPAIHRD), with hand-made model values: path
invariants, degenerate rates, the distribution of each of the 13 draws, an independent numpy simulation, the stream coordinates
and the argument rules.  No device."""
import math

import numpy as np
import pytest

from test_stoch_sir_cpu import chi_square_against_binomial

PROBS = [0.05, 0.5, 0.95]
SEED = 0x0BAD_CAFE_1234_5678
S_, E_, P_, A_, I_, H_, ICU_, R_, D_, CUMH_, CUMICU_ = range(11)
POP = [S_, E_, P_, A_, I_, H_, ICU_, R_, D_]


def initial(n, **counts):
    x = np.zeros((11, n))
    for name, v in counts.items():
        x[{"S": 0, "E": 1, "P": 2, "A": 3, "I": 4, "H": 5, "ICU": 6, "R": 7, "D": 8}[name]] = v
    return x


def run(mm, rows, times, N, M, R, m, seed=SEED, status=None, keep=None, kappa_ends=(1e9,), beta_ends=(), probs=PROBS):
    rows = np.atleast_2d(rows)
    st = np.zeros(rows.shape[0], dtype=np.int32) if status is None else status
    return mm.hostabi.stochastic_from_values(rows, st, times, N, M, kappa_ends, R, m, seed, probs, beta_end_times=beta_ends,
                                             keep=R if keep is None else keep)


# ---- invariants
def three_age_case(mm):
    n = 3
    x0 = initial(n, S=[900, 1500, 700], E=[10, 20, 5], P=[5, 5, 5], A=[3, 4, 5], I=[8, 2, 6], H=[2, 1, 3], ICU=[1, 0, 2], R=[4, 4, 4])
    row = mm.hostabi.stochastic_pack_values(
        n, x0, beta_values=[0.9, 0.4], kappa_values=[1.0, 0.5], theta=0.6, sigma=0.4, gamma_p=0.5, gamma_A=0.3, gamma_I=0.2, gamma_H=0.15,
        gamma_ICU=0.1, a=[0.8, 1.0, 1.2], h_infec=[1.0, 0.9, 1.1], p=[0.5, 0.4, 0.3], h=[0.05, 0.1, 0.2], icu=[0.05, 0.1, 0.15],
        d_H=[0.01, 0.02, 0.08], d_ICU=[0.05, 0.1, 0.2], d_community=[0.001, 0.01, 0.05])
    N = x0[POP].sum(axis=0)
    M = np.array([[3.0, 1.0, 0.5], [1.0, 2.0, 1.0], [0.5, 1.0, 1.5]])
    times = np.arange(8.0)  # the beta breakpoint at 2.5 and the kappa breakpoint at 4.5 lie inside; no midpoint of m = 2 meets them
    return row, times, N, M, x0


def test_path_invariants(mm):
    row, times, N, M, x0 = three_age_case(mm)
    out = run(mm, row, times, N, M, R=50, m=2, beta_ends=[2.5, 1e9], kappa_ends=[4.5, 1e9], probs=[0.0, 0.5, 1.0])
    tr = out["traj"][0]  # [R][T][11][n]
    assert tr.shape == (50, 8, 11, 3)
    assert np.array_equal(tr, np.round(tr)) and (tr >= 0).all()
    assert np.array_equal(tr[:, 0], np.broadcast_to(x0, (50, 11, 3)))
    total = tr[:, :, POP].sum(axis=2)
    assert np.array_equal(total, np.broadcast_to(total[:, :1], total.shape))
    for c in (D_, CUMH_, CUMICU_, R_):
        assert (np.diff(tr[:, :, c], axis=1) >= 0).all()
    assert (np.diff(tr[:, :, S_], axis=1) <= 0).all()
    assert (np.diff(tr[:, :, S_], axis=1) < 0).any() and (np.diff(tr[:, :, D_], axis=1) > 0).any()  # the epidemic moves
    assert np.array_equal(out["final_state"][0], tr[:, -1])
    # quantiles at 0, 0.5 (R even: interpolated) and 1 from the paths themselves; series 3..5 are running sums of 0..2
    daily = np.stack([np.diff(tr[:, :, c], axis=1, prepend=tr[:, :1, c]) for c in (CUMH_, CUMICU_, D_)])  # [3][R][T][n]
    series = np.concatenate([daily, np.cumsum(daily, axis=2)])                                              # [6][R][T][n]
    srt = np.sort(series, axis=1)
    q = out["quantiles"]
    assert np.array_equal(q[:, 0], srt[:, 0]) and np.array_equal(q[:, 2], srt[:, -1])
    assert np.array_equal(q[:, 1], srt[:, 24] * 0.5 + srt[:, 25] * 0.5)
    assert (q[3:, :, -1] > 0).any()
    extinct = np.mean((tr[:, -1, [E_, P_, A_, I_]] == 0).all(axis=(1, 2)))
    assert out["extinct"][0] == extinct


# ---- degenerate rates
def one_age(mm, counts=1000, **fields):
    x0 = initial(1, S=counts, E=counts, P=counts, A=counts, I=counts, H=counts, ICU=counts)
    fields.setdefault("a", 1.0)
    fields.setdefault("h_infec", 1.0)
    beta = fields.pop("beta", 0.0)
    return mm.hostabi.stochastic_pack_values(1, x0, beta=beta, **fields), x0


def one_step(mm, row, R, times=(0.0, 1.0), m=1, seed=SEED):
    out = run(mm, row, list(times), [7000.0], [[1.0]], R, m, seed=seed, keep=0)
    return out["final_state"][0, :, :, 0].astype(np.int64)  # [R][11]


ALL_RATES = dict(beta=0.8, theta=0.5, sigma=0.3, gamma_p=0.4, gamma_A=0.2, gamma_I=0.25, gamma_H=0.15, gamma_ICU=0.1, p=0.4, h=0.1, icu=0.1,
                 d_H=0.05, d_ICU=0.1, d_community=0.02)


def test_degenerate_rates(mm):
    x0 = initial(1, S=1000, E=1000, P=1000, A=1000, I=1000, H=1000, ICU=1000)[:, 0]
    times = [0.0, 1.0, 2.0, 3.0]
    fin = one_step(mm, one_age(mm, **{**ALL_RATES, "beta": 0.0})[0], 40, times, m=2)
    assert (fin[:, S_] == 1000).all() and (fin[:, E_] < 1000).all()
    # every rate 0: each share has a zero denominator and every row stays row 0
    out = run(mm, one_age(mm)[0], times, [7000.0], [[1.0]], 40, 2)
    assert np.array_equal(out["traj"][0][:, :, :, 0], np.broadcast_to(x0, (40, 4, 11)))
    assert not out["quantiles"].any() and out["extinct"][0] == 0.0
    # p_i = 1 sends nobody to I, p_i = 0 nobody to A (nothing else feeds or drains them here)
    fin = one_step(mm, one_age(mm, gamma_p=0.5, p=1.0)[0], 40)
    assert (fin[:, I_] == 1000).all() and (fin[:, A_] > 1000).all() and np.array_equal(fin[:, A_] - 1000, 1000 - fin[:, P_])
    fin = one_step(mm, one_age(mm, gamma_p=0.5, p=0.0)[0], 40)
    assert (fin[:, A_] == 1000).all() and (fin[:, I_] > 1000).all() and np.array_equal(fin[:, I_] - 1000, 1000 - fin[:, P_])
    # a rate of 1e6 empties its compartment in one step
    for field, comp in (("sigma", E_), ("gamma_p", P_), ("gamma_A", A_), ("gamma_I", I_), ("gamma_H", H_), ("gamma_ICU", ICU_)):
        fin = one_step(mm, one_age(mm, **{field: 1e6})[0], 10)
        assert (fin[:, comp] == (1000 if comp == I_ and field == "gamma_p" else 0)).all(), field
    fin = one_step(mm, one_age(mm, beta=1e6)[0], 10)
    assert (fin[:, S_] == 0).all() and (fin[:, E_] == 2000).all()


# ---- each of the 13 draws
def pr(rate, h=1.0):
    return 1.0 - math.exp(-rate * h)


def check_binomial(name, draws, n, p):
    pval, z = chi_square_against_binomial(np.asarray(draws, dtype=np.int64), n, p)
    print(f"{name}: Binomial({n}, {p:.6g}) chi-square p-value {pval:.4g}, z of the mean {z:+.3f}")
    assert pval >= 1e-6, (name, pval)
    assert abs(z) <= 6.0, (name, z)


def test_each_draw_has_its_binomial_distribution(mm):
    """One step of length 1 from 1000 in every non-absorbing compartment, n = 1, R = 20 000.  The seven draws out of a compartment
    come from one run in which no split moves anybody (p_i = 0, h_i = 0, icu_i = 0); each of the six splits from a run of its own
    in which a rate of 1e6 empties the parent compartment, so that the split's n is 1000 in every replicate."""
    R = 20000
    r = dict(ALL_RATES, p=0.0, h=0.0, icu=0.0)
    fin = one_step(mm, one_age(mm, **r)[0], R)
    d = 1000 - fin  # net outflow
    lam = 1.0 * ((1000 + 1000 + r["theta"] * 1000) * 1.0 * (1.0 / 7000.0)) * (r["beta"] * 1.0 * 1.0)
    d0 = d[:, S_]
    d1 = d0 + d[:, E_]
    d2 = d1 + d[:, P_]
    check_binomial("0 S->E", d0, 1000, pr(lam))
    check_binomial("1 E->P", d1, 1000, pr(r["sigma"]))
    check_binomial("2 P out", d2, 1000, pr(r["gamma_p"]))
    check_binomial("4 A->R", d[:, A_], 1000, pr(r["gamma_A"]))
    check_binomial("5 I out", d2 + d[:, I_], 1000, pr(r["gamma_I"] + r["d_community"]))
    check_binomial("8 H out", d[:, H_], 1000, pr(r["gamma_H"] + r["d_H"]))
    check_binomial("11 ICU out", d[:, ICU_], 1000, pr(r["gamma_ICU"] + r["d_ICU"]))
    assert not fin[:, CUMH_].any() and not fin[:, CUMICU_].any()
    splits = (("3 P->A", dict(gamma_p=1e6, p=0.35), A_, P_, 0.35),
              ("6 I->H", dict(gamma_I=7e5, h=3e5), CUMH_, I_, 0.3),
              ("7 I->D", dict(gamma_I=6e5, d_community=4e5), D_, I_, 0.4),
              ("9 H->ICU", dict(gamma_H=7.5e5, icu=2.5e5), CUMICU_, H_, 0.25),
              ("10 H->D", dict(gamma_H=4e5, d_H=6e5), D_, H_, 0.6),
              ("12 ICU->D", dict(gamma_ICU=8e5, d_ICU=2e5), D_, ICU_, 0.2))
    for k, (name, rates, into, parent, share) in enumerate(splits):
        fin = one_step(mm, one_age(mm, **rates)[0], R, seed=SEED + 1 + k)
        assert (fin[:, parent] == 0).all(), name
        gain = fin[:, into] - (1000 if into == A_ else 0)
        check_binomial(name, gain, 1000, share)


# ---- an independent implementation
def numpy_simulation(rates, x0, N, M, T, m, R, seed):
    """The table of the issue with numpy's generator, vectorised over replicates: rows [R][T][11][n]."""
    rng = np.random.default_rng(seed)
    n = len(N)
    x = np.broadcast_to(x0.astype(np.int64), (R, 11, n)).copy()
    rows = np.empty((R, T, 11, n), dtype=np.int64)
    rows[:, 0] = x
    h = 1.0 / m
    g = rates

    def p_of(rate):
        return 1.0 - np.exp(-np.asarray(rate) * h)

    def share(a, b):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        return np.where(a + b > 0, a / np.where(a + b > 0, a + b, 1.0), 0.0)

    for k in range(T - 1):
        for _ in range(m):
            inf = (x[:, P_] + x[:, A_] + g["theta"] * x[:, I_]) * g["h_infec"] / N          # [R][n]
            lam = np.maximum(0.0, inf @ M.T * (g["beta"] * g["a"]))
            d0 = rng.binomial(x[:, S_], p_of(lam))
            d1 = rng.binomial(x[:, E_], p_of(g["sigma"]))
            d2 = rng.binomial(x[:, P_], p_of(g["gamma_p"]))
            d3 = rng.binomial(d2, np.clip(g["p"], 0, 1))
            d4 = rng.binomial(x[:, A_], p_of(g["gamma_A"]))
            d5 = rng.binomial(x[:, I_], p_of(g["gamma_I"] + g["h"] + g["d_community"]))
            d6 = rng.binomial(d5, share(g["h"], g["gamma_I"] + g["d_community"]))
            d7 = rng.binomial(d5 - d6, share(g["d_community"], g["gamma_I"]))
            d8 = rng.binomial(x[:, H_], p_of(g["gamma_H"] + g["d_H"] + g["icu"]))
            d9 = rng.binomial(d8, share(g["icu"], g["gamma_H"] + g["d_H"]))
            d10 = rng.binomial(d8 - d9, share(g["d_H"], g["gamma_H"]))
            d11 = rng.binomial(x[:, ICU_], p_of(g["gamma_ICU"] + g["d_ICU"]))
            d12 = rng.binomial(d11, share(g["d_ICU"], g["gamma_ICU"]))
            x[:, S_] -= d0
            x[:, E_] += d0 - d1
            x[:, P_] += d1 - d2
            x[:, A_] += d3 - d4
            x[:, I_] += d2 - d3 - d5
            x[:, H_] += d6 - d8
            x[:, ICU_] += d9 - d11
            x[:, R_] += d4 + (d5 - d6 - d7) + (d8 - d9 - d10) + (d11 - d12)
            x[:, D_] += d7 + d10 + d12
            x[:, CUMH_] += d6
            x[:, CUMICU_] += d9
        rows[:, k + 1] = x
    return rows


def test_paths_agree_in_distribution_with_a_numpy_simulation(mm):
    """two-sample Kolmogorov-Smirnov on I, H and D of age 0 at times 5, 15 and 29, 20 000 replicates each: p >= 1e-6"""
    from scipy import stats
    R, T, m, n = 20000, 30, 2, 2
    vec = dict(a=np.array([0.9, 1.1]), h_infec=np.array([1.0, 0.8]), p=np.array([0.4, 0.3]), h=np.array([0.08, 0.15]),
               icu=np.array([0.1, 0.15]), d_H=np.array([0.03, 0.06]), d_ICU=np.array([0.1, 0.2]), d_community=np.array([0.03, 0.05]))
    sc = dict(theta=0.6, sigma=0.35, gamma_p=0.5, gamma_A=0.25, gamma_I=0.2, gamma_H=0.12, gamma_ICU=0.1, beta=0.45)
    x0 = initial(n, S=[4000, 6000], E=[30, 20], P=[10, 10], A=[10, 5], I=[30, 20], H=[4, 6], ICU=[1, 2])
    N = x0[POP].sum(axis=0)
    M = np.array([[2.5, 1.0], [0.8, 2.0]])
    ref = numpy_simulation({**vec, **sc}, x0, N, M, T, m, R, seed=77)
    cells = [(c, t) for t in (5, 15, 29) for c in (I_, H_, D_)]
    for c, t in cells:  # the test would be empty on a constant cell: checked on the numpy simulation alone
        assert np.unique(ref[:, t, c, 0]).size > 3, (c, t)
    row = mm.hostabi.stochastic_pack_values(n, x0, **sc, **vec)
    tr = run(mm, row, np.arange(float(T)), N, M, R, m)["traj"][0]
    worst = 1.0
    for c, t in cells:
        pval = float(stats.ks_2samp(tr[:, t, c, 0], ref[:, t, c, 0]).pvalue)
        print(f"time {t} compartment {mm.hostabi.STOCH_COMPARTMENTS[c]}: KS p-value {pval:.4g}")
        worst = min(worst, pval)
    assert worst >= 1e-6, worst


# ---- the stream
def test_stream_coordinates_and_independence(mm):
    host = mm.hostabi
    n = 2
    sc = dict(theta=0.5, sigma=0.3, beta=0.7)
    a, h_infec = [0.9, 1.2], [1.0, 0.7]
    x0 = initial(n, S=[5000, 300], E=[40, 7], P=[12, 3], A=[5, 9], I=[20, 4])
    row = host.stochastic_pack_values(n, x0, a=a, h_infec=h_infec, **sc)
    N = [6000.0, 400.0]
    M = np.array([[2.0, 0.5], [0.7, 1.5]])
    times = [0.0, 0.5, 1.5]  # two intervals of different length, m = 1: row k + 1 is the state after step k
    rows = np.stack([row, row, row])
    R = 6
    base = run(mm, rows, times, N, M, R, 1)
    tr = base["traj"].astype(np.int64)  # [S][R][T][11][n]
    for s, r, step, age in ((0, 0, 0, 0), (2, 5, 1, 1), (1, 3, 1, 0), (2, 0, 0, 1)):
        x = tr[s, r, step]
        hk = times[step + 1] - times[step]
        inf = [((float(x[P_, j]) + float(x[A_, j])) + sc["theta"] * float(x[I_, j])) * h_infec[j] * (1.0 / N[j]) for j in range(n)]
        total = 0.0
        for j in range(n):
            total += M[age, j] * inf[j]
        lam = total * ((sc["beta"] * 1.0) * a[age])
        p_inf = 1.0 - float(host.glibc_exp(np.array([-(lam * hk)]))[0])
        p_e = 1.0 - float(host.glibc_exp(np.array([-(sc["sigma"] * hk)]))[0])
        word = (step * 64 + age) * 16
        d0 = host.stoch_binomial_at(SEED, word // 2, s, r, 0, int(x[S_, age]), p_inf)  # 2 group + transition = word + transition
        d1 = host.stoch_binomial_at(SEED, word // 2, s, r, 1, int(x[E_, age]), p_e)
        nxt = tr[s, r, step + 1]
        assert d0 == x[S_, age] - nxt[S_, age] and d0 > 0, (s, r, step, age)
        assert d1 == d0 - (nxt[E_, age] - x[E_, age]) and d1 > 0
    # samples with equal values differ by their position in theta, replicates by their index
    assert not np.array_equal(tr[0], tr[1]) and not np.array_equal(tr[0, 0], tr[0, 1])
    # the same (seed, s, r): whatever R, keep, and whether the samples before it are valid
    more = run(mm, rows, times, N, M, R + 5, 1, keep=2)
    assert np.array_equal(more["final_state"][:, :R], base["final_state"]) and np.array_equal(more["traj"], base["traj"][:, :2])
    holes = run(mm, rows, times, N, M, R, 1, status=np.array([1, 0, 1], dtype=np.int32))
    assert np.array_equal(holes["traj"][1], base["traj"][1]) and np.array_equal(holes["final_state"][1], base["final_state"][1])
    assert np.isnan(holes["traj"][[0, 2]]).all() and np.isnan(holes["final_state"][[0, 2]]).all() and np.isnan(holes["extinct"][[0, 2]]).all()
    assert holes["n_valid"] == 1 and np.isfinite(holes["quantiles"]).all()
    alone = run(mm, rows[1:2], times, N, M, R, 1, probs=PROBS)
    assert not np.array_equal(alone["traj"][0], base["traj"][1])  # position 0 now: another stream
    none = run(mm, rows, times, N, M, R, 1, status=np.ones(3, dtype=np.int32))
    assert none["n_valid"] == 0 and np.isnan(none["quantiles"]).all()
    other = run(mm, rows, times, N, M, R, 1, seed=SEED + 1)
    assert not np.array_equal(other["traj"], base["traj"])
    other_hi = run(mm, rows, times, N, M, R, 1, seed=SEED + (1 << 32))
    assert not np.array_equal(other_hi["traj"], base["traj"])


# ---- arguments
def test_validator_messages(mm):
    ok = dict(S=3, R=4, steps_per_interval=2, keep=1, n_times=10, T_pos=8, n_age=4, probs=PROBS)
    mm.hostabi.stochastic_validate(**ok)
    for change, word in ((dict(S=0), "S must be >= 1"), (dict(R=0), "R must be >= 1"), (dict(steps_per_interval=0), "steps_per_interval must be >= 1"),
                         (dict(keep=-1), "keep must lie in [0, R]"), (dict(keep=5), "keep must lie in [0, R]"),
                         (dict(S=2 ** 16, R=2 ** 15), "below 2^31"), (dict(S=2 ** 31 - 1, R=1), "below 2^31"),
                         (dict(T_pos=0), "output time >= 0"), (dict(T_pos=11), "n_times >= T_pos"), (dict(n_age=0), "n_age must be >= 1"),
                         (dict(n_times=2 ** 21, T_pos=5, steps_per_interval=2), "below 2^22"), (dict(probs=[]), "need probs"),
                         (dict(probs=[0.5, 1.5]), "probabilities must lie in [0, 1]"), (dict(probs=[float("nan")]), "probabilities")):
        with pytest.raises(ValueError) as e:
            mm.hostabi.stochastic_validate(**{**ok, **change})
        assert word in str(e.value) and str(e.value).startswith("ensemble_stochastic: "), (change, str(e.value))
    mm.hostabi.stochastic_validate(**{**ok, "n_times": 2 ** 21 - 1, "T_pos": 5})
    assert mm.hostabi.stochastic_values_width(4, 2, 3) == 8 + 2 + 3 + 19 * 4
    assert mm.hipabi.load_library().sepaihrd_stochastic_values_width(0, 0, 1) == -1


def test_twin_refuses_what_the_device_call_refuses(mm):
    row, times, N, M, _ = three_age_case(mm)
    with pytest.raises(ValueError, match="R must be >= 1"):
        run(mm, row, times, N, M, R=0, m=1, beta_ends=[2.5, 1e9], kappa_ends=[4.5, 1e9], keep=0)
    with pytest.raises(ValueError, match="at most 16 age classes"):
        x0 = initial(17, S=10)
        wide = mm.hostabi.stochastic_pack_values(17, x0)
        run(mm, wide, [0.0, 1.0], np.ones(17), np.eye(17), R=1, m=1, keep=0)


def test_header_and_exports(mm):
    import os
    for sym in ("sepaihrd_ensemble_stochastic", "sepaihrd_stochastic_validate", "sepaihrd_stochastic_values_width", "sepaihrd_stochastic_timing"):
        assert sym in mm.hipabi.EXPORTED_SYMBOLS
        assert hasattr(mm.hipabi.load_library(), sym)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sepaihrd_hip.h")).read()
    assert "#define SEPAIHRD_ABI_VERSION 3" in text and "int sepaihrd_ensemble_stochastic(" in text
