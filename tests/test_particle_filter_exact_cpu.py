"""The particle filter and the stochastic SEPAIHRD stepper of the host twin against EXACT likelihoods of tiny epidemics.  With a
handful of people the model is a finite hidden Markov chain: exact_filter below walks it forward over every reachable state and
returns p(y | theta), its prefixes and the unnormalised final-state moments to rounding error.  A bootstrap filter that
resamples at every weighted row is unbiased for exactly these numbers (Del Moral 2004, section 7.4.2), whatever J is, so the
means over many independent estimates must meet them within their standard errors.  The reference is written from the table
and the prose at the head of csrc/sepaihrd_stoch_sepaihrd.inc and csrc/sepaihrd_particle.inc and calls nothing of the package.
No device."""
import functools
import itertools
import math

import numpy as np
import pytest

from test_stoch_sir_cpu import chi_square_against_pmf

S_, E_, P_, A_, I_, H_, ICU_, R_, D_ = range(9)
NUM_POP = 9          # the population compartments; CumH and CumICU follow them in a row of 11
NUM_SCALARS, NUM_VECTORS, NUM_COMP = 8, 8, 11
THETA, SIGMA, GAMMA_P, GAMMA_A, GAMMA_I, GAMMA_H, GAMMA_ICU, BETA = range(8)
V_A, V_H_INFEC, V_P, V_H, V_ICU, V_D_H, V_D_ICU, V_D_COMM = range(8)
SIM_FLOOR = 1e-10
COMP_NAMES = ("S", "E", "P", "A", "I", "H", "ICU", "R", "D")


# ---- the exact reference
def schedule_value(values, ends, t):
    """value j on (ends[j - 1], ends[j]], the first for t <= ends[0], the last beyond the last end"""
    return values[min(sum(1 for e in ends if t > e), len(values) - 1)]


def pr(rate, h):
    return min(1.0, max(0.0, -math.expm1(-(rate * h))))


def share(x, y):
    return x / (x + y) if x + y > 0.0 else 0.0


def multinomial_outcomes(count, probs):
    """[(k_1, .., k_r), probability] of `count` people each leaving by way i with probability probs[i] (staying otherwise)"""
    stay = max(0.0, 1.0 - math.fsum(probs))
    out = []
    for ks in itertools.product(range(count + 1), repeat=len(probs)):
        left = count - sum(ks)
        if left < 0:
            continue
        ways, rest, p = 1, count, stay ** left if left else 1.0
        for k, q in zip(ks, probs):
            ways *= math.comb(rest, k)
            rest -= k
            p *= q ** k if k else 1.0
        if p > 0.0:
            out.append((ks, ways * p))
    return out


class ExactResult:
    """Z [T_pos]; G [9][n]; states, the number of states of the final row; pmf [9][n] -> array over the counts 0 .. (only where no
    observation is usable: the weights are then all 1 and alpha is a probability)"""


def exact_filter(row, n, nb, nk, times, N, M, beta_ends, kappa_ends, m, runup_offset, obs_H, obs_ICU, obs_D):
    """Forward recursion over the reachable states of the chain-binomial SEPAIHRD model of csrc/sepaihrd_stoch_sepaihrd.inc with
    the row weights of csrc/sepaihrd_particle.inc.  alpha_k(x) = E[prod of the weights of rows <= k; state at row k = x].

    row is one model-values row in the RowLayout order: 8 scalars (theta, sigma, gamma_p, gamma_A, gamma_I, gamma_H, gamma_ICU,
    beta), nb beta values, nk kappa values, 8 vectors [n] (a, h_infec, p, h, icu, d_H, d_ICU, d_community), 11 initial counts [n]
    (S, E, P, A, I, H, ICU, R, D, CumH, CumICU).  obs_* [n_obs][n] belong to the output rows k = runup_offset + t.

    Only sums and products of non-negative float64 terms, a few hundred deep, the totals by math.fsum: the relative error of
    every returned number is below 1e-12.  Age classes without people are not part of the state and cost nothing."""
    row = [float(v) for v in np.asarray(row).ravel()]
    assert len(row) == NUM_SCALARS + nb + nk + (NUM_VECTORS + NUM_COMP) * n
    times = [float(t) for t in times]
    N = [float(v) for v in N]
    M = np.asarray(M, dtype=np.float64).reshape(n, n).tolist()
    obs = [np.asarray(o, dtype=np.float64).reshape(-1, n) for o in (obs_H, obs_ICU, obs_D)]
    beta_values, kappa_values = row[NUM_SCALARS:NUM_SCALARS + nb], row[NUM_SCALARS + nb:NUM_SCALARS + nb + nk]
    vec = lambda f, a: row[NUM_SCALARS + nb + nk + f * n + a]
    x0 = [[row[NUM_SCALARS + nb + nk + NUM_VECTORS * n + c * n + a] for c in range(NUM_POP)] for a in range(n)]
    assert all(v == int(v) and v >= 0 for xs in x0 for v in xs)
    ages = [a for a in range(n) if any(x0[a])]  # the classes that hold people
    T = len(times)

    def usable(series, k, a):
        t = k - runup_offset
        return 0 <= t < obs[series].shape[0] and bool(np.isfinite(obs[series][t, a]) and obs[series][t, a] >= 0.0)

    def log_term(series, k, a, inc):
        sim = max(0, inc) + SIM_FLOOR
        return obs[series][k - runup_offset, a] * math.log(sim) - sim

    @functools.lru_cache(maxsize=None)
    def compartment_outcomes(count, probs):
        return multinomial_outcomes(count, probs)

    @functools.lru_cache(maxsize=None)
    def class_step(a, x, p_inf, h):
        """{(state after the step, (new CumH, new CumICU, new D)): probability} of age class a from counts x"""
        gI, gH, gICU = row[GAMMA_I], row[GAMMA_H], row[GAMMA_ICU]
        hi, icu, dH, dICU, dC = vec(V_H, a), vec(V_ICU, a), vec(V_D_H, a), vec(V_D_ICU, a), vec(V_D_COMM, a)
        pP, to_A = pr(row[GAMMA_P], h), min(1.0, max(0.0, vec(V_P, a)))
        pI, to_H, to_D_I = pr(gI + hi + dC, h), share(hi, gI + dC), share(dC, gI)
        pH, to_ICU, to_D_H = pr(gH + dH + icu, h), share(icu, gH + dH), share(dH, gH)
        pICU, to_D_ICU = pr(gICU + dICU, h), share(dICU, gICU)
        parts = (compartment_outcomes(x[S_], (p_inf,)),
                 compartment_outcomes(x[E_], (pr(row[SIGMA], h),)),
                 compartment_outcomes(x[P_], (pP * to_A, pP * (1.0 - to_A))),
                 compartment_outcomes(x[A_], (pr(row[GAMMA_A], h),)),
                 compartment_outcomes(x[I_], (pI * to_H, pI * (1.0 - to_H) * to_D_I, pI * (1.0 - to_H) * (1.0 - to_D_I))),
                 compartment_outcomes(x[H_], (pH * to_ICU, pH * (1.0 - to_ICU) * to_D_H, pH * (1.0 - to_ICU) * (1.0 - to_D_H))),
                 compartment_outcomes(x[ICU_], (pICU * to_D_ICU, pICU * (1.0 - to_D_ICU))))
        out = {}
        for (s, ps), (e, pe), (pp, ppp), (aa, pa), (ii, pi), (hh, ph), (cc, pc) in itertools.product(*parts):
            y = (x[S_] - s[0], x[E_] + s[0] - e[0], x[P_] + e[0] - pp[0] - pp[1], x[A_] + pp[0] - aa[0], x[I_] + pp[1] - sum(ii),
                 x[H_] + ii[0] - sum(hh), x[ICU_] + hh[0] - sum(cc), x[R_] + aa[0] + ii[2] + hh[2] + cc[1], x[D_] + ii[1] + hh[1] + cc[0])
            key = (y, (ii[0], hh[0], ii[1] + hh[1] + cc[0]))
            out[key] = out.get(key, 0.0) + ps * pe * ppp * pa * pi * ph * pc
        return tuple(out.items())

    @functools.lru_cache(maxsize=None)
    def joint_step(xs, bk, h, tracked, discounted):
        """((states after the step, increments of the step in the cells `tracked`), probability times exp(-(the increments of the
        step in the cells `discounted`))) of all classes together from the joint counts xs; cells are (class slot, series)"""
        inf = {b: (x[P_] + x[A_] + row[THETA] * x[I_]) * vec(V_H_INFEC, b) * (1.0 / N[b] if N[b] > 0.0 else 0.0) for b, x in zip(ages, xs)}
        per_class = []
        for a, x in zip(ages, xs):
            lam = max(0.0, math.fsum(M[a][b] * inf[b] for b in ages) * (bk * vec(V_A, a)))
            per_class.append(class_step(a, x, pr(lam, h), h))
        out = {}
        for combo in itertools.product(*per_class):
            p = math.exp(-sum(combo[i][0][1][ser] for i, ser in discounted)) if discounted else 1.0
            for _, q in combo:
                p *= q
            key = (tuple(c[0][0] for c in combo), tuple(combo[i][0][1][ser] for i, ser in tracked))
            out[key] = out.get(key, 0.0) + p
        return tuple((ys, d, q) for (ys, d), q in out.items())

    slot = {a: i for i, a in enumerate(ages)}

    def cells_of(k):
        """the usable (series, age) cells of output row k"""
        return [(ser, a) for a in range(n) for ser in range(3) if k >= runup_offset and usable(ser, k, a)]

    def split(k):
        """The cells of row k by how their factor of the weight is formed.  An observed 0 gives exp(-(inc + 1e-10)), which is a
        product over the steps of the interval: exp(-d) joins each step's probability (`discounted`) and no increment need be
        carried.  An observed count > 0 needs the interval's increment (`tracked`).  A class without people has the increment 0:
        its cells, and the 1e-10 of the discounted ones, give the row one constant log-factor."""
        tracked, discounted, constant = [], [], []
        for ser, a in cells_of(k):
            y = obs[ser][k - runup_offset, a]
            if a not in slot:
                constant.append(log_term(ser, k, a, 0))
            elif y > 0.0:
                tracked.append((slot[a], ser))
            else:
                discounted.append((slot[a], ser))
                constant.append(-SIM_FLOOR)
        return tuple(tracked), tuple(discounted), math.fsum(constant)

    def weigh(alpha_inc, k, tracked, constant):
        """alpha over (states, increments of the interval in the cells `tracked`) -> alpha over states with the rest of the weight
        of row k folded in"""
        out = {}
        for (xs, inc), p in alpha_inc.items():
            lw = math.fsum([constant] + [log_term(ser, k, ages[i], v) for (i, ser), v in zip(tracked, inc)])
            out.setdefault(xs, []).append(p * math.exp(lw))
        return {xs: math.fsum(ps) for xs, ps in out.items()}

    alpha = {tuple(tuple(int(v) for v in x0[a]) for a in ages): 1.0}
    Z, z = [], 1.0
    any_usable = False
    if runup_offset == 0:  # the run's first row is observed: its increments are 0
        if cells_of(0):
            lw = math.fsum(log_term(ser, 0, a, 0) for ser, a in cells_of(0))
            alpha, any_usable = {xs: p * math.exp(lw) for xs, p in alpha.items()}, True
            z = math.fsum(alpha.values())
        Z.append(z)
    for k in range(1, T):
        h = (times[k] - times[k - 1]) / m
        tracked, discounted, constant = split(k)
        cur = {(xs, (0,) * len(tracked)): p for xs, p in alpha.items()}
        for j in range(m):
            t_mid = times[k - 1] + (j + 0.5) * h
            beta = schedule_value(beta_values, beta_ends, t_mid) if nb > 0 else row[BETA]
            bk = beta * schedule_value(kappa_values, kappa_ends, t_mid)
            nxt = {}
            for (xs, inc), p in cur.items():
                for ys, d, q in joint_step(xs, bk, h, tracked, discounted):
                    key = (ys, tuple(map(int.__add__, inc, d)))
                    nxt[key] = nxt.get(key, 0.0) + p * q
            cur = nxt
        if cells_of(k):
            alpha, any_usable = weigh(cur, k, tracked, constant), True
            z = math.fsum(alpha.values())
        else:
            alpha = {}
            for (xs, _), p in cur.items():
                alpha[xs] = alpha.get(xs, 0.0) + p
        if k >= runup_offset:
            Z.append(z)
    res = ExactResult()
    res.Z, res.states = np.array(Z), len(alpha)
    res.G = np.zeros((NUM_POP, n))
    for i, a in enumerate(ages):
        for c in range(NUM_POP):
            res.G[c, a] = math.fsum(p * xs[i][c] for xs, p in alpha.items())
    res.pmf = None
    if not any_usable:
        res.pmf = [[np.ones(1) for _ in range(n)] for _ in range(NUM_POP)]
        for i, a in enumerate(ages):
            people = int(sum(x0[a]))
            for c in range(NUM_POP):
                res.pmf[c][a] = np.array([math.fsum(p for xs, p in alpha.items() if xs[i][c] == v) for v in range(people + 1)])
    return res


# ---- the tiny epidemics
T_ROWS, RUNUP = 6, 1   # six output rows at times -1 .. 4, the first of them run-up
KAPPA_VALUES, KAPPA_ENDS = (1.0, 0.5, 0.7, 0.9), (0.4, 2.6, 111.0, 305.0)  # two kappa breakpoints inside the grid
BETA_ENDS = (1.6, 1e9)                                                      # and one of beta; no midpoint of m = 1, 2 meets one
NAN = float("nan")


class Tiny:
    """One tiny problem: the fields of the model, N, M, the initial counts and the observations [3][T_pos][n] (H, ICU, D).
    `rate` scales every rate, so that the m = 1 case keeps its per-step probabilities in the range of the m = 2 cases; `contact`
    scales M, whose entries grow with the row, so that a susceptible of class 7 is infected with a probability of a few tenths
    per step like everybody else."""

    def __init__(self, name, n, m, J, people, obs, rate=1.0, contact=1.0):
        self.name, self.n, self.m, self.J = name, n, m, J
        age = np.arange(n, dtype=np.float64)
        self.scalars = dict(beta=0.05, theta=0.6, sigma=1.0 * rate, gamma_p=1.2 * rate, gamma_A=0.8 * rate, gamma_I=0.5 * rate, gamma_H=0.4 * rate,
                            gamma_ICU=0.5 * rate)
        self.vectors = dict(a=0.8 + 0.03 * age, h_infec=1.1 - 0.02 * age, p=0.3 + 0.02 * age, h=(0.4 + 0.01 * age) * rate,
                            icu=(0.5 - 0.01 * age) * rate, d_H=(0.2 + 0.005 * age) * rate, d_ICU=(0.5 + 0.01 * age) * rate,
                            d_community=(0.15 + 0.005 * age) * rate)
        self.beta_values = (2.5 * rate, 4.0 * rate)   # the schedule; the scalar beta of the row is not read where there is one
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        self.M = contact * (0.5 + (16 * i + (5 * j + 3) % 16) / 64.0)   # dense, asymmetric, every entry distinct
        assert len(set(self.M.ravel())) == n * n
        self.x0 = np.zeros((11, n))
        for a, counts in people.items():
            for comp, v in counts.items():
                self.x0[COMP_NAMES.index(comp), a] = v
        self.N = self.x0[:NUM_POP].sum(axis=0)   # 0 for a class without people
        self.times = np.arange(T_ROWS, dtype=np.float64) - RUNUP
        self.Tp = T_ROWS - RUNUP
        self.obs = np.zeros((3, self.Tp, n))
        for (ser, t, a), v in obs.items():
            self.obs[ser, t, a] = v
        self.blank_row = 3
        self.obs[:, self.blank_row] = NAN        # a row without a usable cell
        self.occupied = sorted(people)

    def row(self, mm):
        return mm.hostabi.stochastic_pack_values(self.n, self.x0, beta_values=self.beta_values, kappa_values=KAPPA_VALUES, **self.scalars,
                                                 **self.vectors)

    def exact(self, row, obs=None):
        ob = self.obs if obs is None else obs
        return exact_of(np.asarray(row, dtype=np.float64).tobytes(), self.n, self.m, self.M.tobytes(), self.N.tobytes(), ob.tobytes())

    def filter(self, mm, B, seed, J=None, obs=None, want_final=True):
        ob = self.obs if obs is None else obs
        rows = np.stack([self.row(mm)] * B)
        return mm.hostabi.particle_from_values(rows, np.zeros(B, dtype=np.int32), self.times, self.N, self.M, KAPPA_ENDS, ob[0], ob[1], ob[2],
                                               self.J if J is None else J, self.m, seed, beta_end_times=BETA_ENDS, want_final=want_final)

    def paths(self, mm, S, R, seed):
        rows = np.stack([self.row(mm)] * S)
        return mm.hostabi.stochastic_from_values(rows, np.zeros(S, dtype=np.int32), self.times, self.N, self.M, KAPPA_ENDS, R, self.m, seed, [0.5],
                                                 beta_end_times=BETA_ENDS)


@functools.lru_cache(maxsize=None)
def exact_of(row, n, m, M, N, obs):
    """exact_filter once per (row, problem, observations): the CPU and the GPU tests of a case share the result"""
    ob = np.frombuffer(obs).reshape(3, -1, n)
    return exact_filter(np.frombuffer(row), n, len(BETA_ENDS), len(KAPPA_VALUES), np.arange(T_ROWS, dtype=np.float64) - RUNUP, np.frombuffer(N),
                        np.frombuffer(M).reshape(n, n), BETA_ENDS, KAPPA_ENDS, m, RUNUP, ob[0], ob[1], ob[2])


H_SER, ICU_SER, D_SER = 0, 1, 2
# Observations are {(series, t, age): count}, 0 elsewhere; row 3 is blank in every case.  The counts are 0, 1 and 2, placed where
# the exact recursion gives such a row a probability of a few tenths, so that the weights do not degenerate.
CASES = {
    # five people in one class; m = 1 with every rate halved
    "n1": Tiny("n1", 1, 1, 64, {0: dict(S=2, E=1, I=1, H=1)},
               {(H_SER, 0, 0): 1, (ICU_SER, 1, 0): 1, (D_SER, 2, 0): NAN, (D_SER, 4, 0): 2}, rate=0.5),
    # four people in three classes, the last two of them in late compartments only; four lanes per particle on the device, one of
    # them padding; J above the 128 particles of a pass.  Counts above 0 are observed only in the class with two people: where one
    # person is all a class has, such a count would fix that person's path and leave G of some compartment at 1e-10 of the rest
    "n3": Tiny("n3", 3, 2, 130, {0: dict(S=1, E=1), 1: dict(I=1), 2: dict(H=1)},
               {(ICU_SER, 0, 2): NAN, (H_SER, 2, 0): 1, (ICU_SER, 4, 0): 2}),
    # four people in the classes 0, 7 and 15 of sixteen, the other thirteen empty with N = 0; J above the 32 particles of a pass
    "n16": Tiny("n16", 16, 2, 34, {0: dict(S=1), 7: dict(S=1, P=1), 15: dict(I=1)},
                {(D_SER, 0, 3): NAN, (H_SER, 1, 7): 1, (D_SER, 2, 15): NAN, (ICU_SER, 2, 7): 2}, contact=0.4),
}
ESTIMATES = {"n1": (1024, 8), "n3": (1024, 8), "n16": (1024, 16)}   # (B positions, K seeds): E = B K independent estimates
SEED = 0x5EED_0F_7E57


@functools.lru_cache(maxsize=None)
def estimates_of(mm, name):
    """E = B K runs of the filter of a case: increments [E][T_pos], loglik [E], the particle mean of the final counts [E][9][n],
    their maximum over all particles [9][n]"""
    case = CASES[name]
    B, K = ESTIMATES[name]
    inc, ll, mean, top = [], [], [], np.zeros((NUM_POP, case.n))
    for k in range(K):
        got = case.filter(mm, B, SEED + k)
        inc.append(got["increments"])
        ll.append(got["loglik"])
        mean.append(got["final_state"][:, :, :NUM_POP].mean(axis=1))
        top = np.maximum(top, got["final_state"][:, :, :NUM_POP].max(axis=(0, 1)))
    return np.concatenate(inc), np.concatenate(ll), np.concatenate(mean), top


def check_prefix_likelihoods(name, increments, Z):
    """mean of exp(cumsum(increments)[k] - log Z[k]) against 1 for every k: |z| < 5, relative standard error <= 0.05"""
    ratio = np.exp(np.cumsum(increments, axis=1) - np.log(Z))
    mean, se = ratio.mean(axis=0), ratio.std(axis=0, ddof=1) / math.sqrt(ratio.shape[0])
    z = (mean - 1.0) / se
    for k in range(len(Z)):
        print(f"{name} prefix {k}: Z {Z[k]:.6e}, estimate / exact {mean[k]:.4f} +- {se[k]:.4f}, z {z[k]:+.2f}")
    assert (se <= 0.05).all(), se
    assert (np.abs(z) < 5.0).all(), z
    return z


def check_final_moments(name, loglik, particle_mean, top, G):
    """mean of exp(loglik) mean_j final_state[j][c][a] against G[c][a] wherever G > 0: |z| < 5, relative standard error <= 0.05;
    where G is exactly 0, no particle has anybody there"""
    est = np.exp(loglik)[:, None, None] * particle_mean
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(est.shape[0])
    worst = 0.0
    for c, a in itertools.product(range(NUM_POP), range(G.shape[1])):
        if G[c, a] == 0.0:
            assert top[c, a] == 0.0, (c, a)
            continue
        z = (mean[c, a] - G[c, a]) / se[c, a]
        print(f"{name} {COMP_NAMES[c]}[{a}]: G {G[c, a]:.6e}, estimate / exact {mean[c, a] / G[c, a]:.4f} +- {se[c, a] / G[c, a]:.4f}, z {z:+.2f}")
        assert se[c, a] / G[c, a] <= 0.05, (c, a, se[c, a] / G[c, a])
        assert abs(z) < 5.0, (c, a, z)
        worst = max(worst, abs(z))
    return worst


def check_against_pmf(name, what, final, pmf, occupied):
    """final [samples][>= 9][n] counts against the exact marginal pmf of every compartment: the project's bar for samplers,
    p >= 1e-6 and |z| of the mean <= 6; classes without people hold nobody"""
    n = final.shape[2]
    for a in range(n):
        if a not in occupied:
            assert not final[:, :, a].any(), a
            continue
        for c in range(NUM_POP):
            p, z = chi_square_against_pmf(final[:, c, a], pmf[c][a])
            print(f"{name} {what} {COMP_NAMES[c]}[{a}]: p {p:.3g}, z of the mean {z:+.2f}, pmf {np.round(pmf[c][a], 4)}")
            assert p >= 1e-6 and abs(z) <= 6.0, (what, c, a, p, z)


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_what_it_claims(mm, name):
    case = CASES[name]
    ob = case.obs
    used = np.isfinite(ob) & (ob >= 0)
    assert case.x0[:NUM_POP].sum() <= 6 and set(np.unique(ob[used])) == {0.0, 1.0, 2.0}
    assert np.isnan(np.delete(ob, case.blank_row, axis=1)).sum() >= 1 and not used[:, case.blank_row].any()
    assert used.any(axis=(0, 2)).sum() == case.Tp - 1
    assert sorted(np.nonzero(case.N)[0]) == case.occupied and (case.N[[a for a in range(case.n) if a not in case.occupied]] == 0).all()
    assert case.times[0] < 0.0 <= case.times[1] and 0.0 < BETA_ENDS[0] < case.times[-1] and 0.0 < KAPPA_ENDS[0] < KAPPA_ENDS[1] < case.times[-1]
    assert CASES["n1"].m == 1 and CASES["n3"].m == CASES["n16"].m == 2
    assert CASES["n3"].J > 128 and CASES["n16"].J > 32 and CASES["n1"].J == 64
    assert case.J <= mm.hostabi.particle_max_particles(case.n)
    # every outflow probability of a step lies in the regime where a count of 0, 1 or 2 changes: 0.15 .. 0.55
    h = 1.0 / case.m
    s, v = case.scalars, case.vectors
    rates = [np.full(case.n, s["sigma"]), np.full(case.n, s["gamma_p"]), np.full(case.n, s["gamma_A"]), s["gamma_I"] + v["h"] + v["d_community"],
             s["gamma_H"] + v["d_H"] + v["icu"], s["gamma_ICU"] + v["d_ICU"]]
    prob = -np.expm1(-np.array(rates) * h)
    assert prob.min() > 0.15 and prob.max() < 0.55, (prob.min(), prob.max())


@pytest.mark.parametrize("name", list(CASES))
def test_prefix_likelihoods_are_unbiased_for_the_exact_ones(mm, name):
    """exp of the running sum of the increments estimates Z[k], the exact expectation of the product of the row weights up to
    row k, without bias: see check_prefix_likelihoods"""
    case = CASES[name]
    exact = case.exact(case.row(mm))
    inc, _, _, _ = estimates_of(mm, name)
    assert exact.Z[case.blank_row] == exact.Z[case.blank_row - 1] and not inc[:, case.blank_row].any()
    print(f"{name}: {exact.states} final states, E = {inc.shape[0]}, J = {case.J}")
    check_prefix_likelihoods(name, inc, exact.Z)


@pytest.mark.parametrize("name", list(CASES))
def test_final_state_moments_are_unbiased_for_the_exact_ones(mm, name):
    """exp(loglik) times the particle mean of a final count estimates G = sum_x alpha(x) x without bias: see check_final_moments"""
    case = CASES[name]
    exact = case.exact(case.row(mm))
    _, ll, mean, top = estimates_of(mm, name)
    assert (exact.G[:, case.occupied] > 0).sum() >= 5 * len(case.occupied) and not exact.G[:, [a for a in range(case.n) if a not in case.occupied]].any()
    check_final_moments(name, ll, mean, top, exact.G)


@pytest.mark.parametrize("name", list(CASES))
def test_unweighted_run_has_the_exact_final_distribution(mm, name):
    """no usable observation: the filter is the plain ensemble and so is stochastic_from_values; the final counts of either
    follow the exact marginal pmf of every compartment"""
    case = CASES[name]
    blank = np.full_like(case.obs, NAN)
    exact = case.exact(case.row(mm), blank)
    assert exact.pmf is not None and (exact.Z == 1.0).all()
    for a in case.occupied:
        for c in range(NUM_POP):
            assert abs(exact.pmf[c][a].sum() - 1.0) < 1e-12
    B = 256
    got = case.filter(mm, B, SEED + 100, obs=blank)
    assert not got["loglik"].any()
    check_against_pmf(name, "filter", got["final_state"].reshape(B * case.J, 11, case.n), exact.pmf, case.occupied)
    ens = case.paths(mm, B, case.J, SEED + 101)
    check_against_pmf(name, "ensemble", ens["final_state"].reshape(B * case.J, 11, case.n), exact.pmf, case.occupied)
