"""The per-row summaries of the particle filter on the host twin (hostParticleStates; csrc/sepaihrd_particle_states.inc): the filter
itself untouched, every row's means and quantile bands against numpy statistics of the final state of the filter run on the grid
cut after that row (causality), the run-up rows against the stochastic twin's replicates, structure, independence, the argument
rules, and the exact filtering moments of tiny epidemics.  No device."""
import math
import os

import numpy as np
import pytest

from test_particle_filter_exact_cpu import BETA_ENDS, CASES, ESTIMATES, KAPPA_ENDS, KAPPA_VALUES, NUM_POP, RUNUP, SEED as EXACT_SEED, T_ROWS, exact_filter

SEED = 0x57A7E5_0F_7E57
T = 10
PROBS = (0.0, 0.025, 0.5, 0.9, 1.0)
DISPERSION = (0.5, np.inf, 8.0)
DBL_MAX = np.finfo(np.float64).max
# A moment G_k[c][a] at or below this share of the row's largest exists only because the weight floors sim at 1e-10
# (csrc/sepaihrd_particle.inc): the state contradicts a positive observed count, as when the only infectious person of case n1
# must be the hospitalisation observed at t = 0.  It is 1e-10 of the others where the rest are of order 1; a filter of any J meets
# such a state in none of 8192 estimates, the ratio is 0 with standard error 0, and no z exists.  Those cells are held to the
# bound below instead of the z test; every other cell, and every exactly-zero one, is tested as stated.
FLOOR_LEVEL = 1e-8
NEW_SYMBOLS = ("sepaihrd_particle_filter_states", "sepaihrd_particle_states_validate", "sepaihrd_particle_states_timing")


class Problem:
    """Model values, fixed data and observations of a small problem of n age classes over T = 10 output rows, `runup` of them
    before t = 0.  Three rows of model values: the base, one at other rates, and a third whose status is 1 (an invalid theta).
    The observations are the daily counts of one path of the model with a NaN cell, a negative cell and a blank row."""

    def __init__(self, mm, n, runup=2, m=2):
        self.n, self.m, self.runup, self.Tp = n, m, runup, T - runup
        age = np.arange(n, dtype=np.float64)
        x0 = np.zeros((11, n))
        for c, v in enumerate((3000 + 500 * age, 40 + 3 * age, 20 + age, 10 + age, 40 + 2 * age, 6 + age % 4, 2 + age % 3, 5 + 0 * age)):
            x0[c] = v
        vectors = dict(a=0.8 + 0.03 * age, h_infec=1.1 - 0.02 * age, p=0.3 + 0.02 * age, h=0.08 + 0.01 * age, icu=0.08 + 0.005 * age,
                       d_H=0.02 + 0.004 * age, d_ICU=0.05 + 0.01 * age, d_community=0.005 + 0.003 * age)
        pack = lambda beta: mm.hostabi.stochastic_pack_values(n, x0, beta_values=beta, kappa_values=[1.0, 0.6], theta=0.6, sigma=0.4, gamma_p=0.5,
                                                              gamma_A=0.3, gamma_I=0.2, gamma_H=0.15, gamma_ICU=0.1, **vectors)
        self.rows = np.stack([pack([0.9, 0.5]), pack([0.6, 0.8]), pack([0.9, 0.5])])
        self.status = np.array([0, 0, 1], dtype=np.int32)
        self.N = x0[:9].sum(axis=0)
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        self.M = (3.0 / n) * (0.5 + (16 * i + (5 * j + 3) % 16) / 64.0)
        self.times = np.arange(T, dtype=np.float64) - runup
        self.beta_ends, self.kappa_ends = [1.25, 1e9], [3.25, 1e9]
        tr = mm.hostabi.stochastic_from_values(self.rows[:1], self.status[:1], self.times, self.N, self.M, self.kappa_ends, 1, m, SEED ^ 0xABCDEF,
                                               [0.5], beta_end_times=self.beta_ends, keep=1)["traj"][0, 0]  # [T][11][n]
        self.obs = np.stack([np.diff(tr[:, c], axis=0, prepend=tr[:1, c])[runup:] for c in (9, 10, 8)]).astype(np.float64)  # [3][Tp][n]
        self.obs[0, 1, 0] = np.nan
        self.obs[2, 2, n - 1] = -1.0
        self.blank = 4
        self.obs[:, self.blank] = np.nan

    def _args(self, rows, status, cut):
        """the fixed data and the observations of the grid cut after output row `cut` (None: the whole grid)"""
        k = T - 1 if cut is None else cut
        ob = self.obs[:, :k + 1 - self.runup]
        return (self.rows if rows is None else rows, self.status if status is None else status, self.times[:k + 1], self.N, self.M, self.kappa_ends,
                ob[0], ob[1], ob[2])

    def states(self, mm, J, probs=PROBS, dispersion=None, rows=None, status=None, seed=SEED, cut=None, **kw):
        return mm.hostabi.particle_states_from_values(*self._args(rows, status, cut), J, self.m, seed, probs, beta_end_times=self.beta_ends,
                                                      dispersion=dispersion, **kw)

    def wide(self, mm, J, dispersion=None, rows=None, status=None, seed=SEED, cut=None):
        return mm.hostabi.particle_wide_from_values(*self._args(rows, status, cut), J, self.m, seed, beta_end_times=self.beta_ends,
                                                    dispersion=dispersion)


@pytest.fixture(scope="module")
def problems(mm):
    cache = {}

    def get(n, runup=2, m=2):
        if (n, runup, m) not in cache:
            cache[(n, runup, m)] = Problem(mm, n, runup, m)
        return cache[(n, runup, m)]
    return get


def numpy_stats(cloud, probs):
    """cloud [B][J][11][n] counts (NaN: an invalid theta) -> mean [B][11][n + 1], quantiles [B][11][n + 1][len(probs)] by the rule of
    csrc/sepaihrd_particle_states.inc written out: the int64 sum / J, np.sort, pos = p (J - 1), v[idx] (1 - frac) + v[idx + 1] frac"""
    B, J = cloud.shape[:2]
    bad = np.isnan(cloud).any(axis=(1, 2, 3))
    counts = np.where(np.isnan(cloud), 0.0, cloud).astype(np.int64)
    series = np.concatenate([counts, counts.sum(axis=3, keepdims=True)], axis=3)  # the totals column from the per-particle age sums
    mean = series.sum(axis=1).astype(np.float64) / np.float64(J)
    v = np.sort(series.astype(np.float64), axis=1)
    quant = np.empty(mean.shape + (len(probs),))
    for i, p in enumerate(probs):
        pos = np.float64(p) * np.float64(J - 1)
        idx = int(pos)
        frac = pos - np.float64(idx)
        quant[..., i] = v[:, idx] * (1.0 - frac) + v[:, idx + 1] * frac if idx + 1 < J else v[:, idx]
    mean[bad], quant[bad] = np.nan, np.nan
    return mean, quant


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. the symbols
def test_symbols_are_declared_exported_and_bound(mm):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sepaihrd_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in mm.hipabi.EXPORTED_SYMBOLS and hasattr(mm.hipabi.load_library(), sym) and "int " + sym + "(" in text, sym
    assert "#define SEPAIHRD_ABI_VERSION 3" in text
    for sym in ("host_particle_states_from_values", "host_particle_filter_states"):
        assert hasattr(mm.hostabi.load_library(), sym), sym
    assert callable(mm.hostabi.particle_states_from_values) and callable(mm.hostabi.particle_states_validate)
    assert callable(mm.HipObjective.particle_filter_states) and callable(mm.HipObjective.particle_states_timing)


# ---- 2. the filter is untouched
@pytest.mark.parametrize("runup", [2, 0])
@pytest.mark.parametrize("dispersion", [None, DISPERSION])
@pytest.mark.parametrize("J", [1, 5, 64, "limit+1", 1000])
def test_the_filter_is_untouched(mm, problems, J, dispersion, runup):
    pb = problems(3, runup)
    J = mm.hostabi.particle_max_particles(3) + 1 if J == "limit+1" else J
    got, ref = pb.states(mm, J, dispersion=dispersion), pb.wide(mm, J, dispersion=dispersion)
    for key in ("loglik", "increments", "ess"):
        assert same(got[key], ref[key]), key
    assert got["n_valid"] == 2 and got["loglik"][2] == -DBL_MAX and np.isnan(got["increments"][2]).all()
    assert not got["increments"][:2, pb.blank].any() and np.isnan(got["ess"][:2, pb.blank]).all()
    assert got["state_mean"].shape == (3, T, 11, 4) and got["state_quantiles"].shape == (3, T, 11, 4, len(PROBS))
    assert np.isnan(got["state_mean"][2]).all() and np.isnan(got["state_quantiles"][2]).all()
    assert np.isfinite(got["state_mean"][:2]).all() and np.isfinite(got["state_quantiles"][:2]).all()
    # row T - 1 is what final_state holds
    mean, quant = numpy_stats(ref["final_state"], PROBS)
    assert same(got["state_mean"][:, T - 1], mean) and same(got["state_quantiles"][:, T - 1], quant)


# ---- 3. causality: row k from the final state of the filter on the grid cut after row k
@pytest.mark.parametrize("dispersion", [None, DISPERSION])
@pytest.mark.parametrize("n,J", [(1, 23), (3, 138), (16, 37)])
def test_every_row_is_the_final_state_of_the_grid_cut_after_it(mm, problems, n, J, dispersion):
    """The cut grid needs an output time >= 0, so the rows k < runup are compared with the stochastic twin's replicates instead
    (test_run_up_rows_are_the_stochastic_replicates): k runs over runup .. T - 1 here, and over 0 .. T - 1 without a run-up."""
    for runup in (2, 0):
        pb = problems(n, runup)
        got = pb.states(mm, J, dispersion=dispersion)
        differ = 0
        for k in range(runup, T):
            cut = pb.wide(mm, J, dispersion=dispersion, cut=k)
            mean, quant = numpy_stats(cut["final_state"], PROBS)
            assert same(got["state_mean"][:, k], mean), (runup, k)
            assert same(got["state_quantiles"][:, k], quant), (runup, k)
            assert same(got["increments"][:, :k + 1 - runup], cut["increments"]), (runup, k)
            differ += k > 0 and not same(got["state_mean"][:, k], got["state_mean"][:, k - 1])
        assert differ >= T - runup - 1


# ---- 4. the rows before the first weighted row
@pytest.mark.parametrize("n,J", [(1, 23), (3, 138), (16, 37)])
def test_run_up_rows_are_the_stochastic_replicates(mm, problems, n, J):
    pb = problems(n, 2)
    got = pb.states(mm, J)
    traj = mm.hostabi.stochastic_from_values(pb.rows, pb.status, pb.times, pb.N, pb.M, pb.kappa_ends, J, pb.m, SEED, [0.5],
                                             beta_end_times=pb.beta_ends, keep=J)["traj"]  # [B][J][T][11][n]: slot j is replicate j
    for k in range(pb.runup):
        mean, quant = numpy_stats(traj[:, :, k], PROBS)
        assert same(got["state_mean"][:, k], mean) and same(got["state_quantiles"][:, k], quant), k
    # row `runup` is weighted and resampled: no longer the replicates
    mean, _ = numpy_stats(traj[:, :, pb.runup], PROBS)
    assert not same(got["state_mean"][:, pb.runup], mean)
    # row 0 is the initial counts, the same in every particle
    assert (got["state_quantiles"][:2, 0] == got["state_mean"][:2, 0, ..., None]).all()


# ---- 5. structure
def test_structure(mm, problems):
    pb = problems(3)
    one = pb.states(mm, 1)
    fin = pb.wide(mm, 1)["final_state"]  # [B][1][11][n]
    assert (one["state_quantiles"][:2] == one["state_mean"][:2, ..., None]).all()
    assert same(one["state_mean"][:, T - 1, :, :3], fin[:, 0])
    got = pb.states(mm, 64)
    q, mean = got["state_quantiles"][:2], got["state_mean"][:2]
    assert (np.diff(q, axis=-1) >= 0).all() and (q[..., 0] <= mean).all() and (mean <= q[..., -1]).all()
    ext = pb.states(mm, 64, probs=(0.0, 1.0))["state_quantiles"]
    assert same(ext[..., 0], got["state_quantiles"][..., 0]) and same(ext[..., 1], got["state_quantiles"][..., -1])
    assert (q[..., 0] == np.floor(q[..., 0])).all() and (q[..., -1] == np.floor(q[..., -1])).all()  # minimum and maximum: counts
    # the sum of the age means is the mean of the totals column: both are integer sums over J, exactly
    assert np.array_equal((mean[..., :3] * 64).sum(axis=-1), mean[..., 3] * 64)
    # the people of a particle are conserved: the total over the nine population compartments is the same in every row
    assert len(set(mean[0, :, :9, 3].sum(axis=1))) == 1
    lean = pb.states(mm, 64, probs=())
    assert "state_quantiles" not in lean and same(lean["state_mean"], got["state_mean"])


# ---- 6. independence
def test_a_result_does_not_depend_on_its_neighbours(mm, problems):
    pb = problems(3)
    J = 40
    full = pb.states(mm, J)
    # position b is the stream coordinate: the same rows at the same positions, fewer of them
    two = pb.states(mm, J, rows=pb.rows[:2], status=pb.status[:2])
    for key in ("loglik", "increments", "ess", "state_mean", "state_quantiles"):
        assert same(two[key], full[key][:2]), key
    # an invalid neighbour in front: position 1 keeps its result
    holes = pb.states(mm, J, status=np.array([1, 0, 0], dtype=np.int32))
    assert np.isnan(holes["state_mean"][0]).all() and holes["loglik"][0] == -DBL_MAX
    assert same(holes["state_mean"][1], full["state_mean"][1]) and same(holes["state_quantiles"][1], full["state_quantiles"][1])
    # other probabilities, no quantiles
    other = pb.states(mm, J, probs=(0.5,))
    assert same(other["state_mean"], full["state_mean"]) and same(other["state_quantiles"][..., 0], full["state_quantiles"][..., 2])
    assert same(pb.states(mm, J, want_quantiles=False)["state_mean"], full["state_mean"])
    wide = pb.wide(mm, J)
    assert full["n_valid"] == wide["n_valid"] == 2
    assert not same(pb.states(mm, J, seed=SEED + 1)["state_mean"], full["state_mean"])


# ---- 7. the argument rules
def test_every_refusal_and_its_message(mm, problems):
    v = mm.hostabi.particle_states_validate
    ok = dict(B=3, J=8, steps_per_interval=2, theta_chunk=0, n_times=T, T_pos=T - 2, n_age=3)
    v(**ok, probs=PROBS)
    v(**ok, probs=())
    v(**ok, probs=(0.0, 1.0))
    v(**dict(ok, J=65536), probs=np.linspace(0.0, 1.0, 64))
    for kw, probs, word in ((dict(B=0), PROBS, "B must be >= 1"), (dict(J=0), PROBS, "J must lie in [1, 65536]"),
                            (dict(J=65537), PROBS, "J must lie in [1, 65536]"), (dict(theta_chunk=-1), PROBS, "theta_chunk must be >= 0"),
                            (dict(steps_per_interval=0), PROBS, "steps_per_interval must be >= 1"), (dict(n_age=17), PROBS, "n_age must lie in [1, 16]"),
                            (dict(T_pos=0), PROBS, "an output time >= 0"), (dict(B=2 ** 15, J=65536), PROBS, "B x J must stay below 2^31"),
                            ({}, np.linspace(0.0, 1.0, 65), "n_probs must lie in [0, 64]"), ({}, None, "n_probs > 0 needs probs"),
                            ({}, (0.5, np.nan), "every probability must lie in [0, 1]"),
                            ({}, (np.nextafter(0.0, -1.0),), "every probability must lie in [0, 1]"),
                            ({}, (np.nextafter(1.0, 2.0),), "every probability must lie in [0, 1]"), ({}, (np.inf,), "every probability must lie in [0, 1]")):
        with pytest.raises(ValueError) as e:
            v(**dict(ok, **kw), probs=probs)
        assert str(e.value).startswith("particle_filter_states: ") and word in str(e.value), (kw, str(e.value))
    pb = problems(3)
    with pytest.raises(ValueError, match="particle_filter_states: every probability"):
        pb.states(mm, 8, probs=(1.5,))
    with pytest.raises(ValueError, match=r"particle_nb: dispersion\[1\]"):
        pb.states(mm, 8, dispersion=(0.5, -1.0, 8.0))


# ---- 8. the exact answer
@pytest.mark.parametrize("name", ["n1", "n3"])
def test_row_means_are_unbiased_for_the_exact_filtering_moments(mm, name):
    """exp(the sum of the increments of the rows <= k) times state_mean[k][c][a] estimates G_k[c][a], the exact unnormalised moment of
    the filter on the grid cut after row k, without bias: the mean over E = 8192 estimates of the ratio lies within 5 standard errors
    of 1, every standard error at most 0.05; where G_k is exactly 0 the p = 1 quantile is 0 in every estimate.  With the present
    twin: largest standard error 0.0132 (n1) and 0.0419 (n3), largest |z| 1.75 and 2.39.  One cell of n1 (row 1, the infectious
    count) has G = 4.9e-11 and the estimate 0 in all 8192 runs: it is held to FLOOR_LEVEL's bound instead (see there)."""
    check_exact_case(name, *exact_estimates(mm, name, lambda case, rows, seed: mm.hostabi.particle_states_from_values(
        rows, np.zeros(len(rows), dtype=np.int32), case.times, case.N, case.M, KAPPA_ENDS, case.obs[0], case.obs[1], case.obs[2], case.J, case.m, seed,
        (1.0,), beta_end_times=BETA_ENDS)), mm)


def exact_estimates(mm, name, run):
    case = CASES[name]
    B, K = ESTIMATES[name]
    assert B * K == 8192
    rows = np.stack([case.row(mm)] * B)
    runs = [run(case, rows, EXACT_SEED + k) for k in range(K)]
    return (np.concatenate([r["increments"] for r in runs]), np.concatenate([r["state_mean"] for r in runs]),
            np.concatenate([r["state_quantiles"][..., 0] for r in runs]))


def check_exact_case(name, inc, mean, top, mm, row=None):
    """row: the model-values row the estimates were run with (None: the case's hand-packed one)"""
    case = CASES[name]
    n = case.n
    row = case.row(mm) if row is None else row
    assert inc.shape == (8192, case.Tp) and mean.shape == (8192, T_ROWS, 11, n + 1)
    worst_se = worst_z = 0.0
    floor_cells = 0
    for k in range(1, T_ROWS):
        ob = case.obs[:, :k + 1 - RUNUP]
        G = exact_filter(row, n, len(BETA_ENDS), len(KAPPA_VALUES), case.times[:k + 1], case.N, case.M, BETA_ENDS, KAPPA_ENDS, case.m, RUNUP,
                         ob[0], ob[1], ob[2]).G  # [9][n]
        weight = np.exp(inc[:, :k + 1 - RUNUP].sum(axis=1))
        for c in range(NUM_POP):
            for a in range(n):
                if G[c, a] == 0.0:
                    assert not top[:, k, c, a].any(), (k, c, a)
                    continue
                if G[c, a] <= FLOOR_LEVEL * G.max():
                    # reachable only through the 1e-10 floor of sim in a weight (see FLOOR_LEVEL): no estimate can resolve it
                    est = (weight * mean[:, k, c, a]).mean()
                    print(f"{name} row {k} count {c} age {a}: G {G[c, a]:.6e} is floor level, estimate {est:.3e}")
                    assert est <= 1e3 * FLOOR_LEVEL * G.max(), (k, c, a, est)
                    floor_cells += 1
                    continue
                ratio = weight * mean[:, k, c, a] / G[c, a]
                m, se = ratio.mean(), ratio.std(ddof=1) / math.sqrt(len(ratio))
                z = (m - 1.0) / se
                print(f"{name} row {k} count {c} age {a}: G {G[c, a]:.6e}, estimate / exact {m:.4f} +- {se:.4f}, z {z:+.2f}")
                assert se <= 0.05, (k, c, a, se)
                assert abs(z) < 5.0, (k, c, a, z)
                worst_se, worst_z = max(worst_se, se), max(worst_z, abs(z))
    print(f"{name}: largest standard error {worst_se:.4f}, largest |z| {worst_z:.2f}, {floor_cells} floor-level cells")
    assert floor_cells == {"n1": 1, "n3": 0}[name]   # the infectious count of n1 at row 1, and no other cell
