"""The bootstrap particle filter of the stochastic SEPAIHRD model on the host twin (hostParticleLoglik, hostParticleResample),
with hand-made model values: a single particle against the stochastic twin's replicate 0, the slots before the first resampling,
the resampling rule on random and adversarial log-weights, unbiasedness across particle counts, unusable observations, invalid
parameter vectors, independence of the call around a position, and the argument rules.  No device."""
import math
import os

import numpy as np
import pytest

SEED = 0x0DDB_A11_5EED_1234
S_, E_, P_, A_, I_, H_, ICU_, R_, D_, CUMH_, CUMICU_ = range(11)
POP = [S_, E_, P_, A_, I_, H_, ICU_, R_, D_]
DBL_MAX = np.finfo(np.float64).max
RESAMPLE_J = (1, 2, 5, 64, 257)


def initial(n, **counts):
    x = np.zeros((11, n))
    for name, v in counts.items():
        x[{"S": 0, "E": 1, "P": 2, "A": 3, "I": 4, "H": 5, "ICU": 6, "R": 7, "D": 8}[name]] = v
    return x


class Case:
    """model values, fixed data and observations of one tiny problem; the observations are the daily counts of one path of the
    model itself (replicate 0 at another seed), so that they are as probable as data can be"""

    def __init__(self, mm, n=3, T=10, runup=2, m=2):
        self.n, self.m = n, m
        x0 = initial(n, S=[9000, 15000, 7000][:n], E=[40, 60, 30][:n], P=[20, 20, 20][:n], A=[10, 15, 20][:n], I=[40, 30, 50][:n],
                     H=[6, 4, 9][:n], ICU=[2, 1, 3][:n], R=[5, 5, 5][:n])
        self.row = mm.hostabi.stochastic_pack_values(
            n, x0, beta_values=[0.9, 0.5], kappa_values=[1.0, 0.6], theta=0.6, sigma=0.4, gamma_p=0.5, gamma_A=0.3, gamma_I=0.2, gamma_H=0.15,
            gamma_ICU=0.1, a=[0.8, 1.0, 1.2][:n], h_infec=[1.0, 0.9, 1.1][:n], p=[0.5, 0.4, 0.3][:n], h=[0.08, 0.12, 0.2][:n],
            icu=[0.08, 0.1, 0.15][:n], d_H=[0.02, 0.04, 0.08][:n], d_ICU=[0.05, 0.1, 0.2][:n], d_community=[0.005, 0.01, 0.05][:n])
        self.N = x0[POP].sum(axis=0)
        self.M = np.array([[3.0, 1.0, 0.5], [1.0, 2.0, 1.0], [0.5, 1.0, 1.5]])[:n, :n]
        self.times = np.arange(T, dtype=np.float64) - runup  # `runup` rows of run-up, then the observed ones
        self.runup, self.T, self.Tp = runup, T, T - runup
        self.beta_ends, self.kappa_ends = [1.25, 1e9], [3.25, 1e9]  # no midpoint of m = 1, 2, 3 meets them
        tr = self.paths(mm, 1, SEED ^ 0xABCDEF)["traj"][0, 0]     # [T][11][n]
        self.obs = self.daily(tr)[:, runup:].astype(np.float64)     # [3][Tp][n]: H, ICU, D

    def paths(self, mm, R, seed, rows=None, status=None):
        rows = np.atleast_2d(self.row if rows is None else rows)
        st = np.zeros(rows.shape[0], dtype=np.int32) if status is None else status
        return mm.hostabi.stochastic_from_values(rows, st, self.times, self.N, self.M, self.kappa_ends, R, self.m, seed, [0.5],
                                                 beta_end_times=self.beta_ends, keep=R)

    @staticmethod
    def daily(tr):
        """increments of CumH, CumICU and D since the previous output row, 0 at the first: [3][T][n] from [T][11][n]"""
        return np.stack([np.diff(tr[:, c], axis=0, prepend=tr[:1, c]) for c in (CUMH_, CUMICU_, D_)])

    def filter(self, mm, J, seed=SEED, rows=None, status=None, obs=None, want_final=True):
        rows = np.atleast_2d(self.row if rows is None else rows)
        st = np.zeros(rows.shape[0], dtype=np.int32) if status is None else status
        ob = self.obs if obs is None else obs
        return mm.hostabi.particle_from_values(rows, st, self.times, self.N, self.M, self.kappa_ends, ob[0], ob[1], ob[2], J, self.m, seed,
                                               beta_end_times=self.beta_ends, want_final=want_final)

    def log_weights(self, tr, obs=None):
        """lw of one path per observed row in numpy: [Tp]; cells whose observation is not usable count 0"""
        ob = self.obs if obs is None else obs
        sim = np.maximum(self.daily(tr)[:, self.runup:], 0.0) + 1e-10
        use = np.isfinite(ob) & (ob >= 0.0)
        with np.errstate(invalid="ignore"):
            term = np.where(use, np.where(use, ob, 0.0) * np.log(sim) - sim, 0.0)
        return term.sum(axis=(0, 2)), use.any(axis=(0, 2))


@pytest.fixture(scope="module")
def case(mm):
    return Case(mm)


def logsumexp(x):
    m = np.max(x)
    return m + math.log(math.fsum(np.exp(x - m)))


# ---- J = 1
def test_one_particle_is_replicate_zero_of_the_stochastic_call(mm, case):
    rows = np.stack([case.row, case.row])
    got = case.filter(mm, 1, rows=rows)
    ref = case.paths(mm, 1, SEED, rows=rows)
    assert np.array_equal(got["final_state"], ref["final_state"])
    assert not np.array_equal(ref["traj"][0, 0], ref["traj"][1, 0])  # the stream word s = b is in use
    for b in range(2):
        lw, used = case.log_weights(ref["traj"][b, 0])
        assert used.all() and (case.obs > 0).any()
        assert got["loglik"][b] == pytest.approx(lw.sum(), rel=1e-12)
        np.testing.assert_allclose(got["increments"][b], lw, rtol=1e-12)
        assert np.array_equal(got["ess"][b], np.ones(case.Tp))


# ---- the slots before the first resampling
def match_ancestors(final, replicates):
    """the replicate every final particle is a copy of (the replicates are distinct)"""
    anc = []
    for x in final:
        hits = [j for j, r in enumerate(replicates) if np.array_equal(x, r)]
        assert len(hits) == 1, hits
        anc.append(hits[0])
    return np.array(anc)


def check_ancestors(anc, logw):
    """systematic resampling: non-decreasing ancestors, each j taken floor(J W_j) or ceil(J W_j) times.  J W_j comes from numpy's
    weights here: 1e-9 covers their rounding (a dozen ulps of a sum of J <= 257 terms) where J W_j is an integer."""
    J = len(logw)
    assert anc.shape == (J,) and (np.diff(anc) >= 0).all() and anc.min() >= 0 and anc.max() < J
    w = np.exp(logw - np.max(logw))
    share = J * w / w.sum()
    count = np.bincount(anc, minlength=J)
    assert (count >= np.floor(share - 1e-9)).all() and (count <= np.ceil(share + 1e-9)).all(), (count, share)


def test_slots_are_the_stochastic_replicates_until_the_first_observed_row(mm, case):
    J = 9
    obs = np.full_like(case.obs, np.nan)
    obs[:, -1] = case.obs[:, -1]  # the only usable row is the last
    got = case.filter(mm, J, obs=obs)
    ref = case.paths(mm, J, SEED)
    reps = ref["traj"][0]  # [J][T][11][n]
    lw = np.array([case.log_weights(reps[j], obs)[0][-1] for j in range(J)])
    assert got["loglik"][0] == pytest.approx(logsumexp(lw) - math.log(J), rel=1e-12)
    assert np.isnan(got["ess"][0, :-1]).all() and not got["increments"][0, :-1].any()
    w = np.exp(lw - lw.max())
    assert got["ess"][0, -1] == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-12) and 1.0 < got["ess"][0, -1] < J
    anc = match_ancestors(got["final_state"][0], ref["final_state"][0])
    check_ancestors(anc, lw)
    assert np.array_equal(anc, mm.hostabi.particle_resample(lw, SEED, b=0, row=case.T - 1)["ancestors"])


def test_a_problem_without_usable_observations_is_the_stochastic_call(mm, case):
    J = 6
    got = case.filter(mm, J, obs=np.full_like(case.obs, np.nan))
    assert np.array_equal(got["final_state"], case.paths(mm, J, SEED)["final_state"])
    assert got["loglik"][0] == 0.0 and not got["increments"].any() and np.isnan(got["ess"]).all()
    # fewer observation rows than output times >= 0: the rows beyond them have none
    short = case.filter(mm, J, obs=case.obs[:, :3])
    padded = case.obs.copy()
    padded[:, 3:] = np.nan
    full = case.filter(mm, J, obs=padded)
    for key in ("loglik", "increments", "ess", "final_state"):
        assert np.array_equal(short[key], full[key], equal_nan=True), key
    assert np.isfinite(short["ess"][0, :3]).all() and np.isnan(short["ess"][0, 3:]).all()


# ---- the resampling rule
def logw_sets():
    """(name, logw) for every J of RESAMPLE_J: random, one dominant, ties, a spread of 700 in log"""
    rng = np.random.default_rng(20240607)
    out = []
    for J in RESAMPLE_J:
        out.append((f"random-{J}", rng.normal(-300.0, 3.0, J)))
        dominant = rng.normal(-50.0, 1.0, J)
        dominant[J // 2] = 40.0
        out.append((f"dominant-{J}", dominant))
        out.append((f"ties-{J}", np.full(J, -12.5)))
        out.append((f"two-levels-{J}", np.where(np.arange(J) % 3 == 0, -1.0, -1.0 + math.log(2.0))))
        out.append((f"spread-{J}", np.linspace(-700.0, 0.0, J) if J > 1 else np.array([-700.0])))
        out.append((f"spread-down-{J}", np.linspace(0.0, -1400.0, J) if J > 1 else np.array([3.0])))
    return out


def check_resampled_row(res, logw):
    J = len(logw)
    check_ancestors(res["ancestors"], logw)
    assert res["increment"] == pytest.approx(logsumexp(logw) - math.log(J), rel=1e-13, abs=1e-13)
    w = np.exp(logw - np.max(logw))
    assert res["ess"] == pytest.approx(math.fsum(w) ** 2 / math.fsum(w * w), rel=1e-13)
    assert 1.0 - 1e-12 <= res["ess"] <= J + 1e-9


def test_resampling_rule(mm):
    seen = set()
    for k, (name, logw) in enumerate(logw_sets()):
        res = mm.hostabi.particle_resample(logw, SEED + k, b=k % 3, row=k)
        check_resampled_row(res, logw)
        again = mm.hostabi.particle_resample(logw, SEED + k, b=k % 3, row=k)
        assert np.array_equal(res["ancestors"], again["ancestors"]) and res["increment"] == again["increment"]
        seen.add(name.split("-")[0])
        if name.startswith("ties"):  # equal weights: every slot keeps itself
            assert np.array_equal(res["ancestors"], np.arange(len(logw))) and res["ess"] == len(logw)
        if name.startswith("dominant") and len(logw) > 2:
            assert (res["ancestors"] == len(logw) // 2).all()
    assert seen == {"random", "dominant", "ties", "two", "spread"}
    # the uniform depends on each of seed, b and row
    logw = logw_sets()[18][1]  # random-64
    base = mm.hostabi.particle_resample(logw, SEED, b=1, row=4)["ancestors"]
    others = [mm.hostabi.particle_resample(logw, SEED + ds, b=1 + db, row=4 + dr)["ancestors"]
              for ds, db, dr in ((1, 0, 0), (1 << 32, 0, 0), (0, 1, 0), (0, 0, 1))]
    assert len(logw) == 64 and all(not np.array_equal(base, o) for o in others)


# ---- unbiasedness
def test_the_estimate_is_unbiased_across_particle_counts(mm):
    """n = 1, 6 output rows (one of them run-up).  exp(loglik) estimates p(y | theta) without bias for every J, so the means of
    exp(loglik - c) at J = 2 and at J = 64 agree within their standard errors: K = 150 seeds x 4 positions = 600 estimates each,
    difference below 5 combined standard errors.  Deterministic: the seeds are fixed.
    An error that biases both arms alike passes here; tests/test_particle_filter_exact_cpu.py compares with the exact likelihood."""
    case = Case(mm, n=1, T=6, runup=1, m=2)
    rows = np.stack([case.row] * 4)
    K = 150
    ll = {J: np.concatenate([case.filter(mm, J, seed=1000 + k, rows=rows, want_final=False)["loglik"] for k in range(K)]) for J in (2, 64)}
    c = ll[64].mean()
    est = {J: np.exp(v - c) for J, v in ll.items()}
    mean = {J: v.mean() for J, v in est.items()}
    se = {J: v.std(ddof=1) / math.sqrt(v.size) for J, v in est.items()}
    z = (mean[2] - mean[64]) / math.hypot(se[2], se[64])
    print(f"J = 2: {mean[2]:.4f} +- {se[2]:.4f}; J = 64: {mean[64]:.4f} +- {se[64]:.4f}; z = {z:+.2f}; mean loglik {ll[2].mean():.3f} / {ll[64].mean():.3f}")
    assert abs(z) < 5.0
    assert se[64] < se[2] and ll[2].mean() < ll[64].mean()  # more particles: less noise, less of Jensen's gap


# ---- observations that are not usable
def test_nan_and_negative_observations_are_skipped_cell_by_cell(mm, case):
    obs = case.obs.copy()
    obs[0, 1, 0] = np.nan
    obs[1, 1, 2] = -1.0
    obs[2, 4, 1] = np.inf
    obs[:, 5] = np.nan
    obs[0, 5, 1] = -3.0  # row 5: nothing usable
    got = case.filter(mm, 1, obs=obs)
    lw, used = case.log_weights(case.paths(mm, 1, SEED)["traj"][0, 0], obs)
    assert list(used) == [True] * 5 + [False] + [True] * (case.Tp - 6)
    np.testing.assert_allclose(got["increments"][0], lw, rtol=1e-12)
    assert got["increments"][0, 5] == 0.0 and np.isnan(got["ess"][0, 5]) and np.isfinite(np.delete(got["ess"][0], 5)).all()
    assert got["loglik"][0] == pytest.approx(lw.sum(), rel=1e-12)
    full = case.filter(mm, 1)
    assert got["loglik"][0] != full["loglik"][0] and got["increments"][0, 0] == full["increments"][0, 0]


def test_a_row_with_no_usable_observation_leaves_the_particles_alone(mm, case):
    """the same observations with the last two rows blanked: everything up to them is unchanged, the particles then run on
    without being resampled -- each final particle continues the particle of its slot"""
    J = 8
    cut = case.obs.copy()
    cut[:, -2:] = np.nan
    got, full = case.filter(mm, J, obs=cut), case.filter(mm, J)
    assert np.array_equal(got["increments"][0, :-2], full["increments"][0, :-2]) and np.array_equal(got["ess"][0, :-2], full["ess"][0, :-2])
    assert not got["increments"][0, -2:].any() and np.isnan(got["ess"][0, -2:]).all()
    assert got["loglik"][0] == np.cumsum(full["increments"][0])[-3]  # the same sum in the same order
    # a filter over the shorter problem ends where the blank rows begin; D and the cumulative counts only grow from there
    short = Case(mm)
    short.times, short.T, short.Tp, short.obs = case.times[:-2], case.T - 2, case.Tp - 2, case.obs[:, :-2]
    before = short.filter(mm, J)["final_state"][0]
    after = got["final_state"][0]
    assert np.array_equal(short.filter(mm, J)["loglik"], got["loglik"])
    for c in (D_, CUMH_, CUMICU_, R_):
        assert (after[:, c] >= before[:, c]).all()
    assert np.array_equal(after[:, POP].sum(axis=1), before[:, POP].sum(axis=1)) and not np.array_equal(after, before)


# ---- invalid parameter vectors, independence
def test_an_invalid_theta_does_not_disturb_its_neighbours(mm, case):
    rows = np.stack([case.row] * 3)
    ok = case.filter(mm, 5, rows=rows)
    bad = case.filter(mm, 5, rows=rows, status=np.array([0, 1, 0], dtype=np.int32))
    assert bad["loglik"][1] == -DBL_MAX and bad["n_valid"] == 2
    assert np.isnan(bad["final_state"][1]).all() and np.isnan(bad["increments"][1]).all() and np.isnan(bad["ess"][1]).all()
    for key in ("loglik", "increments", "ess", "final_state"):
        assert np.array_equal(bad[key][[0, 2]], ok[key][[0, 2]]), key
    assert ok["loglik"][0] != ok["loglik"][2]  # equal values at another position: another stream


def test_a_position_does_not_depend_on_the_call_around_it(mm, case):
    rows = np.stack([case.row, case.row * 1.0, case.row])
    rows[1, 7] *= 1.1  # another beta in the middle
    three = case.filter(mm, 12, rows=rows)
    two = case.filter(mm, 12, rows=rows[:2], want_final=False)
    assert "final_state" not in two
    for key in ("loglik", "increments", "ess"):
        assert np.array_equal(two[key], three[key][:2]), key
    assert not np.array_equal(case.filter(mm, 12, seed=SEED + 1)["loglik"], three["loglik"][:1])
    assert not np.array_equal(case.filter(mm, 13)["loglik"], three["loglik"][:1])


# ---- arguments
def test_validator_messages_and_particle_limits(mm):
    host = mm.hostabi
    ok = dict(B=3, J=64, steps_per_interval=2, n_times=10, T_pos=8, n_age=4)
    host.particle_validate(**ok)
    limit = {n: host.particle_max_particles(n) for n in range(1, 17)}
    assert limit[4] >= 128 and limit[16] >= 32
    assert limit[1] >= limit[2] >= limit[3] == limit[4] >= limit[5] == limit[8] >= limit[9] == limit[16]  # a function of n rounded up to 2^k
    assert host.particle_max_particles(0) == -1 and host.particle_max_particles(17) == -1
    for change, word in ((dict(B=0), "B must be >= 1"), (dict(J=0), "J must lie in [1, "), (dict(J=limit[4] + 1), "J must lie in [1, %d]" % limit[4]),
                         (dict(steps_per_interval=0), "steps_per_interval must be >= 1"), (dict(T_pos=0), "output time >= 0"),
                         (dict(T_pos=11), "n_times >= T_pos"), (dict(n_age=0), "n_age must lie in [1, 16]"), (dict(n_age=17), "n_age must lie in [1, 16]"),
                         (dict(n_times=2 ** 21, T_pos=5, steps_per_interval=2), "below 2^22"), (dict(n_age=16, J=limit[16] + 1), "J must lie in")):
        with pytest.raises(ValueError) as e:
            host.particle_validate(**{**ok, **change})
        assert word in str(e.value) and str(e.value).startswith("particle_loglik: "), (change, str(e.value))
    host.particle_validate(**{**ok, "J": limit[4]})
    host.particle_validate(**{**ok, "n_age": 16, "J": limit[16]})
    host.particle_validate(**{**ok, "n_times": 2 ** 21 - 1, "T_pos": 5})


def test_twin_refuses_what_the_device_call_refuses(mm, case):
    with pytest.raises(ValueError, match="J must lie in"):
        case.filter(mm, 0)
    with pytest.raises(ValueError, match="J must lie in"):
        case.filter(mm, mm.hostabi.particle_max_particles(3) + 1)
    with pytest.raises(ValueError, match="steps_per_interval"):
        mm.hostabi.particle_from_values(case.row, [0], case.times, case.N, case.M, case.kappa_ends, case.obs[0], case.obs[1], case.obs[2], 4, 0, SEED,
                                        beta_end_times=case.beta_ends)


def test_header_and_exports(mm):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sepaihrd_hip.h")).read()
    for sym in ("sepaihrd_particle_loglik", "sepaihrd_particle_validate", "sepaihrd_particle_max_particles", "sepaihrd_particle_timing",
                "sepaihrd_particle_resample_device"):
        assert sym in mm.hipabi.EXPORTED_SYMBOLS and hasattr(mm.hipabi.load_library(), sym) and "int " + sym + "(" in text
    assert "#define SEPAIHRD_ABI_VERSION 3" in text
