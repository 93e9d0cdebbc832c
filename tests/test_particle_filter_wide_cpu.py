"""The wide form of the particle filter on the host twin (hostParticleLoglikWide behind sepaihrd_particle_wide_validate): the bits
of the narrow twin wherever that takes J, runs above its limit, the argument rules with their messages, the exact likelihood of a
tiny epidemic at J = 1000, and the fall of the estimate's spread with J.  No device."""
import math
import os

import numpy as np
import pytest

from test_particle_filter_cpu import SEED, Case, check_ancestors
from test_particle_filter_exact_cpu import BETA_ENDS, CASES, KAPPA_ENDS, check_prefix_likelihoods

KEYS = ("loglik", "increments", "ess", "final_state")
WIDE_MAX = 65536


@pytest.fixture(scope="module")
def case(mm):
    return Case(mm)


def wide_filter(mm, case, J, seed=SEED, rows=None, status=None, obs=None, want_final=True):
    rows = np.atleast_2d(case.row if rows is None else rows)
    st = np.zeros(rows.shape[0], dtype=np.int32) if status is None else status
    ob = case.obs if obs is None else obs
    return mm.hostabi.particle_wide_from_values(rows, st, case.times, case.N, case.M, case.kappa_ends, ob[0], ob[1], ob[2], J, case.m, seed,
                                                beta_end_times=case.beta_ends, want_final=want_final)


def test_wide_twin_equals_the_narrow_twin_within_its_limit(mm, case):
    rows = np.stack([case.row, case.row, case.row])
    status = np.array([0, 1, 0], dtype=np.int32)  # an invalid vector between two valid ones
    obs = case.obs.copy()
    obs[0, 1, 0] = np.nan
    obs[:, 4] = np.nan  # a row without a usable cell
    for J in (1, 5, 64, mm.hostabi.particle_max_particles(3)):
        narrow = case.filter(mm, J, rows=rows, status=status, obs=obs)
        wide = wide_filter(mm, case, J, rows=rows, status=status, obs=obs)
        for key in KEYS:
            assert np.array_equal(narrow[key], wide[key], equal_nan=True), (J, key)
        assert wide["n_valid"] == 2 and np.isfinite(wide["loglik"][[0, 2]]).all()


@pytest.mark.parametrize("J", ["limit + 1", 1000])
def test_wide_twin_runs_above_the_limit(mm, case, J):
    J = mm.hostabi.particle_max_particles(3) + 1 if J == "limit + 1" else J
    with pytest.raises(ValueError, match="J must lie in"):
        case.filter(mm, J)
    got = wide_filter(mm, case, J)
    assert np.isfinite(got["loglik"]).all() and np.isfinite(got["increments"]).all() and np.isfinite(got["final_state"]).all()
    assert (got["ess"] >= 1.0).all() and (got["ess"] <= J).all() and (got["ess"] < J).any()
    assert got["loglik"][0] == np.cumsum(got["increments"][0])[-1]
    # the only usable row the last: the final particles are copies of the plain replicates, chosen by systematic resampling
    obs = np.full_like(case.obs, np.nan)
    obs[:, -1] = case.obs[:, -1]
    last = wide_filter(mm, case, J, obs=obs)
    ref = case.paths(mm, J, SEED)
    lw = np.array([case.log_weights(ref["traj"][0, j], obs)[0][-1] for j in range(J)])
    reps = np.unique(ref["final_state"][0].reshape(J, -1), axis=0)
    assert len(reps) == J  # the replicates are distinct
    anc = mm.hostabi.particle_resample(lw, SEED, b=0, row=case.T - 1)["ancestors"]
    check_ancestors(anc, lw)
    assert np.array_equal(last["final_state"][0], ref["final_state"][0][anc])


def test_wide_validator_messages_and_limits(mm):
    host = mm.hostabi
    assert host.particle_wide_max_particles() == WIDE_MAX
    ok = dict(B=3, J=5000, steps_per_interval=2, theta_chunk=0, n_times=10, T_pos=8, n_age=4)
    host.particle_wide_validate(**ok)
    for change, word in ((dict(B=0), "B must be >= 1"), (dict(J=0), "J must lie in [1, 65536]"), (dict(J=WIDE_MAX + 1), "J must lie in [1, 65536]"),
                         (dict(theta_chunk=-1), "theta_chunk must be >= 0"), (dict(steps_per_interval=0), "steps_per_interval must be >= 1"),
                         (dict(T_pos=0), "output time >= 0"), (dict(T_pos=11), "n_times >= T_pos"), (dict(n_age=0), "n_age must lie in [1, 16]"),
                         (dict(n_age=17), "n_age must lie in [1, 16]"), (dict(n_times=2 ** 21, T_pos=5, steps_per_interval=2), "below 2^22"),
                         (dict(B=2 ** 15, J=WIDE_MAX), "B x J must stay below 2^31"), (dict(B=2 ** 19, J=4096), "B x J must stay below 2^31")):
        with pytest.raises(ValueError) as e:
            host.particle_wide_validate(**{**ok, **change})
        assert word in str(e.value) and str(e.value).startswith("particle_loglik_wide: "), (change, str(e.value))
    host.particle_wide_validate(**{**ok, "J": WIDE_MAX})
    host.particle_wide_validate(**{**ok, "J": 1})
    host.particle_wide_validate(**{**ok, "n_age": 16, "J": WIDE_MAX})
    host.particle_wide_validate(**{**ok, "theta_chunk": 7})
    host.particle_wide_validate(**{**ok, "B": 2 ** 15 - 1, "J": WIDE_MAX})
    host.particle_wide_validate(**{**ok, "n_times": 2 ** 21 - 1, "T_pos": 5})
    # the narrow rules are where they were
    limit = host.particle_max_particles(4)
    with pytest.raises(ValueError, match=r"particle_loglik: J must lie in \[1, %d\]" % limit):
        host.particle_validate(3, limit + 1, 2, 10, 8, 4)


def test_wide_twin_refuses_what_the_device_call_refuses(mm, case):
    with pytest.raises(ValueError, match=r"particle_loglik_wide: J must lie in \[1, 65536\]"):
        wide_filter(mm, case, 0)
    with pytest.raises(ValueError, match=r"particle_loglik_wide: J must lie in \[1, 65536\]"):
        wide_filter(mm, case, WIDE_MAX + 1)
    with pytest.raises(ValueError, match="particle_loglik_wide: steps_per_interval"):
        mm.hostabi.particle_wide_from_values(case.row, [0], case.times, case.N, case.M, case.kappa_ends, case.obs[0], case.obs[1], case.obs[2], 4, 0,
                                             SEED, beta_end_times=case.beta_ends)


def test_header_and_exports_of_the_wide_form(mm):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sepaihrd_hip.h")).read()
    for sym in ("sepaihrd_particle_loglik_wide", "sepaihrd_particle_wide_validate", "sepaihrd_particle_wide_max_particles",
                "sepaihrd_particle_wide_timing", "sepaihrd_particle_wide_resample_device"):
        assert sym in mm.hipabi.EXPORTED_SYMBOLS and hasattr(mm.hipabi.load_library(), sym) and "int " + sym + "(" in text
    assert "#define SEPAIHRD_ABI_VERSION 3" in text
    assert hasattr(mm.hostabi.load_library(), "host_particle_wide_from_values")


def test_prefix_likelihoods_at_a_thousand_particles_meet_the_exact_ones(mm):
    """The n = 1 case of tests/test_particle_filter_exact_cpu.py (five people) at J = 1000, E = 2048 independent estimates: the mean
    of exp(sum of the increments up to k) / Z[k] within 5 standard errors of 1 at every row, every standard error at most 0.05
    (check_prefix_likelihoods).  Measured: the largest standard error is 0.0028."""
    tiny = CASES["n1"]
    exact = tiny.exact(tiny.row(mm))
    B, K, J = 1024, 2, 1000
    rows = np.stack([tiny.row(mm)] * B)
    inc = np.concatenate([mm.hostabi.particle_wide_from_values(rows, np.zeros(B, dtype=np.int32), tiny.times, tiny.N, tiny.M, KAPPA_ENDS, tiny.obs[0],
                                                               tiny.obs[1], tiny.obs[2], J, tiny.m, 0x57A7_15_71C5 + k, beta_end_times=BETA_ENDS,
                                                               want_final=False)["increments"] for k in range(K)])
    assert inc.shape == (2048, tiny.Tp) and J > mm.hostabi.particle_max_particles(1)
    check_prefix_likelihoods("n1 at J = 1000", inc, exact.Z)


def test_the_spread_of_the_estimate_falls_with_the_particles(mm, case):
    """loglik over 64 seeds at J = 64 and at J = 2048: 32 times the particles, so about 1 / sqrt(32) = 0.18 of the standard
    deviation.  Measured: 1.79 and 0.30, ratio 0.17."""
    sd = {}
    for J in (64, 2048):
        ll = np.array([wide_filter(mm, case, J, seed=9000 + k, want_final=False)["loglik"][0] for k in range(64)])
        sd[J] = ll.std(ddof=1)
    print(f"sd of loglik over 64 seeds: J = 64 {sd[64]:.4f}, J = 2048 {sd[2048]:.4f}, ratio {sd[2048] / sd[64]:.3f} (1 / sqrt(32) = {1 / math.sqrt(32):.3f})")
    assert sd[2048] < sd[64]
