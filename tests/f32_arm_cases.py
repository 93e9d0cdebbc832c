"""Problems and theta batches of the fp32-arm tests (csrc/sepaihrd_kernels_f32.hip), shared by tests/test_f32_arm_inputs_cpu.py
(oracle only: can these inputs see what they are meant to see?) and tests/test_gpu_f32_arm.py (kernel against oracle).
A plain module: every problem is built in code from shipped_problem.json and reference_test_fixture.json.

Why the problems look as they do.  widen_age_classes replicates age bands, M'(i,j) = M(i/f, j/f)/f, so the columns inside a
replicated block are identical and a kernel that reads lane sigma(J) for lane J computes the same trajectory: the 8- and
16-lane contact sums cannot be tested on such a matrix.  lane_problem() makes the columns distinct and lane_batch() gives every
chain ONE infectious age class, so that a wrong source lane replaces that class's column of M by another one.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The bars of the fp32 arm (tests/test_gpu_parity.py::test_fp32_arm_*): states relative (floor of one person), loglik relative.
STATE_BAR = 5e-4
LOGLIK_BAR = 2e-3

LANE_COUNTS = (3, 4, 5, 7, 8, 9, 15, 16)   # LPC 4: 3, 4; LPC 8: 5, 7, 8; LPC 16: 9, 15, 16
LPC_FULL = {4: 4, 8: 8, 16: 16}            # lanes per chain -> the unpadded age count that uses them


def lanes_per_chain(n):
    return 4 if n <= 4 else (8 if n <= 8 else 16)


def rel_state_err(a, b):
    """tests/test_gpu_parity.py rel_state_err: relative error per state entry with a floor of one person"""
    return np.abs(a - b) / np.maximum(np.abs(b), 1.0)


def load(mm, name):
    return mm.SEPAIHRDProblem.load(os.path.join(GOLDEN, name))


def cut_grid(pb, times):
    """The problem on another output grid, with as many observation rows as the objective wants (T - runup offset)."""
    times = np.asarray(times, dtype=np.float64)
    q = pb.with_(times=times)
    rows = q.n_times - q.runup_offset
    return q.with_(obs_H=pb.obs_H[:rows], obs_ICU=pb.obs_ICU[:rows], obs_D=pb.obs_D[:rows])


# ------------------------------------------------------------------------------------------------------------ A: source lanes
def lane_problem(mm, n, rows=40):
    """shipped problem widened to the lane width, M made column-distinct, restricted to n classes, first `rows` outputs,
    every h_infec_j free in (0.01, 1.2)."""
    shipped = load(mm, "shipped_problem.json")
    f = lanes_per_chain(n) // 4
    pb = mm.widen_age_classes(shipped, f) if f > 1 else shipped
    i, j = np.indices(pb.M.shape)
    pb = pb.with_(M=pb.M * (1.0 + 0.5 * np.sin(1.0 + 3.0 * i + 7.0 * j)))
    if n < pb.n:
        pb = mm.restrict_age_classes(pb, list(range(n)))
    pb = cut_grid(pb, pb.times[:rows])
    bounds = dict(pb.bounds)
    for c in range(n):
        bounds[f"h_infec_{c}"] = (0.01, 1.2)
    return pb.with_(bounds=bounds, arith=mm.ARITH_FMA)


def lane_batch(mm, pb):
    """n chains, chain c with h_infec_c at its upper bound and every other h_infec_j at its lower bound, then 5 or 6 jittered
    chains so that the last wave is ragged in the problem's lane layout."""
    from mmid_amd import draws
    n = pb.n
    theta = np.tile(pb.base_theta, (n, 1))
    cols = [pb.param_names.index(f"h_infec_{c}") for c in range(n)]
    theta[:, cols] = 0.01
    theta[np.arange(n), cols] = 1.2
    cpw = 64 // lanes_per_chain(n)
    extra = 5 if (n + 5) % cpw else 6
    return np.vstack([theta, draws.jitter_draws(pb, 11, extra)])


def swap_columns(pb, a, b):
    M = pb.M.copy()
    M[:, [a, b]] = M[:, [b, a]]
    return pb.with_(M=M)


# ---------------------------------------------------------------------------------------- B: every instantiation, both builds
def big_problem(mm, lpc):
    """the problem of A with unpadded lanes on 12 outputs three days apart (t = -20 .. 13: the run-up, five observed rows)"""
    pb = lane_problem(mm, LPC_FULL[lpc])
    return cut_grid(pb, load(mm, "shipped_problem.json").times[:36:3])


def big_batch(mm, pb):
    """(tile of 64 distinct jittered theta, B): B = 1024 chains-per-wave + 1 chains, i.e. 1025 workgroups, the last one with
    a single chain -- one more than the one-wave-per-SIMD build is launched for."""
    from mmid_amd import draws
    tile = draws.jitter_draws(pb, 21, 64)
    return tile, 1024 * (64 // lanes_per_chain(pb.n)) + 1


# ------------------------------------------------------------------------------------------------- C: independence of company
def company_problem(mm, lpc, constraint_mode):
    """the problem of A (40 outputs, the beta and kappa breakpoint at t = 13 inside) with kappa_3 allowed below zero, so that
    a wave-mate can fail at once"""
    pb = lane_problem(mm, LPC_FULL[lpc])
    bounds = dict(pb.bounds)
    bounds["kappa_3"] = (-1.0, 1.2)
    return pb.with_(bounds=bounds, constraint_mode=constraint_mode)


def company_batch(mm, pb):
    """(target theta, batch, positions of the target in the batch).  The target sits first in a full wave, in the middle of
    a full wave and last in a ragged wave; every other chain is one of the mates below, in turn."""
    from mmid_amd import draws
    lo, hi, _ = pb.bounds_arrays()
    names = pb.param_names
    target = draws.jitter_draws(pb, 31, 1)[0]
    fails = pb.base_theta.copy()
    fails[names.index("kappa_3")] = -0.5                        # negative calibrated kappa: status 1 before the first step
    jump = pb.base_theta.copy()                                 # another beta kappa jump at t = 13 and another growth rate
    jump[names.index("kappa_2")] = 1.2                          # before it: its steps meet the breakpoint on other attempts
    jump[names.index("beta_1")] = 0.9
    far = pb.base_theta.copy()                                  # the far end of the bounds of everything that drives growth
    for k, nm in enumerate(names):
        if nm.startswith(("beta_", "kappa_", "h_infec_", "a_")) or nm in ("theta", "sigma", "gamma_p"):
            far[k] = hi[k]
    rs = np.random.RandomState(41)
    outside = lo + (hi - lo) * rs.uniform(-0.3, 1.3, (2, pb.n_params))   # beyond the bounds: the constraint rule acts
    outside[:, names.index("kappa_3")] = np.abs(outside[:, names.index("kappa_3")]) + 0.2  # ... but these two still run
    mates = [fails, jump, far, outside[0], outside[1], draws.jitter_draws(pb, 32, 1)[0]]
    cpw = 64 // lanes_per_chain(pb.n)
    B = 2 * cpw + max(2, cpw // 2)
    positions = [0, cpw + cpw // 2, B - 1]
    batch = np.empty((B, pb.n_params))
    m = 0
    for b in range(B):
        if b in positions:
            batch[b] = target
        else:
            batch[b] = mates[m % len(mates)]
            m += 1
    return target, batch, positions


# -------------------------------------------------------------------------------------------------------------- D: schedule
def schedule_problem(mm, n=4):
    """reference fixture (30 daily outputs from t = 0, dt hint 1) with the largest schedule the C ABI takes: 32 beta periods and
    32 kappa periods with no end time in common, i.e. 64 merged end times and 65 segments of beta kappa.  Two breakpoints lie
    inside the first step (kappa at 0.2, beta at 0.6), four on grid times (kappa at 2, 5, 9, 14), the others between grid
    times (0.86 apart in each list, the two lists interleaved); one factor jumps by 2 x or more at every one."""
    pb = load(mm, "reference_test_fixture.json")
    k_ends = sorted([0.2, 2.0, 5.0, 9.0, 14.0] + [round(1.43 + 0.86 * k, 10) for k in range(26)]) + [305.0]
    b_ends = sorted([0.6] + [round(1.86 + 0.86 * k, 10) for k in range(30)]) + [306.0]
    k_pat, b_pat = (1.0, 0.4, 1.1, 0.3, 0.9, 0.45, 1.2, 0.5), (0.12, 0.05, 0.14, 0.06, 0.13, 0.055)
    k_val = np.array([k_pat[k % len(k_pat)] for k in range(len(k_ends))])
    b_val = np.array([b_pat[k % len(b_pat)] for k in range(len(b_ends))])
    names = ["beta_1" if nm == "beta" else nm for nm in pb.param_names]
    rename = lambda d: {("beta_1" if k == "beta" else k): v for k, v in d.items()}
    base = pb.base_theta.copy()
    base[names.index("beta_1")] = b_val[0]
    for nm in ("kappa_1", "kappa_2", "kappa_3"):
        base[names.index(nm)] = k_val[int(nm[6:])]
    pb = pb.with_(kappa_end_times=np.array(k_ends), kappa_values=k_val, npi_names=[f"kappa_{k + 1}" for k in range(len(k_ends) - 1)],
                  beta_end_times=np.array(b_ends), beta_values=b_val, param_names=names, sigmas=rename(pb.sigmas),
                  bounds=rename(pb.bounds), base_theta=base, arith=mm.ARITH_FMA)
    return mm.widen_age_classes(pb, n // 4) if n > 4 else pb


def merged_end_times(pb):
    return np.unique(np.concatenate([pb.beta_end_times, pb.kappa_end_times]))


def schedule_batch(pb):
    rs = np.random.RandomState(51)
    theta = pb.base_theta[None, :] * (1.0 + 0.1 * rs.uniform(-1, 1, (7, pb.n_params)))
    theta[0] = pb.base_theta
    return theta


def shift_breakpoints(pb):
    """every breakpoint moved to the next one of the merged schedule: each segment's value holds over the next segment as well
    -- what a schedule cache that is one refresh late computes"""
    merged = merged_end_times(pb)
    nxt = np.append(merged[1:], merged[-1] + 1.0)
    move = lambda ends: nxt[np.searchsorted(merged, ends)]
    return pb.with_(kappa_end_times=move(pb.kappa_end_times), beta_end_times=move(pb.beta_end_times))


def no_schedule_problem(mm):
    """tests/test_gpu_parity.py::test_minimal_problem_one_parameter_no_schedule on all four age classes (the fp32 arm is built
    for 3 to 16): one calibrated parameter, one kappa period, no breakpoint inside the run"""
    pb = load(mm, "reference_test_fixture.json")
    return pb.with_(param_names=["beta"], sigmas={"beta": 0.01}, bounds={"beta": (0.01, 1.0)}, base_theta=np.array([0.06]),
                    kappa_end_times=np.array([1000.0]), kappa_values=np.array([0.8]), npi_names=[], arith=mm.ARITH_FMA)


NO_SCHEDULE_THETA = np.linspace(0.02, 0.4, 23)[:, None]


# ----------------------------------------------------------------------------------------------------------------- E: edges
def sentinel_cases(mm):
    """name -> (problem, theta, expected status per chain)"""
    shipped = load(mm, "shipped_problem.json")
    shipped = cut_grid(shipped, shipped.times[:60]).with_(arith=mm.ARITH_FMA)
    out = {}
    b = dict(shipped.bounds)
    b["kappa_3"] = (-1.0, 1.2)
    pb = shipped.with_(bounds=b)
    theta = np.tile(pb.base_theta, (5, 1))
    theta[[1, 3], pb.param_names.index("kappa_3")] = (-0.5, -1e-3)
    out["negative_kappa"] = (pb, theta, [0, 1, 0, 1, 0])
    b = dict(shipped.bounds)
    b["seed_exposed"] = (5.0, 1e9)
    pb = shipped.with_(bounds=b)
    theta = np.tile(pb.base_theta, (5, 1))
    theta[[1, 3], pb.param_names.index("seed_exposed")] = (9e8, 2e8)
    out["initial_sum_above_N"] = (pb, theta, [0, 1, 0, 1, 0])
    pb = shipped.with_(obs_H=shipped.obs_H[:-1], obs_ICU=shipped.obs_ICU[:-1], obs_D=shipped.obs_D[:-1])
    out["observation_rows_do_not_match"] = (pb, np.tile(pb.base_theta, (3, 1)), [1, 1, 1])
    return out


def budget_problem(mm):
    return load(mm, "reference_test_fixture.json").with_(arith=mm.ARITH_FMA)


def budget_batch(pb):
    rs = np.random.RandomState(61)
    lo, hi, _ = pb.bounds_arrays()
    return lo + (hi - lo) * rs.uniform(0.2, 0.8, (9, pb.n_params))


BUDGET_SHORT, BUDGET_AMPLE = 50, 600   # attempts: at most half the smallest / at least twice the largest count of the oracle


def observation_problem(mm):
    """NaN, negative and +inf entries in the hospital and ICU streams, a death stream that is all NaN"""
    pb = load(mm, "reference_test_fixture.json").with_(arith=mm.ARITH_FMA)
    oH, oI = pb.obs_H.copy(), pb.obs_ICU.copy()
    oH[3, 1] = np.nan
    oH[7, 2] = -1.0
    oH[0, 0] = np.inf
    oI[29, 3] = np.inf
    oI[12, 0] = np.nan
    oI[13, :] = -3.0
    return pb.with_(obs_H=oH, obs_ICU=oI, obs_D=np.full_like(pb.obs_D, np.nan))


def negative_increment_case(mm):
    """Initial I and H below zero (their multipliers calibrated with a negative lower bound; the reference checks no sign): the
    flows into CumH, CumICU and D run backwards for a while and the daily increments the likelihood reads are negative until
    the epidemic has refilled the compartments -- the observer's cwiseMax(0).  Chain 0 is the fixture as it is."""
    pb = load(mm, "reference_test_fixture.json")
    extra = ["I0_multiplier", "H0_multiplier"]
    bounds, sigmas = dict(pb.bounds), dict(pb.sigmas)
    for nm in extra:
        bounds[nm], sigmas[nm] = (-2.0, 3.0), 0.1
    pb = pb.with_(param_names=pb.param_names + extra, bounds=bounds, sigmas=sigmas, base_theta=np.append(pb.base_theta, [1.0, 1.0]),
                  arith=mm.ARITH_FMA)
    theta = np.tile(pb.base_theta, (4, 1))
    theta[1, -2] = -1.0
    theta[2, -1] = -1.0
    theta[3, -2:] = -1.5
    return pb, theta


def fixture_batch(pb, B, seed, lo_u=0.0, hi_u=1.0):
    rs = np.random.RandomState(seed)
    lo, hi, _ = pb.bounds_arrays()
    return lo + (hi - lo) * rs.uniform(lo_u, hi_u, (B, pb.n_params))


def short_grid_problem(mm, T, solver):
    pb = load(mm, "reference_test_fixture.json")
    return pb.with_(times=np.array([0.0, 0.37, 1.0])[:T], solver=solver, arith=mm.ARITH_FMA, obs_H=pb.obs_H[:T],
                    obs_ICU=pb.obs_ICU[:T], obs_D=pb.obs_D[:T])


def init_mode_problem(mm):
    """the shipped problem's first 60 outputs: the objective seeds the epidemic from theta (mode 0); its stored initial state
    as given (mode 1) and scaled by the multipliers (mode 2) are two other runs"""
    shipped = load(mm, "shipped_problem.json")
    return cut_grid(shipped, shipped.times[:60]).with_(arith=mm.ARITH_FMA)


def extreme_beta_case(mm, scale):
    pb = load(mm, "reference_test_fixture.json").with_(arith=mm.ARITH_FMA, bounds={})
    th = pb.base_theta.copy()
    th[pb.param_names.index("beta")] *= scale
    return pb, th[None, :]
