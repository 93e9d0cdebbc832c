"""The 16-lane integrator's RK body against the 4-lane kernel, bit for bit, after its instruction stream was rearranged
(csrc/sepaihrd_lane_split.inc: the contact sum as one fixed sequence, the leading tableau factors from the row vector).

The shipped 4-age problem on a 12-row output grid whose rows are 4-5 days apart and skip the beta / kappa breakpoint at
t = 13: the step size grows past its first value, the breakpoint makes steps fail, and the step from 12 to 16 has stages on
both sides of it (the second copy of the attempt code in the tolerance build).  1, 5 and 67 chains: a partial wave, a partial
workgroup, and more than one workgroup with a partial last one (a wave holds 4 chains, a workgroup 16)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = np.array([-20.0, -15.0, -10.0, -5.0, 0.0, 4.0, 8.0, 12.0, 16.0, 20.0, 24.0, 28.0])
FIELDS = ("loglik", "status", "n_accept", "n_reject")


def _problem(mm, shipped, solver, arith, constraint_mode):
    assert np.sum((shipped.kappa_end_times > GRID[0]) & (shipped.kappa_end_times < GRID[-1])) == 1
    assert not np.any(np.isin(shipped.kappa_end_times, GRID))
    nobs = int(np.sum(GRID >= 0.0))
    return shipped.with_(times=GRID, obs_H=shipped.obs_H[:nobs], obs_ICU=shipped.obs_ICU[:nobs], obs_D=shipped.obs_D[:nobs],
                         solver=solver, arith=arith, constraint_mode=constraint_mode)


def _theta(mm, pb, B):
    """jittered draws around the calibrated point; every fifth chain drawn across (and a little beyond) the bounds, so that
    the constraint rule acts"""
    from mmid_amd import draws
    theta = draws.jitter_draws(pb, 11, B)
    lo, hi, has = pb.bounds_arrays()
    rs = np.random.RandomState(3)
    wide = lo + (hi - lo) * rs.uniform(-0.1, 1.1, theta.shape)
    rows = np.arange(B) % 5 == 4
    theta[rows] = np.where(has.astype(bool), wide, theta)[rows]
    return theta


def _run(mm, pb, theta, form):
    hip = mm.HipObjective(pb)
    try:
        hip.set_integrator_form(form)
        return hip.eval_batch(theta)
    finally:
        hip.close()


@pytest.mark.parametrize("chains", [1, 5, 67])
@pytest.mark.parametrize("constraint", ["reflect", "clamp"])
@pytest.mark.parametrize("arith", ["fma", "strict"])
@pytest.mark.parametrize("solver", [0, 1])
def test_quad_body_gives_the_four_lane_kernels_bits(mm, oracle_py, shipped, solver, arith, constraint, chains):
    pb = _problem(mm, shipped, solver, mm.ARITH_FMA if arith == "fma" else mm.ARITH_STRICT,
                  mm.CONSTRAINT_REFLECT if constraint == "reflect" else mm.CONSTRAINT_CLAMP)
    theta = _theta(mm, pb, chains)
    quad = _run(mm, pb, theta, mm.hipabi.FORM_QUAD)
    lane = _run(mm, pb, theta, mm.hipabi.FORM_LANE_PER_AGE)
    for k in FIELDS:
        a, b = quad[k], lane[k]
        same = np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b)
        assert same, (k, a, b)
    ok = quad["status"] == 0
    assert ok.any()
    if chains == 67:  # the grid does what it was chosen for: steps longer than the first, and failed steps
        assert np.all(quad["n_accept"][ok] >= len(GRID) - 1)
        assert quad["n_reject"][ok].max() > 0
    if arith == "strict":
        ref = oracle_py.Oracle(pb).eval_batch(theta)
        assert np.array_equal(quad["status"], ref["status"])
        assert np.array_equal(quad["n_accept"], ref["n_accept"]), (quad["n_accept"], ref["n_accept"])
        assert np.array_equal(quad["n_reject"], ref["n_reject"]), (quad["n_reject"], ref["n_reject"])
