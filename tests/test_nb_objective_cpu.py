"""The negative-binomial observation model of the deterministic objective on the host: lgamma_pos against
libm, the twin's cell against the negative-binomial log-pmf written out in Python, the Poisson limit, the order of the sums and
the special cases, the validation with its messages, and the twin over the CPU oracle's trajectories.  No device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from nb_objective_cases import (INF, increments, lgamma_grid, nb_logpmf, nb_logpmf_sound, observation_grid, python_reference,
                                with_dispersion)

NAN = float("nan")
GRID_K = (0.01, 0.5, 3.0, 50.0, 1e6)   # tests/test_particle_nb_cpu.py's grid of k; its obs are 0 .. 20
NEW_SYMBOLS = ("sepaihrd_set_dispersion", "sepaihrd_get_dispersion", "sepaihrd_dispersion_validate", "sepaihrd_nb_objective_host",
               "sepaihrd_lgamma_device")


def twin_cells(mm, obs_values, sims, k, lib="host"):
    """cell [len(obs_values)][len(sims)] of the H series under k: one chain per sim, one call per observation"""
    sims = np.asarray(sims, dtype=np.float64)
    out = np.empty((len(obs_values), sims.size))
    inc = np.zeros((sims.size, 1, 3, 1))
    inc[:, 0, 0, 0] = sims - 1e-10   # the twin adds the floor back (exact for the values used here or within an ulp: see callers)
    kk = np.tile([k, INF, INF], (sims.size, 1))
    none = np.full((1, 1), NAN)
    for i, o in enumerate(obs_values):
        out[i] = mm.hostabi.nb_objective(inc, np.full((1, 1), float(o)), none, none, kk, lib=lib)["ll_parts"][:, 0]
    return out


# ---- 1. declarations
def test_header_exports_and_bindings(mm):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sepaihrd_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in mm.hipabi.EXPORTED_SYMBOLS and hasattr(mm.hipabi.load_library(), sym) and "int " + sym + "(" in text, sym
    assert "double sepaihrd_lgamma_host(double x);" in text and hasattr(mm.hipabi.load_library(), "sepaihrd_lgamma_host")
    assert "#define SEPAIHRD_ABI_VERSION 3" in text and mm.hipabi.load_library().sepaihrd_abi_version() == 3
    assert "SEPAIHRD_F_DISPERSION = 28" in text and mm.hipabi.F_DISPERSION == 28 and mm.problem.F_DISPERSION == 28
    for sym in ("host_lgamma_pos", "host_nb_objective", "host_objective_set_dispersion"):
        assert hasattr(mm.hostabi.load_library(), sym), sym
    for name in ("lgamma_pos", "nb_objective"):
        assert callable(getattr(mm.hostabi, name))
    for name in ("set_dispersion", "get_dispersion", "lgamma_device"):
        assert callable(getattr(mm.HipObjective, name))
    assert callable(mm.HostObjective.set_dispersion)
    for i, nm in enumerate(("dispersion_H", "dispersion_ICU", "dispersion_D")):
        assert mm.resolve_param_name(nm, [], 4, 0) == (28, i)


def test_config_reader_and_parameter_views_accept_the_three_names(mm, ref_fixture, tmp_path):
    p = tmp_path / "initial_guess.txt"
    p.write_text("theta 0.3\ndispersion_ICU 7.5\ndispersion_H 2\n")
    par = mm.config_io.read_sepaihrd_parameters(str(p), 4)
    assert par["dispersion"] == [2.0, 7.5, INF] and par["theta"] == 0.3
    p.write_text("theta 0.3\n")
    assert "dispersion" not in mm.config_io.read_sepaihrd_parameters(str(p), 4)
    pb = with_dispersion(ref_fixture, ("dispersion_D", "dispersion_H"), fixed=(INF, 4.0, 9.0))
    codes, idxs = pb.field_map()
    assert codes[-2:].tolist() == [28, 28] and idxs[-2:].tolist() == [2, 0]
    cur = pb.current_parameters()
    assert cur[-2] == 9.0 and cur[-1] == pb.bounds["dispersion_H"][1]   # the fixed value; the Poisson end of the bounds


# ---- 2. lgamma_pos
def test_lgamma_pos_against_libm(mm):
    """lgamma_pos (csrc/sepaihrd_lgamma.inc) against math.lgamma over 10^U(-3, 6.1) (4e5 arguments) and k + obs for
    k in {1e-3, 0.01, 0.5, 1, 3, 50, 1e6}, obs in 0 .. 3000: at most 1e-12 relative to max(1, |ref|).  The series truncates below
    1.2e-16 at x >= 16; what remains is the cancellation of the shifted branch, a few ulp of ~30.  Measured worst case: 9.8e-15
    (at x = 2.21); the library's two compiles (g++ for libsepaihrd_host.so, hipcc's host side for libsepaihrd_hip.so) agree bit
    for bit."""
    x = lgamma_grid()
    got = mm.hostabi.lgamma_pos(x)
    ref = np.array([math.lgamma(v) for v in x])
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    i = int(np.argmax(err))
    print(f"lgamma_pos: largest error {err[i]:.3g} relative to max(1, |ref|) at x = {x[i]:.6g} over {x.size} arguments")
    assert err[i] <= 1e-12
    hip = mm.hipabi.load_library().sepaihrd_lgamma_host
    sub = x[::97]
    assert np.array_equal(np.array([hip(float(v)) for v in sub]), got[::97])


# ---- 3. the cell against the log-pmf
@pytest.mark.parametrize("k", GRID_K)
def test_cell_is_the_negative_binomial_log_pmf(mm, k):
    """cell - lgamma(obs + 1) against the log-pmf with mean sim and size k, obs in 0 .. 20 and 21 real-valued sim in [1e-10, 27.4],
    relative to max(1, |log-pmf|): at most 1e-9 (tests/test_particle_nb_cpu.py's bound and grid of k).  The pmf is written out in
    Python twice: nb_logpmf as that file writes it, and nb_logpmf_sound, the same quantity without the cancellation of
    lgamma(obs + k) - lgamma(k) and of k log(k / (k + sim)).  At k = 1e6 nb_logpmf itself is 1.17e-9 off a 40-digit evaluation of
    the pmf -- more than the bound -- so the bound is asserted against the sound form for every k and against nb_logpmf for
    k < 1e6.  Measured against the sound form: 1.0e-10 at k = 1e6 (the rounding of 1 + sim / k, times k), below 4e-14 elsewhere;
    against nb_logpmf: 1.24e-9 at k = 1e6 (with both lgammas rounded to doubles the twin too was 1.0e-9 off the 40-digit value;
    hence the two-part lgamma of csrc/sepaihrd_lgamma.inc), below 4e-14 elsewhere."""
    obs = np.arange(21.0)
    sims = np.arange(21) * 1.37 + 1e-10
    cells = twin_cells(mm, obs, sims, k)
    worst = literal = 0.0
    for i, o in enumerate(obs):
        for j, sim in enumerate(sims):
            eff = max(0.0, sim - 1e-10) + 1e-10   # the sim the twin formed
            got = cells[i, j] - math.lgamma(o + 1.0)
            ref, lit = nb_logpmf_sound(o, eff, k), nb_logpmf(o, eff, k)
            worst = max(worst, abs(got - ref) / max(1.0, abs(ref)))
            literal = max(literal, abs(got - lit) / max(1.0, abs(lit)))
    print(f"k = {k:g}: largest relative error {worst:.3g} (against nb_logpmf as the particle test writes it: {literal:.3g})")
    assert worst <= 1e-9
    assert k >= 1e6 or literal <= 1e-9


# ---- 4. the Poisson limit
def test_cell_tends_to_the_poisson_cell(mm):
    """at k = 1e6: within 2.1e-4 of the Poisson cell over obs, sim in {0 .. 20}^2 (+ the floor), and within 1e-8 of it once the
    first-order difference ((sim - obs)^2 - obs) / (2 k) is taken out (the particle test's bounds).  Measured: 2.0e-4 and 2.7e-9."""
    k = 1e6
    obs = np.arange(21.0)
    sims = np.arange(21.0) + 1e-10
    cells = twin_cells(mm, obs, sims, k)
    plain = first = 0.0
    for i, o in enumerate(obs):
        for j, s in enumerate(sims):
            sim = max(0.0, s - 1e-10) + 1e-10
            poisson = o * math.log(sim) - sim
            plain = max(plain, abs(cells[i, j] - poisson))
            first = max(first, abs(cells[i, j] - poisson - ((sim - o) ** 2 - o) / (2.0 * k)))
    print(f"k = 1e6: |cell - poisson| {plain:.3g}, after the first-order difference {first:.3g}")
    assert plain <= 2.1e-4 and first <= 1e-8


# ---- 5. sum order and special cases
def test_sum_order_and_special_cases(mm, oracle_py):
    rs = np.random.RandomState(3)
    B, T, n = 3, 7, 5
    inc = rs.gamma(2.0, 4.0, (B, T, 3, n)) - 1.5          # some negative: clamped at 0
    obs = [rs.poisson(lam, (T, n)).astype(float) for lam in (9.0, 2.0, 0.4)]
    k = np.array([[3.0, 0.5, 50.0], [INF, 7.0, INF], [INF, INF, INF]])
    base = mm.hostabi.nb_objective(inc, *obs, k)
    assert np.array_equal(base["status"], np.zeros(B, dtype=np.int32))
    # the Python pmf in the stated order (libm's lgamma against lgamma_pos: 1e-9)
    ref_ll, ref_parts = python_reference(inc, obs, k)
    np.testing.assert_allclose(base["ll_parts"], ref_parts, rtol=1e-9)
    np.testing.assert_allclose(base["loglik"], ref_ll, rtol=1e-9)
    assert np.array_equal(base["loglik"], (base["ll_parts"][:, 0] + base["ll_parts"][:, 1]) + base["ll_parts"][:, 2])
    # a series at +inf: the oracle's Poisson sum of that series, bit for bit
    for b in range(B):
        for s in range(3):
            if k[b, s] == INF:
                assert base["ll_parts"][b, s] == oracle_py.poisson_loglik(inc[b, :, s, :], obs[s]), (b, s)
    # the same bits from libsepaihrd_hip.so's compile of the text
    other = mm.hostabi.nb_objective(inc, *obs, k, lib="hip")
    for key in ("loglik", "ll_parts", "status"):
        assert np.array_equal(base[key], other[key]), key
    # a NaN, negative or infinite observation is skipped: the series' sum is that of the remaining cells
    spoiled = [o.copy() for o in obs]
    spoiled[0][2, 1], spoiled[0][4, 0], spoiled[2][6, 4] = NAN, -1.0, INF
    got = mm.hostabi.nb_objective(inc, *spoiled, k)
    _, ref_parts2 = python_reference(inc, spoiled, k)   # python_cell skips them
    np.testing.assert_allclose(got["ll_parts"], ref_parts2, rtol=1e-9)
    assert np.array_equal(got["ll_parts"][:, 1], base["ll_parts"][:, 1])
    assert not np.array_equal(got["ll_parts"][:, 0], base["ll_parts"][:, 0]) and not np.array_equal(got["ll_parts"][:, 2], base["ll_parts"][:, 2])
    # obs == 0: g is exactly 0, the cell is -k log(1 + sim / k) with the library's log
    zero = [np.zeros((T, n))] * 3
    gz = mm.hostabi.nb_objective(inc, *zero, k)
    for b in range(B):
        for s in range(3):
            if k[b, s] != INF:
                acc = 0.0
                for t in range(T):
                    row = 0.0
                    for a in range(n):
                        sim = max(0.0, inc[b, t, s, a]) + 1e-10
                        row += 0.0 * math.log(sim) - (0.0 + k[b, s]) * math.log(1.0 + sim / k[b, s])
                    acc += row
                assert gz["ll_parts"][b, s] == acc, (b, s)   # glibc_log is libm's log bit for bit: the same additions
    # a NaN increment: status 1 and lowest()
    bad = inc.copy()
    bad[1, 3, 1, 2] = NAN
    gb = mm.hostabi.nb_objective(bad, *obs, k)
    assert gb["status"].tolist() == [0, 1, 0] and gb["loglik"][1] == mm.LOWEST and gb["loglik"][0] == base["loglik"][0]


# ---- 6. validation
def _validate(mm, fields, idxs, lower, upper, has):
    lib = mm.hipabi.load_library()
    f, i = np.array(fields, dtype=np.int32), np.array(idxs, dtype=np.int32)
    lo, hi, hb = np.array(lower, dtype=np.float64), np.array(upper, dtype=np.float64), np.array(has, dtype=np.uint8)
    src = np.full(3, -7, dtype=np.int32)
    err = C.create_string_buffer(512)
    rc = lib.sepaihrd_dispersion_validate(len(fields), f.ctypes.data, i.ctypes.data, lo.ctypes.data, hi.ctypes.data, hb.ctypes.data,
                                          src.ctypes.data, err, len(err))
    return rc, err.value.decode(), src.tolist()


def test_validation_with_messages(mm, ref_fixture):
    assert _validate(mm, [0, 28, 28], [0, 2, 0], [0, 1e-3, 0.5], [1, 1e6, 0.5], [1, 1, 1]) == (0, "", [2, -1, 1])
    assert _validate(mm, [0, 1], [0, 0], [0, 0], [1, 1], [1, 1]) == (0, "", [-1, -1, -1])
    rc, msg, _ = _validate(mm, [0, 28], [0, 1], [0, 0.1], [1, 10.0], [1, 0])
    assert rc == -1 and msg == "param 1: dispersion of series ICU needs bounds: a calibrated k must stay finite in [1e-3, 1e6]"
    for lo, hi in ((1e-4, 10.0), (0.1, 2e6), (10.0, 1.0), (NAN, 1.0), (0.1, INF)):
        rc, msg, _ = _validate(mm, [28], [0], [lo], [hi], [1])
        assert rc == -1 and msg.startswith("param 0: dispersion of series H has bounds [") and \
            msg.endswith("they must satisfy 1e-3 <= lower <= upper <= 1e6"), msg
    rc, msg, _ = _validate(mm, [28, 0, 28], [2, 0, 2], [1, 0, 1], [2, 1, 2], [1, 1, 1])
    assert rc == -1 and msg == "param 2: dispersion of series D is already calibrated by param 0"
    rc, msg, _ = _validate(mm, [28], [3], [1], [2], [1])
    assert rc == -1 and msg == "param 0: dispersion index out of range (0 = H, 1 = ICU, 2 = D)"
    # sepaihrd_create applies the same rules before it looks for a device
    bad = with_dispersion(ref_fixture, ("dispersion_H",), bounds=(1e-5, 10.0))
    with pytest.raises(RuntimeError, match="dispersion of series H has bounds"):
        mm.HipObjective(bad)
    dup = with_dispersion(ref_fixture, ("dispersion_ICU",))
    dup = dup.with_(param_names=dup.param_names + ["dispersion_ICU"], base_theta=np.append(dup.base_theta, 5.0))
    with pytest.raises(RuntimeError, match="dispersion of series ICU is already calibrated by param 5"):
        mm.HipObjective(dup)
    unbounded = with_dispersion(ref_fixture, ("dispersion_D",))
    del unbounded.bounds["dispersion_D"]
    with pytest.raises(RuntimeError, match="dispersion of series D needs bounds"):
        mm.HipObjective(unbounded)
    # a bad fixed k: sepaihrd_set_dispersion takes the particle validator's verdict and message
    for k3, part in (((1.0, -2.0, INF), "dispersion[1] (k_ICU) = -2 is not positive"), ((1e-4, 1.0, 1.0), "dispersion[0] (k_H) = 0.0001 is below 1e-3"),
                     ((1.0, 1.0, 2e6), "dispersion[2] (k_D) = 2000000 is above 1e6"), ((NAN, 1.0, 1.0), "dispersion[0] (k_H) is NaN")):
        with pytest.raises(ValueError, match=part.replace("[", r"\[").replace("]", r"\]").replace("(", r"\(").replace(")", r"\)")):
            mm.hostabi.particle_nb_validate(k3)
    assert mm.hipabi.load_library().sepaihrd_set_dispersion(None, np.ones(3).ctypes.data) == -1


# ---- 7. the twin over the CPU oracle's trajectories
def oracle_reference(oracle_py, pb_plain, theta_plain, k):
    """(the Python likelihood, the twin's inputs) over the oracle's trajectories of the problem without its dispersion entries"""
    ref = oracle_py.Oracle(pb_plain).eval_batch(theta_plain, want_traj=True)
    inc = increments(ref["traj"], pb_plain.n)
    obs = observation_grid(pb_plain)
    ll, parts = python_reference(inc, obs, k)
    return {"loglik": ll, "ll_parts": parts, "status": ref["status"], "inc": inc, "obs": obs}


def test_twin_over_the_oracles_trajectories(mm, oracle_py, ref_fixture):
    pb = ref_fixture
    rs = np.random.RandomState(5)
    lo, hi, _ = pb.bounds_arrays()
    theta = lo + (hi - lo) * rs.uniform(0, 1, (5, pb.n_params))
    theta[0] = pb.base_theta
    k = np.array([[0.3, INF, 3.0], [2.0, 40.0, 3.0], [11.0, INF, INF], [150.0, 0.05, 1e6], [INF, INF, INF]])
    ref = oracle_reference(oracle_py, pb, theta, k)
    assert (ref["status"] == 0).all()
    got = mm.hostabi.nb_objective(ref["inc"], *ref["obs"], k)
    np.testing.assert_allclose(got["loglik"], ref["loglik"], rtol=1e-9)
    np.testing.assert_allclose(got["ll_parts"], ref["ll_parts"], rtol=1e-9)
    # the all-Poisson chain is the oracle's own objective
    plain = oracle_py.Oracle(pb).eval_batch(theta[4:5])
    assert got["loglik"][4] == plain["loglik"][0] and np.array_equal(got["ll_parts"][4], plain["ll_parts"][0])
