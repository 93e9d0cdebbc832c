"""The CPU twins of the stochastic SEPAIHRD model and the host constraint rule, pinned to recorded bits.  The device-against-twin
tests compare two readers of ONE text (csrc/sepaihrd_stoch_sepaihrd.inc, csrc/sepaihrd_constrain.inc): a change to that text moves
both and passes them.  tests/golden/twin_pin.json holds what the twins returned before the interval walk and the constraint
rule were gathered into those files (tests/golden/make_twin_pin.py wrote it); this replays its inputs and asserts exact equality.
Doubles are stored as float.hex() strings.  No device."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "twin_pin.json")


def to_hex(a):
    """nested lists of float.hex() strings, the shape of `a`"""
    a = np.asarray(a, dtype=np.float64)
    return float(a).hex() if a.ndim == 0 else [to_hex(x) for x in a]


def from_hex(h):
    if isinstance(h, str):
        return float.fromhex(h)
    return np.array([from_hex(x) for x in h], dtype=np.float64)


def replay(mm, inputs) -> dict:
    """what the twins return for the fixture's inputs (every double as float.hex(), integers as they are)"""
    ha = mm.hostabi
    m = {k: from_hex(v) for k, v in inputs["model"].items()}
    fixed = (m["times"], m["N"], m["M"], m["kappa_end_times"])
    st = inputs["stochastic"]
    out = ha.stochastic_from_values(m["model_values"][:st["S"]], np.array(st["status"], dtype=np.int32), *fixed, st["R"],
                                    inputs["steps_per_interval"], st["seed"], from_hex(st["probs"]), keep=st["keep"])
    got = {"stochastic": {k: to_hex(out[k]) for k in ("traj", "final_state", "quantiles", "extinct")}}
    pf = inputs["particle"]
    obs = [from_hex(pf[k]) for k in ("obs_H", "obs_ICU", "obs_D")]
    out = ha.particle_from_values(m["model_values"][:pf["B"]], np.zeros(pf["B"], dtype=np.int32), *fixed, *obs, pf["J"],
                                  inputs["steps_per_interval"], pf["seed"])
    got["particle"] = {k: to_hex(out[k]) for k in ("loglik", "increments", "ess", "final_state")}
    rs = inputs["resample"]
    out = ha.particle_resample(from_hex(rs["logw"]), rs["seed"], rs["b"], rs["row"])
    got["resample"] = {"ancestors": [int(a) for a in out["ancestors"]], "increment": to_hex(out["increment"]), "ess": to_hex(out["ess"])}
    pb = mm.SEPAIHRDProblem.load(os.path.join(GOLDEN, inputs["constraints"]["problem"]))
    h = mm.HostObjective(pb, with_objective=False)
    theta = from_hex(inputs["constraints"]["theta"])
    got["constraints"] = {"clamp": to_hex(h.apply_constraints(theta, 0)), "reflect": to_hex(h.apply_constraints(theta, 1))}
    return got


@pytest.fixture(scope="module")
def pinned(mm):
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    return fx, replay(mm, fx["inputs"])


def same(got, want, equal_nan=False):
    g, w = from_hex(got), from_hex(want)
    assert np.shape(g) == np.shape(w)
    assert np.array_equal(g, w, equal_nan=equal_nan)
    assert np.array_equal(np.signbit(g), np.signbit(w))  # -0.0 is not 0.0 here


def test_inputs_are_the_case_the_pin_is_for(pinned):
    fx, _ = pinned
    inp = fx["inputs"]
    times = from_hex(inp["model"]["times"])
    assert len(times) == 5 and (times < 0).sum() == 1 and inp["steps_per_interval"] == 2
    assert np.shape(from_hex(inp["model"]["M"])) == (3, 3) and len(inp["model"]["kappa_end_times"]) == 2
    assert times[0] < from_hex(inp["model"]["kappa_end_times"])[0] < times[-1]
    st, pf = inp["stochastic"], inp["particle"]
    assert (st["S"], st["R"], st["keep"], st["status"]) == (3, 3, 2, [0, 1, 0]) and list(from_hex(st["probs"])) == [0.0, 0.5, 1.0]
    assert (pf["B"], pf["J"]) == (2, 5) and len(inp["resample"]["logw"]) == 5
    obs = np.stack([from_hex(pf[k]) for k in ("obs_H", "obs_ICU", "obs_D")])  # [3][T_pos][n]: the last two rows, one NaN cell
    assert np.isnan(obs[:, :2]).all() and np.isnan(obs[:, 2:]).sum() == 1


def test_stochastic_twin_returns_the_recorded_bits(pinned):
    fx, got = pinned
    want = fx["outputs"]["stochastic"]
    for k in ("traj", "final_state", "quantiles", "extinct"):  # NaN: the invalid sample's rows
        same(got["stochastic"][k], want[k], equal_nan=k != "quantiles")
    assert np.isnan(from_hex(want["traj"])[1]).all() and np.isnan(from_hex(want["extinct"])[1])
    assert np.isfinite(from_hex(want["traj"])[[0, 2]]).all()


def test_particle_twin_returns_the_recorded_bits(pinned):
    fx, got = pinned
    want = fx["outputs"]["particle"]
    same(got["particle"]["loglik"], want["loglik"])
    same(got["particle"]["increments"], want["increments"])
    same(got["particle"]["ess"], want["ess"], equal_nan=True)  # NaN: the rows without a usable observation
    same(got["particle"]["final_state"], want["final_state"])
    assert np.isfinite(from_hex(want["loglik"])).all() and (from_hex(want["increments"])[:, 2:] != 0).all()


def test_resampling_twin_returns_the_recorded_bits(pinned):
    fx, got = pinned
    want = fx["outputs"]["resample"]
    assert got["resample"]["ancestors"] == want["ancestors"]
    same(got["resample"]["increment"], want["increment"])
    same(got["resample"]["ess"], want["ess"])


def test_host_constraints_return_the_recorded_bits(mm, pinned):
    fx, got = pinned
    for mode in ("clamp", "reflect"):
        same(got["constraints"][mode], fx["outputs"]["constraints"][mode])
    # the vector holds what it is meant to: per parameter one value below, one inside, one beyond twice the width
    pb = mm.SEPAIHRDProblem.load(os.path.join(GOLDEN, fx["inputs"]["constraints"]["problem"]))
    lo, hi, _ = pb.bounds_arrays()
    theta = from_hex(fx["inputs"]["constraints"]["theta"])
    wide = hi > lo
    assert wide.any() and (theta[0] < lo).all()
    assert ((theta[1] >= lo) & (theta[1] <= hi)).all() and (theta[2][wide] > (hi + 2 * (hi - lo))[wide]).all()
    assert (theta[3] < 0).all()
