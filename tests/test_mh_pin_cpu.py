"""The Adaptive-Metropolis sampler's scalar path pinned to recorded bits, and its scale rule replayed independently.  The device
tests compare readers of ONE text (csrc/sepaihrd_adapt_scale.inc): a change to that text moves all of them and passes them.
tests/golden/mh_pin.json holds what hostabi.mh_analytic returned before the rule was gathered into that file
(tests/golden/make_mh_pin.py wrote it); this replays its inputs and asserts exact equality of every array.  Doubles are stored
as float.hex() strings.  No device.

The replay restates adaptGlobalScale from the reference (MetropolisHastingsSampler.cpp:104-152) over nothing but the accept
trace and must give final_scale of every chain of the burn-in-only cases exactly; it counts the branches it takes.  The recovery
branch (:146-148, scale <= 0.011 with the windowed rate between 0.15 and 0.30) fires on the analytic target too -- in the
`recover` case, once the scale has come down to where proposals are accepted again -- so it is demanded here like the others."""
import json
import math
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "mh_pin.json")
ARRAYS = ("accepted", "best_value", "best", "final_scale", "accept_trace", "samples", "sample_values", "final_cov")
TARGET_RATE = 0.234  # MultiChainMetropolisHastings::configure's default, which mh_analytic leaves alone


def to_hex(a):
    a = np.asarray(a, dtype=np.float64)
    return float(a).hex() if a.ndim == 0 else [to_hex(x) for x in a]


def from_hex(h):
    if isinstance(h, str):
        return float.fromhex(h)
    return np.array([from_hex(x) for x in h], dtype=np.float64)


def run_case(mm, case) -> dict:
    return mm.hostabi.mh_analytic(from_hex(case["mean"]), from_hex(case["precision"]), from_hex(case["initial"]), **case["run"])


def encode(out) -> dict:
    """integer arrays as nested lists, doubles as float.hex()"""
    return {k: out[k].tolist() if out[k].dtype.kind in "iu" else to_hex(out[k]) for k in ARRAYS}


def replay_scale(trace, counts) -> float:
    """adaptGlobalScale (:104-152) for t = 1, 2, .. over one chain's accept flags: the final global_scale_"""
    recent, log_scale, scale = [], 0.0, 1.0
    for t, flag in enumerate((int(f) for f in trace), start=1):
        recent.append(flag)                                        # :107-110
        if len(recent) > 1000:
            recent.pop(0)
        rate = sum(recent) / len(recent)
        if len(recent) >= 1000 and rate < 0.001:                   # :118-123
            log_scale -= 0.7
            counts["emergency"] += 1
        elif rate < 0.02 and len(recent) >= 500:                   # :126-132
            log_scale += min(5.0 / math.sqrt(t + 1.0), 0.3) * (0.0 - TARGET_RATE)
            counts["aggressive"] += 1
        else:                                                      # :134-141
            log_scale += min(1.0 / math.sqrt(t + 1.0), 0.1) * (float(flag) - TARGET_RATE)
            counts["ordinary"] += 1
        if scale <= 0.011 and 0.15 < rate < 0.30:                  # :146-148
            log_scale += 0.01
            counts["recovery"] += 1
        if log_scale < -6.9:                                       # :150-151
            counts["lower_clamp"] += 1
        log_scale = max(min(log_scale, 2.3), -6.9)
        scale = math.exp(log_scale)
    return scale


@pytest.fixture(scope="module")
def pinned(mm):
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    return fx, {name: run_case(mm, case) for name, case in fx["inputs"].items()}


def test_inputs_are_the_cases_the_pin_is_for(pinned):
    fx, _ = pinned
    inp, out = fx["inputs"], fx["outputs"]
    assert set(inp) == {"plumbing", "wide", "recover", "adapting"}
    assert (len(inp["plumbing"]["initial"]), inp["plumbing"]["run"]["iterations"]) == (3, 25)
    for name in ("wide", "recover"):
        run = inp[name]["run"]
        assert len(inp[name]["initial"]) == 2 and run["iterations"] >= 1700 and run["burn_in"] == run["iterations"]
    assert not np.array(out["wide"]["accept_trace"])[:, :1000].any()
    assert np.array(out["recover"]["accept_trace"])[:, -500:].mean() > 0.1
    run = inp["adapting"]["run"]  # the rank-one update from burn_in on, and a refresh over at least P + 10 states
    assert run["burn_in"] < run["adaptation_period"] < run["iterations"] and run["adaptation_period"] >= 2 + 10


@pytest.mark.parametrize("name", ["plumbing", "wide", "recover", "adapting"])
def test_scalar_path_returns_the_recorded_bits(pinned, name):
    fx, got = pinned
    want = fx["outputs"][name]
    for k in ARRAYS:
        g = got[name][k]
        w = np.array(want[k], dtype=g.dtype) if g.dtype.kind in "iu" else from_hex(want[k])
        assert g.shape == w.shape, k
        assert np.array_equal(g, w), k
        if g.dtype.kind == "f":
            assert np.array_equal(np.signbit(g), np.signbit(w)), k


def test_scale_rule_replayed_from_the_accept_trace(pinned):
    _, got = pinned
    counts = dict.fromkeys(("emergency", "aggressive", "ordinary", "recovery", "lower_clamp"), 0)
    for name in ("wide", "recover"):
        for c, trace in enumerate(got[name]["accept_trace"]):
            assert replay_scale(trace, counts) == got[name]["final_scale"][c], (name, c)
    assert all(n > 0 for n in counts.values()), counts
