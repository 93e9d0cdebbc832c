"""The device buffers sepaihrd_ensemble_quantiles and sepaihrd_scenario_ensemble keep with their context, shared by role:
one context that serves both in turn gives what a context of its own gives for every call."""
import numpy as np
import pytest


def _hip(mm, pb):
    hip = mm.HipObjective(pb)
    hip.set_initial_state_mode(1)
    return hip


@pytest.mark.gpu
def test_one_context_serves_quantiles_and_scenarios_in_turn(mm, oracle_py, synth400):
    """Every shared buffer grows on the way (S = 70, then K = 2 scenarios of S = 33) and is reused larger than needed
    afterwards (S = 33 again); seroprevalence, Rt and the metric table are asked for, so every role is in use.  Each call
    equals, bit for bit, the same call on a fresh context."""
    pb = synth400.with_(arith=mm.ARITH_FMA)
    probs = [0.05, 0.5, 0.95]
    theta = oracle_py.Oracle(pb).jitter_draws(pb.base_theta, 11, 70, mode=1)
    table = np.ones((2, len(pb.kappa_values)))
    table[1, 1] = 0.8
    calls = [lambda h: h.ensemble_quantiles(theta, probs, want_sero=True, want_rt=True, want_metrics=True),
             lambda h: h.scenario_ensemble(theta[:33], table, probs, want_sero=True, want_rt=True),
             lambda h: h.ensemble_quantiles(theta[:33], probs, want_sero=True, want_rt=True, want_metrics=True)]
    shared = _hip(mm, pb)
    for i, call in enumerate(calls):
        got, fresh = call(shared), call(_hip(mm, pb))
        assert got.keys() == fresh.keys()
        for key in fresh:
            assert np.array_equal(got[key], fresh[key], equal_nan=True), (i, key)
    assert (got["status"] == 0).any()
