#!/usr/bin/env python3
"""Writes tests/golden/mh_pin.json: four runs of hostabi.mh_analytic (MultiChainMetropolisHastings' scalar path over a correlated
Gaussian) and every array they return.  `plumbing` is the case of tests/test_mh_plumbing_cpu.py; `wide` proposes so widely that
nothing is accepted for the first 1000 iterations (the aggressive and the emergency branch of adaptGlobalScale, the lower clamp);
`recover` starts wide enough for the scale to come down to the floor region, where acceptance returns (the recovery branch);
`adapting` leaves burn-in early (rank-one updates and covariance refreshes).  Run it at a commit whose sampler is trusted;
tests/test_mh_pin_cpu.py replays the inputs and asserts the same bits.

    python tests/golden/make_mh_pin.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mmid_amd_loader  # noqa: E402
from test_mh_pin_cpu import encode, run_case, to_hex  # noqa: E402
from test_mh_plumbing_cpu import MEAN, PRECISION, RUN, STARTS  # noqa: E402

mm = mmid_amd_loader.load()
target = {"mean": to_hex(MEAN), "precision": to_hex(PRECISION)}
# few stored samples: the thinning of the long runs is a third of their length
inputs = {
    "plumbing": dict(target, initial=to_hex(STARTS), run=dict(RUN)),
    "wide": dict(target, initial=to_hex(STARTS[:2]),
                 run=dict(seed=23, iterations=1700, burn_in=1700, adaptation_period=100, thinning=600, sigma=1e8)),
    "recover": dict(target, initial=to_hex(STARTS[1:]),
                    run=dict(seed=41, iterations=1750, burn_in=1750, adaptation_period=100, thinning=600, sigma=300.0)),
    "adapting": dict(target, initial=to_hex(STARTS[:2]),
                     run=dict(seed=7, iterations=90, burn_in=8, adaptation_period=20, thinning=30, sigma=1.0)),
}
with open(os.path.join(HERE, "mh_pin.json"), "w") as fh:
    json.dump({"inputs": inputs, "outputs": {name: encode(run_case(mm, case)) for name, case in inputs.items()}}, fh, separators=(",", ":"))
    fh.write("\n")
