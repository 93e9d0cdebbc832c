#!/usr/bin/env python3
"""Writes tests/golden/twin_pin.json: a tiny stochastic SEPAIHRD problem (3 age classes, 5 output times of which the first is
negative, 2 kappa values with the end time inside the span, no beta schedule, 2 steps per interval), what hostStochasticSEPAIHRD,
hostParticleLoglik and hostParticleResample return for it, and the host manager's applyConstraints in both modes on the shipped
problem.  Run it at a commit whose twins are trusted; tests/test_twin_pin_cpu.py replays the inputs and asserts the same bits.

    python tests/golden/make_twin_pin.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mmid_amd_loader  # noqa: E402
from test_twin_pin_cpu import replay, to_hex  # noqa: E402

mm = mmid_amd_loader.load()
n = 3
x0 = np.zeros((11, n))
x0[:8] = [[900, 1500, 700], [10, 20, 5], [5, 5, 5], [3, 4, 5], [8, 2, 6], [2, 1, 3], [1, 0, 2], [4, 4, 4]]
rates = dict(theta=0.6, sigma=0.4, gamma_p=0.5, gamma_A=0.3, gamma_I=0.2, gamma_H=0.15, gamma_ICU=0.1, a=[0.8, 1.0, 1.2],
             h_infec=[1.0, 0.9, 1.1], p=[0.5, 0.4, 0.3], h=[0.05, 0.1, 0.2], icu=[0.05, 0.1, 0.15], d_H=[0.01, 0.02, 0.08],
             d_ICU=[0.05, 0.1, 0.2], d_community=[0.001, 0.01, 0.05])
rows = np.stack([mm.hostabi.stochastic_pack_values(n, x0, kappa_values=[1.0, 0.5], beta=beta, **rates) for beta in (0.9, 0.7, 1.1)])
obs = np.full((3, 4, n), np.nan)  # [series][output row t >= 0][age]: the last two rows, one cell missing
obs[:, 2:] = [[[3, 2, 4], [5, 1, 6]], [[1, 0, 1], [1, 1, 2]], [[0, 1, 2], [1, np.nan, 3]]]
pb = mm.SEPAIHRDProblem.load(os.path.join(HERE, "shipped_problem.json"))
lo, hi, _ = pb.bounds_arrays()
w = hi - lo
# per parameter: below the bounds, inside, beyond upper + twice the width, and a negative value (the manager bounds every
# parameter, so the rule's branch for a parameter without bounds is not reachable through it)
theta = np.stack([lo - 0.3 * w - 0.01, lo + 0.4 * w, hi + 2.3 * w + 0.01, -0.37 - np.arange(lo.size) / 16.0])
inputs = {
    "steps_per_interval": 2,
    "model": {"times": to_hex([-1.5, 0.0, 1.0, 2.0, 3.5]), "N": to_hex(x0[:9].sum(axis=0)),
              "M": to_hex([[3.0, 1.0, 0.5], [1.0, 2.0, 1.0], [0.5, 1.0, 1.5]]), "kappa_end_times": to_hex([1.7, 1e9]),
              "model_values": to_hex(rows)},
    "stochastic": {"S": 3, "R": 3, "keep": 2, "status": [0, 1, 0], "seed": 0x0BADCAFE12345678, "probs": to_hex([0.0, 0.5, 1.0])},
    "particle": {"B": 2, "J": 5, "seed": 0x5EED0F1E1D, "obs_H": to_hex(obs[0]), "obs_ICU": to_hex(obs[1]), "obs_D": to_hex(obs[2])},
    "resample": {"logw": to_hex([-3.25, -1.5, -40.0, -2.0, -1.75]), "seed": 0x5EED0F1E1D, "b": 1, "row": 3},
    "constraints": {"problem": "shipped_problem.json", "theta": to_hex(theta)},
}
with open(os.path.join(HERE, "twin_pin.json"), "w") as fh:
    json.dump({"inputs": inputs, "outputs": replay(mm, inputs)}, fh, separators=(",", ":"))
    fh.write("\n")
