#!/usr/bin/env python3
"""Time of the posterior predictive draws under the negative-binomial observation model (sepaihrd_ensemble_predictive_nb) on the
GPU against the Poisson call (sepaihrd_ensemble_predictive) on the same samples (diagnostic; not part of bench.py).

Runs on the GPU only, one process, one box.  The shipped problem (n = 4, 326 output times) at the two shapes of
tools/bench_predictive.py: S = 1024 samples x R = 16 replicates (16 384 draws per segment: the LDS sort) and S = 32 768 x R = 1
(the segmented radix sort).  Per shape three dispersions through the new call:
  * k = 10 for the three series: a gamma variate in front of every Poisson variate;
  * k = (10, 10, +inf): one series left Poisson;
  * all +inf: the Poisson call's draws in the new call's lane mapping -- one lane per (draw, age, series) against one lane per
    draw -- and so the one measurement of that mapping against the present one.
Each is launched alternately with the Poisson call in the same process, REPS pairs after one warm-up pair; per call the host
wall time and the device time of its phases from the call's own events (sepaihrd_predictive_timing: integrator; draw kernel and
mid-PIT counts; segment sorts and quantiles).  Medians are reported, the repetitions kept; the all-+inf row also says whether
the two calls' outputs were the same bits.  One JSON line per (shape, dispersion) is appended to profiles/predictive_nb_bench.jsonl.

    python tools/bench_predictive_nb.py [--shapes 1024x16,32768x1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
SEED = 20261021
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
INF = float("inf")
CASES = (("k10", (10.0, 10.0, 10.0)), ("k10_one_poisson", (10.0, 10.0, INF)), ("all_inf", (INF, INF, INF)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,32768x1", help="comma-separated SxR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_nb_bench.jsonl"))
    a = ap.parse_args()
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_predictive_nb.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in a.shapes.split(","):
        S, R = (int(x) for x in shape.split("x"))
        distinct = mm.draws.jitter_draws(pb, 11, min(S, 256))
        theta = np.ascontiguousarray(distinct[np.arange(S) % len(distinct)])
        hip = mm.HipObjective(pb, device=0)
        hip.set_initial_state_mode(1)
        for name, disp in CASES:
            wall = {"nb": [], "poisson": []}
            phase = {"nb": [], "poisson": []}
            last = {}
            for rep in range(REPS + 1):  # the first pair warms up
                for which in ("poisson", "nb"):
                    t0 = time.perf_counter()
                    out = hip.ensemble_predictive(theta, R, SEED, PROBS, dispersion=disp if which == "nb" else None)
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep > 0:
                        wall[which].append(dt)
                        phase[which].append(out["phase_ms"].tolist())
                    last[which] = out
            med = {w: np.median(np.array(phase[w]), axis=0) for w in phase}
            Tp = last["nb"]["pred"].shape[2]
            row = {"tool": "bench_predictive_nb", "problem": "shipped", "n_age": pb.n, "T_pos": Tp, "S": S, "R": R, "case": name,
                   "dispersion": [None if np.isinf(k) else k for k in disp], "variates": last["nb"]["n_valid"] * R * 3 * Tp * pb.n,
                   "sort_path": "lds" if S * R <= 16384 else "segmented_radix", "device": torch.cuda.get_device_name(0), "seed": SEED,
                   "reps": REPS}
            for w in ("nb", "poisson"):
                row.update({f"{w}_wall_ms": float(np.median(wall[w])), f"{w}_integrator_ms": float(med[w][0]),
                            f"{w}_draw_and_pit_ms": float(med[w][1]), f"{w}_sort_and_quantile_ms": float(med[w][2]),
                            f"{w}_wall_ms_runs": wall[w], f"{w}_phase_ms_runs": phase[w]})
            row["draw_and_pit_nb_over_poisson"] = float(med["nb"][1] / med["poisson"][1])
            row["mean_pit_nb"] = float(np.nanmean(last["nb"]["pit"]))
            row["mean_pit_poisson"] = float(np.nanmean(last["poisson"]["pit"]))
            if name == "all_inf":
                row["same_bits_as_poisson_call"] = bool(np.array_equal(last["nb"]["pred"], last["poisson"]["pred"], equal_nan=True) and
                                                        np.array_equal(last["nb"]["pit"], last["poisson"]["pit"], equal_nan=True))
            print(json.dumps(row))
            with open(a.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        hip.close()


if __name__ == "__main__":
    main()
