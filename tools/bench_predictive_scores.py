#!/usr/bin/env python3
"""Time of the scored posterior predictive call (sepaihrd_ensemble_predictive_scores) on the GPU against its sibling
sepaihrd_ensemble_predictive_nb on the same samples (diagnostic; not part of bench.py).

Runs on the GPU only, one process, one box.  The shipped problem (n = 4, 326 output times) at the two shapes of
tools/bench_predictive.py: S = 1024 samples x R = 16 replicates (16 384 draws per segment: the LDS sort, scored in LDS) and
S = 32 768 x R = 1 (the segmented radix sort, scored over its scratch); k = 10 for the three series, levels 0.5, 0.9, 0.95.  The
two calls are launched alternately in the same process, REPS pairs after one warm-up pair; per call the host wall time and the
device time of its phases from the call's own events (sepaihrd_predictive_timing: integrator; draws and counts -- with the mid-PIT
pass in the sibling, without it in the scored call; segment sorts and quantiles -- and the scores in the scored call).  Medians are
reported, the repetitions kept, with the two ratios scored / sibling of phases 1 and 2.  The host twin
(hostabi.predictive_scores_from_means) runs once per shape on the threads OMP_NUM_THREADS gives it, from the device's means, and
the row says how long it took and whether it gave the same bits.  One JSON line per shape is appended to
profiles/predictive_scores_bench.jsonl.

    OMP_NUM_THREADS=16 python tools/bench_predictive_scores.py [--shapes 1024x16,32768x1] [--out FILE] [--no-twin]
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
LEVELS = [0.5, 0.9, 0.95]
DISPERSION = (10.0, 10.0, 10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,32768x1", help="comma-separated SxR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_scores_bench.jsonl"))
    ap.add_argument("--no-twin", action="store_true", help="leave the host twin out")
    a = ap.parse_args()
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_predictive_scores.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in a.shapes.split(","):
        S, R = (int(x) for x in shape.split("x"))
        distinct = mm.draws.jitter_draws(pb, 11, min(S, 256))
        theta = np.ascontiguousarray(distinct[np.arange(S) % len(distinct)])
        hip = mm.HipObjective(pb, device=0)
        hip.set_initial_state_mode(1)
        calls = {"nb": lambda: hip.ensemble_predictive(theta, R, SEED, PROBS, dispersion=DISPERSION),
                 "scores": lambda: hip.ensemble_predictive_scores(theta, R, SEED, PROBS, LEVELS, dispersion=DISPERSION)}
        wall = {w: [] for w in calls}
        phase = {w: [] for w in calls}
        last = {}
        for rep in range(REPS + 1):  # the first pair warms up
            for which in ("nb", "scores"):
                t0 = time.perf_counter()
                out = calls[which]()
                dt = (time.perf_counter() - t0) * 1e3
                if rep > 0:
                    wall[which].append(dt)
                    phase[which].append(out["phase_ms"].tolist())
                last[which] = out
        med = {w: np.median(np.array(phase[w]), axis=0) for w in phase}
        got = last["scores"]
        Tp = got["pred"].shape[2]
        n = pb.n
        row = {"tool": "bench_predictive_scores", "problem": "shipped", "n_age": n, "T_pos": Tp, "S": S, "R": R, "dispersion": list(DISPERSION),
               "levels": LEVELS, "draws_per_segment": got["n_valid"] * R, "scored_segments": 3 * Tp * n,
               "sort_path": "lds" if S * R <= 16384 else "segmented_radix", "device": torch.cuda.get_device_name(0), "seed": SEED, "reps": REPS,
               "exact": got["exact"]}
        for w in ("scores", "nb"):
            row.update({f"{w}_wall_ms": float(np.median(wall[w])), f"{w}_integrator_ms": float(med[w][0]), f"{w}_draw_ms": float(med[w][1]),
                        f"{w}_sort_ms": float(med[w][2]), f"{w}_wall_ms_runs": wall[w], f"{w}_phase_ms_runs": phase[w]})
        row["sort_quantile_score_over_sort_quantile"] = float(med["scores"][2] / med["nb"][2])
        row["draw_without_pit_over_draw_with_pit"] = float(med["scores"][1] / med["nb"][1])
        row["same_bits_as_sibling"] = bool(all(np.array_equal(got[k], last["nb"][k], equal_nan=True) for k in ("pred", "pit", "k_used", "status")))
        row["pooled_crps"] = got["summary_crps"][:, n].tolist()
        row["pooled_wis"] = got["summary_wis"][:, n].tolist()
        row["pooled_coverage"] = got["summary_coverage"][:, :, n].tolist()
        if not a.no_twin:
            again = hip.ensemble_predictive_scores(theta, R, SEED, PROBS, LEVELS, dispersion=DISPERSION, want_means=True)
            t0 = time.perf_counter()
            twin = mm.hostabi.predictive_scores_from_means(again["means"], again["status"], again["observed"], R, SEED, PROBS, LEVELS,
                                                           k_used=again["k_used"], want_draws=False)
            row["twin_seconds"] = time.perf_counter() - t0
            row["twin_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
            row["twin_same_bits"] = bool(twin["exact"] == again["exact"] and all(
                np.array_equal(twin[k], again[k], equal_nan=True) for k in ("cell_scores", "summary", "pit", "pred")))
        print(json.dumps(row))
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        hip.close()


if __name__ == "__main__":
    main()
