#!/usr/bin/env python3
"""Time of the posterior predictive scores on window and age-group totals (sepaihrd_ensemble_predictive_targets) on the GPU
against its sibling sepaihrd_ensemble_predictive_scores on the same samples (diagnostic; not part of bench.py).

Runs on the GPU only, one process, one box.  The shipped problem (n = 4, 326 output times, 306 of them >= 0) at the two shapes of
tools/bench_predictive_scores.py: S = 1024 samples x R = 16 replicates (16 384 draws per segment: the LDS sort) and
S = 32 768 x R = 1 (the segmented radix sort); k = 10 for the three series, levels 0.5, 0.9, 0.95.  Three groupings: w = 7 with
one all-ages group, w = 7 with a group per age, and the identity grouping (w = 1, a group per age: the sibling's own cells).  The
two calls are launched alternately in the same process, REPS pairs after one warm-up pair; per call the host wall time and the
device time of its phases from the call's own events (sepaihrd_predictive_timing: integrator; draws -- summed into the targets
in the new call; segment sorts, quantiles and scores).  Medians are reported, the repetitions kept, with the ratios new / sibling
of phases 1 and 2 and the ratio of the segment counts (6 W G against 6 T_pos n).  The row says whether k_used and status had the
sibling's bits in every pair.  The host twin (hostabi.predictive_targets_from_means) runs once per shape and weekly grouping on the
threads OMP_NUM_THREADS gives it, from the device's means.  One JSON line per shape and grouping is appended to
profiles/predictive_targets_bench.jsonl.

    OMP_NUM_THREADS=16 python tools/bench_predictive_targets.py [--shapes 1024x16,32768x1] [--out FILE] [--no-twin]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_targets_bench.jsonl"))
    ap.add_argument("--no-twin", action="store_true", help="leave the host twin out")
    a = ap.parse_args()
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_predictive_targets.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    n = pb.n
    groupings = (("weekly_all_ages", [0] * n, 7), ("weekly_each_age", list(range(n)), 7), ("identity", list(range(n)), 1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in a.shapes.split(","):
        S, R = (int(x) for x in shape.split("x"))
        distinct = mm.draws.jitter_draws(pb, 11, min(S, 256))
        theta = np.ascontiguousarray(distinct[np.arange(S) % len(distinct)])
        hip = mm.HipObjective(pb, device=0)
        hip.set_initial_state_mode(1)
        for name, groups, window in groupings:
            calls = {"scores": lambda: hip.ensemble_predictive_scores(theta, R, SEED, PROBS, LEVELS, dispersion=DISPERSION),
                     "targets": lambda: hip.ensemble_predictive_targets(theta, R, SEED, PROBS, LEVELS, groups, window, dispersion=DISPERSION)}
            wall = {w: [] for w in calls}
            phase = {w: [] for w in calls}
            last = {}
            same = True
            for rep in range(REPS + 1):  # the first pair warms up
                for which in ("scores", "targets"):
                    t0 = time.perf_counter()
                    out = calls[which]()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep > 0:
                        wall[which].append(dt)
                        phase[which].append(out["phase_ms"].tolist())
                    last[which] = out
                same = same and last["targets"]["n_valid"] == last["scores"]["n_valid"] and all(
                    np.array_equal(last["targets"][k], last["scores"][k], equal_nan=True) for k in ("k_used", "status"))
                if name == "identity":  # there every target is one of the sibling's cells
                    same = same and np.array_equal(last["targets"]["target_quantiles"], last["scores"]["pred"]) and np.array_equal(
                        last["targets"]["target_scores"][:3], last["scores"]["cell_scores"], equal_nan=True)
            med = {w: np.median(np.array(phase[w]), axis=0) for w in phase}
            got = last["targets"]
            Tp = last["scores"]["pred"].shape[2]
            W, G = got["W"], got["G"]
            row = {"tool": "bench_predictive_targets", "problem": "shipped", "n_age": n, "T_pos": Tp, "S": S, "R": R, "dispersion": list(DISPERSION),
                   "levels": LEVELS, "grouping": name, "age_group": groups, "window": window, "origin": 0, "W": W, "G": G,
                   "draws_per_segment": got["n_valid"] * R, "target_segments": 6 * W * G, "sibling_segments": 6 * Tp * n,
                   "segment_ratio": 6 * W * G / (6 * Tp * n), "sort_path": "lds" if S * R <= 16384 else "segmented_radix",
                   "device": torch.cuda.get_device_name(0), "seed": SEED, "reps": REPS, "exact": got["exact"]}
            for w in ("targets", "scores"):
                row.update({f"{w}_wall_ms": float(np.median(wall[w])), f"{w}_integrator_ms": float(med[w][0]), f"{w}_draw_ms": float(med[w][1]),
                            f"{w}_sort_ms": float(med[w][2]), f"{w}_wall_ms_runs": wall[w], f"{w}_phase_ms_runs": phase[w]})
            row["draw_targets_over_draw_scores"] = float(med["targets"][1] / med["scores"][1])
            row["sort_score_targets_over_sort_score_scores"] = float(med["targets"][2] / med["scores"][2])
            row["shared_outputs_same_bits_in_every_pair"] = bool(same)
            row["pooled_wis"] = got["summary_wis"][:, G].tolist()
            row["pooled_coverage"] = got["summary_coverage"][:, :, G].tolist()
            if not a.no_twin and name != "identity":
                again = hip.ensemble_predictive_targets(theta, R, SEED, PROBS, LEVELS, groups, window, dispersion=DISPERSION, want_means=True)
                t0 = time.perf_counter()
                twin = mm.hostabi.predictive_targets_from_means(again["means"], again["status"], mm.hostabi.observed_table(pb), R, SEED, PROBS,
                                                                LEVELS, groups, window, k_used=again["k_used"], want_draws=False,
                                                                want_target_draws=False)
                row["twin_seconds"] = time.perf_counter() - t0
                row["twin_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
                # where exact is False the sums of a cumulative target may round, and the twin's bits are then not promised
                row["twin_exact"] = twin["exact"]
                row["twin_same_bits"] = {k: bool(np.array_equal(twin[k], again[k], equal_nan=True))
                                         for k in ("target_scores", "summary", "pit", "target_quantiles", "target_obs")}
                row["twin_same_bits_window_totals"] = bool(np.array_equal(twin["target_scores"][:3], again["target_scores"][:3], equal_nan=True))
                close = np.isclose(twin["target_scores"], again["target_scores"], rtol=1e-12, atol=0.0, equal_nan=True)
                row["twin_within_1e-12"] = bool(close.all())
            print(json.dumps(row))
            with open(a.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        hip.close()


if __name__ == "__main__":
    main()
