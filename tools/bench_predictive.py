#!/usr/bin/env python3
"""Time of the posterior predictive draws (sepaihrd_ensemble_predictive) on the GPU (diagnostic; not part of bench.py).

Runs on the GPU only, one process, one box.  The shipped problem (n = 4, 326 output times) at S = 1024 samples x R = 16
replicates (16 384 draws per segment: the LDS sort) and at S = 32 768 x R = 1 (the segmented radix sort).  Per shape:
  * the call's host wall time (allocation, upload and read-back of quantiles and PIT included) and the device time of its
    phases from the call's own events: integrator; draw kernel and mid-PIT counts; segment sorts and quantiles;
  * the wall time of a plain ensemble_quantiles call (bands of expectations, no seroprevalence) at the same S;
  * the host twin (the same sampler text, OpenMP on 16 threads, std::sort) fed the device's means, and whether it reproduces
    the device's quantiles and PIT bit for bit.
Every timed call is warmed up once; three repetitions (two of the host twin), the median is reported and the repetitions are
kept.  One JSON line per shape is appended to profiles/predictive_bench.jsonl.

    python tools/bench_predictive.py [--shapes 1024x16,32768x1] [--skip-host-twin] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THREADS = 16
REPS = 3
SEED = 20261018
PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]


def timed(run, reps=REPS):
    run()  # warm-up: code objects, the allocator, the host's thread pool
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = run()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,32768x1", help="comma-separated SxR")
    ap.add_argument("--skip-host-twin", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_bench.jsonl"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(THREADS))
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_predictive.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    obs = mm.hostabi.observed_table(pb)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in a.shapes.split(","):
        S, R = (int(x) for x in shape.split("x"))
        # S samples around the base point: 256 distinct jittered draws, repeated (a sample's stream is set by its position)
        distinct = mm.draws.jitter_draws(pb, 11, min(S, 256))
        theta = np.ascontiguousarray(distinct[np.arange(S) % len(distinct)])
        hip = mm.HipObjective(pb, device=0)
        hip.set_initial_state_mode(1)
        phases = []

        def device_run():
            out = hip.ensemble_predictive(theta, R, SEED, PROBS)
            phases.append(out["phase_ms"].tolist())
            return out

        wall, got = timed(device_run)
        med = np.median(np.array(phases[1:]), axis=0)
        pwall, _ = timed(lambda: hip.ensemble_quantiles(theta, PROBS, want_sero=False))
        Tp = got["pred"].shape[2]
        row = {"tool": "bench_predictive", "problem": "shipped", "n_age": pb.n, "n_times": pb.n_times, "T_pos": Tp, "S": S, "R": R,
               "draws_per_segment": got["n_valid"] * R, "segments": 6 * Tp * pb.n, "poisson_variates": got["n_valid"] * R * 3 * Tp * pb.n,
               "sort_path": "lds" if S * R <= 16384 else "segmented_radix", "device": torch.cuda.get_device_name(0), "seed": SEED,
               "wall_ms": float(np.median(wall)), "wall_ms_runs": wall,
               "integrator_ms": float(med[0]), "draw_and_pit_ms": float(med[1]), "sort_and_quantile_ms": float(med[2]),
               "phase_ms_runs": phases[1:],
               "plain_ensemble_quantiles_wall_ms": float(np.median(pwall)), "plain_ensemble_quantiles_wall_ms_runs": pwall,
               "n_valid": got["n_valid"], "mean_pit": float(np.nanmean(got["pit"]))}
        if not a.skip_host_twin:
            full = hip.ensemble_predictive(theta, R, SEED, PROBS, want_means=True)
            twall, twin = timed(lambda: mm.hostabi.predictive_from_means(full["means"], full["status"], obs, R, SEED, PROBS, want_draws=False),
                                reps=2)
            row.update({"twin_threads": THREADS, "twin_wall_ms": float(np.median(twall)), "twin_wall_ms_runs": twall,
                        "twin_over_device": float(np.median(twall) / np.median(wall)),
                        "twin_equals_device": bool(np.array_equal(twin["pred"], got["pred"], equal_nan=True) and
                                                   np.array_equal(twin["pit"], got["pit"], equal_nan=True))})
        print(json.dumps(row))
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        hip.close()


if __name__ == "__main__":
    main()
