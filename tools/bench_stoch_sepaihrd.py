#!/usr/bin/env python3
"""Time of the stochastic chain-binomial SEPAIHRD ensembles (sepaihrd_ensemble_stochastic) on the GPU (diagnostic; not part of
bench.py).

Runs on the GPU only, one process, one box.  The shipped problem (n = 4, 326 output times, x(t0) seeded from theta) at S = 1024
samples x R = 16 replicates (16 384 values per segment: the LDS sort) and at S = 4096 x R = 4, with m = 4 steps per output
interval.  Per shape:
  * the call's host wall time (allocation, upload and read-back of the quantiles and the extinction shares included) and the
    device time of its two phases from the call's own events: step kernel; segment sorts and quantiles;
  * the host twin (the same model text, OpenMP on 16 threads, std::sort) fed the device's model values, and whether it
    reproduces the device's quantiles and extinction shares bit for bit.
Every timed call is warmed up once; three repetitions (two of the host twin), the median is reported and the repetitions are
kept.  Then, reported and not asserted: the relative difference between the replicate mean of the total deaths at the last time
and the deterministic integration's mean over the same samples, at m = 1, 4 and 16 (256 samples x 16 replicates).  One JSON
line per shape and one for the comparison are appended to profiles/stoch_sepaihrd_bench.jsonl.

    python tools/bench_stoch_sepaihrd.py [--shapes 1024x16,4096x4] [--steps 4] [--skip-host-twin] [--out FILE]
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


def thetas(mm, pb, S):
    # S samples around the base point: 256 distinct jittered draws, repeated (a sample's stream is set by its position)
    distinct = mm.draws.jitter_draws(pb, 11, min(S, 256))
    return np.ascontiguousarray(distinct[np.arange(S) % len(distinct)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,4096x4", help="comma-separated SxR")
    ap.add_argument("--steps", type=int, default=4, help="steps per output interval")
    ap.add_argument("--skip-host-twin", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoch_sepaihrd_bench.jsonl"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(THREADS))
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_stoch_sepaihrd.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    device = torch.cuda.get_device_name(0)
    m = a.steps
    for shape in a.shapes.split(","):
        S, R = (int(x) for x in shape.split("x"))
        theta = thetas(mm, pb, S)
        hip = mm.HipObjective(pb, device=0)
        phases = []

        def device_run():
            out = hip.ensemble_stochastic(theta, R, m, SEED, PROBS)
            phases.append(out["phase_ms"].tolist())
            return out

        wall, got = timed(device_run)
        med = np.median(np.array(phases[1:]), axis=0)
        Tp = got["quantiles"].shape[2]
        steps = (pb.n_times - 1) * m
        row = {"tool": "bench_stoch_sepaihrd", "problem": "shipped", "n_age": pb.n, "n_times": pb.n_times, "T_pos": Tp, "S": S, "R": R,
               "steps_per_interval": m, "values_per_segment": got["n_valid"] * R, "segments": 6 * Tp * pb.n,
               "replicate_steps": got["n_valid"] * R * steps, "binomial_draws": got["n_valid"] * R * steps * pb.n * 13,
               "sort_path": "lds" if S * R <= 16384 else "segmented_radix", "device": device, "seed": SEED,
               "wall_ms": float(np.median(wall)), "wall_ms_runs": wall, "step_kernel_ms": float(med[0]), "sort_and_quantile_ms": float(med[1]),
               "phase_ms_runs": phases[1:], "replicate_steps_per_s": got["n_valid"] * R * steps / (float(med[0]) * 1e-3),
               "n_valid": got["n_valid"], "mean_extinct": float(np.nanmean(got["extinct"]))}
        if not a.skip_host_twin:
            full = hip.ensemble_stochastic(theta, R, m, SEED, PROBS, want_values=True)
            twall, twin = timed(lambda: mm.hostabi.stochastic_from_values(full["model_values"], full["status"], pb.times, pb.N, pb.M, pb.kappa_end_times,
                                                                          R, m, SEED, PROBS, beta_end_times=pb.beta_end_times, want_final=False),
                                reps=2)
            row.update({"twin_threads": THREADS, "twin_wall_ms": float(np.median(twall)), "twin_wall_ms_runs": twall,
                        "twin_over_device": float(np.median(twall) / np.median(wall)),
                        "twin_equals_device": bool(np.array_equal(twin["quantiles"], got["quantiles"], equal_nan=True) and
                                                   np.array_equal(twin["extinct"], got["extinct"], equal_nan=True))})
        print(json.dumps(row))
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        hip.close()

    # process noise against the deterministic integration: total deaths at the last time
    S, R = 256, 16
    theta = thetas(mm, pb, S)
    hip = mm.HipObjective(pb, device=0)
    det = hip.eval_batch(theta, want_traj=True)
    ok = det["status"] == 0
    det_deaths = det["traj"].reshape(S, pb.n_times, 11, pb.n)[:, -1, 8].sum(axis=1)
    row = {"tool": "bench_stoch_sepaihrd", "problem": "shipped", "comparison": "total deaths at the last time", "S": S, "R": R, "device": device,
           "seed": SEED, "deterministic_mean": float(det_deaths[ok].mean()), "by_steps_per_interval": {}}
    for mm_steps in (1, 4, 16):
        got = hip.ensemble_stochastic(theta, R, mm_steps, SEED, PROBS, want_final=True)
        both = ok & (got["status"] == 0)
        sto = got["final_state"][:, :, 8].sum(axis=2)  # [S][R]
        mean = float(sto[both].mean())
        ref = float(det_deaths[both].mean())
        row["by_steps_per_interval"][str(mm_steps)] = {"replicate_mean": mean, "deterministic_mean": ref, "relative_difference": (mean - ref) / ref,
                                                       "mean_extinct": float(np.nanmean(got["extinct"])), "samples": int(both.sum())}
    print(json.dumps(row))
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")
    hip.close()


if __name__ == "__main__":
    main()
