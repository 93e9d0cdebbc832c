#!/usr/bin/env python3
"""Time of the bootstrap particle filter of the stochastic SEPAIHRD model (sepaihrd_particle_loglik) on the GPU (diagnostic; not
part of bench.py, run by no test).

Runs on the GPU only, one process, one box.  The shipped problem (n = 4, 326 output times, x(t0) seeded from theta) with m = 4
steps per output interval at B = 256 and 4096 parameter vectors, J = 64 particles and J = sepaihrd_particle_max_particles(4).
Per shape:
  * the call's host wall time (allocation, upload and read-back of loglik included) and the device time of the filter kernel
    from the call's own events;
  * the host twin (the same text, OpenMP on 16 threads) fed the device's model values, and whether it reproduces loglik, the
    increments and the ESS bit for bit;
  * sepaihrd_ensemble_stochastic at S = B, R = J and the same m: the same propagation without the filter, so the ratio of the two
    kernels' device times is what weighting, scanning and resampling cost.
Every timed device call is warmed up once; three repetitions, the median is reported and the repetitions are kept.  The host
twin runs once, and only up to --twin-max-batch parameter vectors (B = 4096 at the largest J is 4 x 10^10 binomial draws).  One
JSON line per shape is appended to profiles/particle_bench.jsonl.

    python tools/bench_particle.py [--batches 256,4096] [--particles 64,max] [--steps 4] [--twin-max-batch 256] [--out FILE]
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
SEED = 20261019
PROBS = [0.5]


def timed(run, reps=REPS):
    run()  # warm-up: code objects, the allocator, the host's thread pool
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = run()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall, out


def thetas(mm, pb, B):
    # B vectors around the base point: 256 distinct jittered draws, repeated (a vector's stream is set by its position)
    distinct = mm.draws.jitter_draws(pb, 11, min(B, 256))
    return np.ascontiguousarray(distinct[np.arange(B) % len(distinct)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096", help="comma-separated B")
    ap.add_argument("--particles", default="64,max", help="comma-separated J; max = sepaihrd_particle_max_particles")
    ap.add_argument("--steps", type=int, default=4, help="steps per output interval")
    ap.add_argument("--twin-max-batch", type=int, default=256, help="largest B the host twin is timed at (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "particle_bench.jsonl"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(THREADS))
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_particle.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    device = torch.cuda.get_device_name(0)
    m = a.steps
    J_max = mm.hostabi.particle_max_particles(pb.n)
    for B in (int(x) for x in a.batches.split(",")):
        for J in (J_max if x == "max" else int(x) for x in a.particles.split(",")):
            theta = thetas(mm, pb, B)
            hip = mm.HipObjective(pb, device=0)
            kernel_ms = []

            def device_run():
                out = hip.particle_loglik(theta, J, m, SEED, want_increments=False, want_ess=False)
                kernel_ms.append(hip.particle_timing().tolist())
                return out

            wall, got = timed(device_run)
            med = np.median(np.array(kernel_ms[1:]), axis=0)
            valid = got["n_valid"]
            steps = (pb.n_times - 1) * m
            row = {"tool": "bench_particle", "problem": "shipped", "n_age": pb.n, "n_times": pb.n_times, "B": B, "J": J, "J_max": J_max,
                   "steps_per_interval": m, "device": device, "seed": SEED, "n_valid": valid,
                   "particle_steps": valid * J * steps, "binomial_draws": valid * J * steps * pb.n * 13,
                   "wall_ms": float(np.median(wall)), "wall_ms_runs": wall, "decode_ms": float(med[0]), "filter_kernel_ms": float(med[1]),
                   "kernel_ms_runs": kernel_ms[1:], "particle_steps_per_s": valid * J * steps / (float(med[1]) * 1e-3),
                   "mean_loglik": float(np.mean(got["loglik"][got["status"] == 0]))}
            # the same propagation without the filter
            phases = []

            def ensemble_run():
                out = hip.ensemble_stochastic(theta, J, m, SEED, PROBS, want_extinct=False)
                phases.append(out["phase_ms"].tolist())
                return out

            ewall, _ = timed(ensemble_run)
            step_ms = float(np.median(np.array(phases[1:]), axis=0)[0])
            row.update({"ensemble_step_kernel_ms": step_ms, "ensemble_wall_ms": float(np.median(ewall)), "ensemble_phase_ms_runs": phases[1:],
                        "filter_over_propagation": float(med[1]) / step_ms})
            if B <= a.twin_max_batch:
                full = hip.particle_loglik(theta, J, m, SEED, want_values=True)
                t0 = time.perf_counter()
                twin = mm.hostabi.particle_from_values(full["model_values"], full["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H,
                                                       pb.obs_ICU, pb.obs_D, J, m, SEED, beta_end_times=pb.beta_end_times, want_final=False)
                twall = (time.perf_counter() - t0) * 1e3
                row.update({"twin_threads": THREADS, "twin_wall_ms": twall, "twin_over_device": twall / float(np.median(wall)),
                            "twin_equals_device": bool(all(np.array_equal(twin[k], full[k], equal_nan=True) for k in ("loglik", "increments", "ess")))})
            print(json.dumps(row))
            with open(a.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
            hip.close()


if __name__ == "__main__":
    main()
