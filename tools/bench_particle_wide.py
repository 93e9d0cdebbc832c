#!/usr/bin/env python3
"""The wide form of the particle filter (sepaihrd_particle_loglik_wide) on the GPU: how noisy the log-likelihood estimate is at the
particle counts it opens up, and what a call costs (diagnostic; not part of bench.py, run by no test).

Runs on the GPU only, one process, one box.  The shipped problem (n = 4, 326 output times, x(t0) seeded from theta) with m = 4
steps per output interval.  Two parts, each appending JSON lines to profiles/particle_wide_bench.jsonl:

  sd      the standard deviation of loglik at the base theta over 32 seeds: at J = sepaihrd_particle_max_particles(4) = 136 through
          the LDS kernel, at J = 1024 and 8192 through the wide call.  Particle-marginal Metropolis-Hastings mixes when this is of
          order 1.
  timing  at B = 16 and 256 with J = 1024 and 8192: the call's host wall time and sepaihrd_particle_wide_timing (decode; all filter
          launches), particle-steps per second of the filter launches, and the host twin (the same text, OpenMP on 16 threads) fed
          the device's model values, with whether it reproduces loglik, the increments and the ESS bit for bit -- the twin only up
          to --twin-max-particles B x J.  The reference point is the LDS kernel at B = 4096, J = 136 on the same box: a comparable
          total particle count through the kernel this form leaves unchanged.
Every timed device call is warmed up once; --reps repetitions, the median is reported and the repetitions are kept.

The split between propagation and resampling is not taken here: run the tool once under `rocprofv3 --kernel-trace --stats --`
(no counters) and read wide_propagate_kernel against wide_resample_kernel.

    python tools/bench_particle_wide.py [--parts sd,timing] [--batches 16,256] [--particles 1024,8192] [--steps 4] [--reps 3]
                                        [--twin-max-particles 131072] [--out FILE]
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
SEED = 20261020
SD_SEEDS = 32
REFERENCE_B = 4096


def timed(run, reps):
    run()  # warm-up: code objects, the allocator
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


def spread(mm, pb, hip, m, J, wide):
    ll = []
    for k in range(SD_SEEDS):
        call = hip.particle_loglik_wide if wide else hip.particle_loglik
        got = call(pb.base_theta, J, m, SEED + k, want_increments=False, want_ess=k == 0)
        assert got["status"][0] == 0
        ll.append(float(got["loglik"][0]))
        if k == 0:
            ess = got["ess"][0]
    ll = np.array(ll)
    return {"part": "sd", "J": J, "form": "wide" if wide else "lds", "seeds": SD_SEEDS, "loglik_mean": float(ll.mean()),
            "loglik_sd": float(ll.std(ddof=1)), "loglik_min": float(ll.min()), "loglik_max": float(ll.max()),
            "weighted_rows": int(np.isfinite(ess).sum()), "mean_ess_first_seed": float(np.nanmean(ess)), "loglik": ll.tolist()}


def timing(mm, pb, hip, m, B, J, wide, reps, twin_max):
    theta = thetas(mm, pb, B)
    device_ms = []

    def device_run():
        if wide:
            out = hip.particle_loglik_wide(theta, J, m, SEED, want_increments=False, want_ess=False)
            device_ms.append(hip.particle_wide_timing().tolist())
        else:
            out = hip.particle_loglik(theta, J, m, SEED, want_increments=False, want_ess=False)
            device_ms.append(hip.particle_timing().tolist())
        return out

    wall, got = timed(device_run, reps)
    med = np.median(np.array(device_ms[1:]), axis=0)
    valid = got["n_valid"]
    steps = (pb.n_times - 1) * m
    row = {"part": "timing", "form": "wide" if wide else "lds", "B": B, "J": J, "n_valid": valid, "particle_steps": valid * J * steps,
           "wall_ms": float(np.median(wall)), "wall_ms_runs": wall, "decode_ms": float(med[0]), "filter_ms": float(med[1]),
           "device_ms_runs": device_ms[1:], "particle_steps_per_s": valid * J * steps / (float(med[1]) * 1e-3),
           "mean_loglik": float(np.mean(got["loglik"][got["status"] == 0]))}
    if wide and B * J <= twin_max:
        full = hip.particle_loglik_wide(theta, J, m, SEED, want_values=True)
        t0 = time.perf_counter()
        twin = mm.hostabi.particle_wide_from_values(full["model_values"], full["status"], pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H,
                                                    pb.obs_ICU, pb.obs_D, J, m, SEED, beta_end_times=pb.beta_end_times, want_final=False)
        twall = (time.perf_counter() - t0) * 1e3
        row.update({"twin_threads": THREADS, "twin_wall_ms": twall, "twin_over_device": twall / float(np.median(wall)),
                    "twin_equals_device": bool(all(np.array_equal(twin[k], full[k], equal_nan=True) for k in ("loglik", "increments", "ess")))})
    elif wide:
        row["twin_wall_ms"] = "not measured"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="sd,timing")
    ap.add_argument("--batches", default="16,256", help="comma-separated B of the timing part")
    ap.add_argument("--particles", default="1024,8192", help="comma-separated J of the wide call, both parts")
    ap.add_argument("--steps", type=int, default=4, help="steps per output interval")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--twin-max-particles", type=int, default=131072, help="largest B x J the host twin is timed at (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "particle_wide_bench.jsonl"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(THREADS))
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_particle_wide.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = {"tool": "bench_particle_wide", "problem": "shipped", "n_age": pb.n, "n_times": pb.n_times, "steps_per_interval": a.steps,
            "device": torch.cuda.get_device_name(0), "seed": SEED}
    J_lds = mm.hostabi.particle_max_particles(pb.n)
    particles = [int(x) for x in a.particles.split(",")]
    hip = mm.HipObjective(pb, device=0)
    rows = []

    def emit(row):
        row = {**head, **row}
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k not in ("loglik", "wall_ms_runs", "device_ms_runs")}), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    parts = a.parts.split(",")
    if "sd" in parts:
        emit(spread(mm, pb, hip, a.steps, J_lds, wide=False))
        for J in particles:
            emit(spread(mm, pb, hip, a.steps, J, wide=True))
    if "timing" in parts:
        ref = timing(mm, pb, hip, a.steps, REFERENCE_B, J_lds, False, a.reps, 0)
        emit(ref)
        for B in (int(x) for x in a.batches.split(",")):
            for J in particles:
                row = timing(mm, pb, hip, a.steps, B, J, True, a.reps, a.twin_max_particles)
                row["particle_steps_per_s_over_lds_reference"] = row["particle_steps_per_s"] / ref["particle_steps_per_s"]
                emit(row)
    hip.close()


if __name__ == "__main__":
    main()
