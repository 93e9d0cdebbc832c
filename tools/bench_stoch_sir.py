#!/usr/bin/env python3
"""Time of the stochastic SIR ensembles (sepaihrd_stoch_sir_run) on the GPU (diagnostic; not part of bench.py).

Runs on the GPU only, one process, one box.  Shapes:
  * the reference driver's workload (tests/golden/stochastic_sir_reference_input.json: N = 1000, h = 1/24, 8641 rows) at 100
    (what the reference runs), 4096 and 65 536 replicates;
  * a sweep of 64 groups, beta from 0.1 to 1.0, 4096 replicates each, same grid.
Per shape: the call's host wall time (allocation, uploads and read-back of the statistics included), the device time of its
phases from the call's own events -- step kernels; segment sorts; summaries (up to 16 384 replicates sort and summary are one
kernel, counted under the sorts) -- and the host twin (the same model text, OpenMP on 16 threads, std::sort) on the same shape.
Every timed shape is warmed up once; three repetitions (two of the host twin), the median is reported and the repetitions
are kept.  The rate is
replicate-steps per second of wall time: groups x replicates x (rows - 1) / wall.
One JSON line per shape is appended to profiles/stoch_sir_bench.jsonl.

    python tools/bench_stoch_sir.py [--replicates 100,4096,65536] [--sweep-replicates 4096] [--skip-host-twin]
                                    [--max-workspace-bytes N] [--out FILE]
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
SEED = 20240611


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
    ap.add_argument("--replicates", default="100,4096,65536")
    ap.add_argument("--sweep-replicates", type=int, default=4096)
    ap.add_argument("--skip-host-twin", action="store_true")
    ap.add_argument("--max-workspace-bytes", type=int, default=0, help="0: the library's default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoch_sir_bench.jsonl"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(THREADS))
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_stoch_sir.py needs a GPU"
    ref, _ = mm.workloads.stochastic_sir_reference()
    shapes = [("reference", ref, int(r)) for r in a.replicates.split(",") if r]
    if a.sweep_replicates > 0:
        shapes.append(("beta_sweep_64", ref.with_(beta=np.linspace(0.1, 1.0, 64)), a.sweep_replicates))
    out_path = a.out
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    for name, pb, R in shapes:
        hip = mm.HipStochasticSIR(pb, device=0)
        phases = []

        def device_run():
            out = hip.run(R, seed=SEED, max_workspace_bytes=a.max_workspace_bytes)
            phases.append([hip.phase_ms["step"], hip.phase_ms["sort"], hip.phase_ms["summary"]])
            return out

        wall, got = timed(device_run)
        steps = got["stats"].shape[-1]
        work = pb.n_groups * R * (steps - 1)
        med = np.median(np.array(phases[1:]), axis=0)
        row = {"tool": "bench_stoch_sir", "shape": name, "groups": pb.n_groups, "replicates": R, "rows": steps, "replicate_steps": work,
               "device": torch.cuda.get_device_name(0), "seed": SEED,
               "max_workspace_bytes": a.max_workspace_bytes or mm.hipabi.STOCH_SIR_DEFAULT_WORKSPACE,
               "wall_ms": float(np.median(wall)), "wall_ms_runs": wall,
               "step_ms": float(med[0]), "sort_ms": float(med[1]), "summary_ms": float(med[2]), "phase_ms_runs": phases[1:],
               "replicate_steps_per_s": work / (float(np.median(wall)) * 1e-3),
               "replicate_steps_per_s_step_kernel_only": work / (float(med[0]) * 1e-3),
               "mean_final_S_group0": float(got["stats"][0, 0, 0, -1])}
        if not a.skip_host_twin:
            twin = mm.HostStochasticSIR(pb)
            twall, tgot = timed(lambda: twin.run(R, seed=SEED), reps=2)
            row.update({"twin_threads": THREADS, "twin_wall_ms": float(np.median(twall)), "twin_wall_ms_runs": twall,
                        "twin_over_device": float(np.median(twall) / np.median(wall)),
                        "twin_equals_device": bool(np.array_equal(tgot["stats"], got["stats"]))})
        print(json.dumps(row))
        with open(out_path, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
