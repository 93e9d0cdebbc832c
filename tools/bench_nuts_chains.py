#!/usr/bin/env python3
"""Lock-step No-U-Turn chains (HostObjective.nuts_chains) against the same chains run one after another
(HostObjective.nuts, the path before the lock-step sampler) on one GPU.

Problems: the reference test fixture with two calibrated multipliers (n = 4, 30 output days, P = 7) and its 300-day
tiling -- tools/time_nuts.py's two.  (The shipped 62-parameter problem has run-up output rows: its finite-difference
gradient is degenerate by the reference's own rule and measures nothing.)  Settings: 40 iterations, window 10, depth <= 4,
fma arithmetic, C in {1, 4, 16, 64, 256, 1024}, after a warm-up call of every shape.  Every run ends with its results on
the host (the call's last action is the wait for the last tick's copy), so the host clock brackets drained work.  Three
windows per row; the median and the spread (max - min over median) are reported.

Baseline: C sequential nuts() calls with seeds seed0 + c in the same process, timed for C = 1, 4, 16; for larger C the
per-chain time of the C = 16 baseline is scaled linearly (`baseline_scaled`: true) -- a sequential loop has no other
way to behave.  Reported per row: wall time, ticks, mean rows per tick, gradient rows per second, the ratio to the
baseline, and from a separate run with the contexts' event timers on (events slow the stream a little: not the timed
run) the share of the run spent outside the evaluation kernels -- 1 - max(centre, perturbed kernel time) / wall, the two
contexts' kernels overlapping.  One JSON line per row, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmid_amd_loader  # noqa: E402

KW = dict(iterations=40, adaptation_window=10, max_tree_depth=4)


def problems(mm):
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "reference_test_fixture.json"))
    names = list(pb.param_names) + ["E0_multiplier", "I0_multiplier"]
    sig = dict(pb.sigmas); sig.update(E0_multiplier=0.05, I0_multiplier=0.05)
    bnd = dict(pb.bounds); bnd.update(E0_multiplier=(0.5, 1.2), I0_multiplier=(0.1, 3.0))
    theta = np.concatenate([np.asarray(pb.base_theta), [1.0, 0.8]])
    pb = pb.with_(param_names=names, sigmas=sig, bounds=bnd, base_theta=theta, arith=mm.ARITH_FMA, constraint_mode=1)
    T = 300
    reps = -(-T // len(pb.times))
    tile = lambda a: np.tile(a, (reps, 1))[:T]
    long = pb.with_(times=np.arange(float(T)), obs_H=tile(pb.obs_H), obs_ICU=tile(pb.obs_ICU), obs_D=tile(pb.obs_D))
    return {"fixture_30d": pb, "fixture_300d": long}


def windows(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        t.append(time.perf_counter() - t0)
    t = np.array(t)
    return r, float(np.median(t)), float((t.max() - t.min()) / np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 4, 16, 64, 256, 1024])
    ap.add_argument("--baseline-chains", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--problems", nargs="+", default=["fixture_30d", "fixture_300d"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nuts_chains_bench.jsonl"))
    args = ap.parse_args()
    mm = mmid_amd_loader.load()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_nuts_chains.py needs a GPU: nothing is measured without one")
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for name, pb in problems(mm).items():
        if name not in args.problems:
            continue
        host = mm.HostObjective(pb)
        base = np.asarray(pb.base_theta)
        rng = np.random.default_rng(1)
        starts = base * (1.0 + 0.01 * rng.standard_normal((max(args.chains), base.size)))
        host.nuts(starts[0], 3, iterations=3, adaptation_window=2, max_tree_depth=2)  # warm-up of the solo path
        per_chain = {}
        for C in args.baseline_chains:
            def solo():
                return [host.nuts(starts[c], 3 + c, **KW) for c in range(C)]
            r, med, spread = windows(solo, args.reps)
            per_chain[C] = med / C
            emit({"problem": name, "path": "sequential", "chains": C, "seconds": med, "spread": spread,
                  "gradient_launches": int(sum(x["gradient_launches"] for x in r)),
                  "gradients_per_second": sum(x["gradient_launches"] for x in r) / med})
        for C in args.chains:
            host.nuts_chains(starts[:C], 3, iterations=3, adaptation_window=2, max_tree_depth=2)  # warm-up of this batch size
            r, med, spread = windows(lambda: host.nuts_chains(starts[:C], 3, **KW), args.reps)
            timed = host.nuts_chains(starts[:C], 3, kernel_timing=True, **KW)
            kernel_s = 1e-3 * max(timed["centre_kernel_ms"], timed["perturbed_kernel_ms"])
            scaled = C not in per_chain
            baseline = (per_chain[C] if not scaled else per_chain[max(per_chain)]) * C if per_chain else None
            grads = int(np.sum(r["rows_evaluated"]))  # rows of all ticks (value-only rows included: one per iteration and chain at most)
            emit({"problem": name, "path": "lock_step", "chains": C, "seconds": med, "spread": spread, "ticks": r["ticks"],
                  "mean_rows_per_tick": r["mean_rows_per_tick"], "seconds_per_tick": med / r["ticks"],
                  "gradients_per_second": grads / med, "baseline_seconds": baseline, "baseline_scaled": scaled,
                  "speedup_vs_sequential": None if baseline is None else baseline / med,
                  "share_outside_kernels": 1.0 - kernel_s / timed["seconds"], "share_outside_evaluation_call":
                  1.0 - timed["evaluation_seconds"] / timed["seconds"], "failed_chains": int(np.sum(r["failure_status"] != 0))})
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
