#!/usr/bin/env python3
"""Time of the SIR scenario ensemble (sepaihrd_sir_scenario_ensemble) on the GPU (diagnostic; not part of bench.py).

Runs on the GPU only, one process, one box.  For tools/bench_sir.py's two problems (BASELINE configs[0]'s three ages and the
sixteen-age synthetic problem, 201 output times), Dopri5, K = 3 scenarios (baseline, contact 0.7 at day 20, the compound
schedule of tests/test_gpu_sir_ensemble.py) at S = 4096 and S = 32 768 samples:
  new  the call itself: host wall time (uploads and read-back of the results included) and the device time of its three
       phases from the context's event timers (sepaihrd_sir_ensemble_timing): integrator (K x S chains, the observer's
       stores included), fix-up + metric passes, sorts + quantiles + scenario summaries;
  (a)  the bare likelihood launch sepaihrd_sir_eval_batch_device on the same K x S chains (theta resident, no events, no
       stores; device events around the launches) -- new.integrator_ms minus this is what the cursor and the observer's
       stores cost.  The shipped kernels are compiled from the same tokens as before the ensemble build existed, so this is
       the previous commit's launch;
  (b)  what a user did before: sepaihrd_sir_eval_batch with trajectories for the S samples of ONE scenario (the baseline: the
       others could not be run at all), then the three series and np.quantile over the samples on 16 threads (host wall time).
Every timed shape is warmed up once; three repetitions, the median is reported and the repetitions are kept.
One JSON line per (problem, S) is appended to profiles/sir_ensemble_bench.jsonl.

    python tools/bench_sir_ensemble.py [--arith fma|strict] [--samples 4096,32768] [--skip-host-baseline]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
SCENARIOS = [[], [(20, "contact", 0.7)], [(30, "transmission", 0.3), (45, "contact", 0.5), (90, "contact", 1.6)]]
THREADS = 16


def host_baseline(mm, hip, pb, theta):
    """eval_batch with trajectories, the three series with their age totals, np.quantile per block of output times"""
    t0 = time.perf_counter()
    traj = hip.eval_batch(theta, want_traj=True)["traj"]
    t1 = time.perf_counter()
    n = pb.n
    v = pb.model_values(theta[0])

    def block(ts):
        rows = traj[:, ts]
        ion = rows[:, :, n:2 * n] / pb.N
        inc = np.maximum(v["q"] * (ion @ (pb.C * v["scale_C_total"]).T), 0.0) * rows[:, :, :n]  # one sample's parameters: timing only
        out = []
        for a in (inc, rows[:, :, n:2 * n], pb.initial_state[:n] - rows[:, :, :n]):
            a = np.concatenate([a, a.sum(axis=-1, keepdims=True)], axis=-1)
            out.append(np.quantile(a, PROBS, axis=0, method="linear"))
        return out

    chunks = np.array_split(np.arange(pb.n_times), THREADS * 2)
    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(block, chunks))
    t2 = time.perf_counter()
    return {"eval_batch_traj_ms": (t1 - t0) * 1e3, "numpy_quantiles_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}


def padded_samples(S):
    """S_pad of the call: a power of two >= 64 up to 16 384 samples (LDS sort), beyond that a multiple of 64"""
    if S <= 16384:
        return max(64, 1 << (S - 1).bit_length())
    return (S + 63) // 64 * 64


def bare_launch(torch, hip, theta, reps=3):
    B = len(theta)
    d_theta = torch.tensor(theta, dtype=torch.float64, device="cuda")
    d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
    d_st = torch.empty(B, dtype=torch.int32, device="cuda")
    hip.eval_batch_device(d_theta, d_ll, d_st)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.eval_batch_device(d_theta, d_ll, d_st)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="fma", choices=["fma", "strict"])
    ap.add_argument("--samples", default="4096,32768")
    ap.add_argument("--skip-host-baseline", action="store_true")
    a = ap.parse_args()
    import oracle_py
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    from bench_sir import sixteen_age_problem
    import torch
    assert torch.cuda.is_available(), "bench_sir_ensemble.py needs a GPU"
    arith = mm.ARITH_FMA if a.arith == "fma" else mm.ARITH_STRICT
    problems = {"config0_n3": mm.workloads.sir_config0(oracle_py.sir_simulate), "synthetic_n16": sixteen_age_problem(mm, oracle_py)}
    out_path = os.path.join(ROOT, "profiles", "sir_ensemble_bench.jsonl")
    K = len(SCENARIOS)
    for name, pb0 in problems.items():
        pb = pb0.with_(solver=mm.SOLVER_DOPRI5, arith=arith)
        for S in [int(x) for x in a.samples.split(",")]:
            rng = np.random.default_rng(1)
            theta = pb.current_parameters() * np.exp(rng.normal(0.0, 0.1, size=(S, pb.n_params)))
            hip = mm.HipSIRObjective(pb)
            hip.scenario_ensemble(theta, SCENARIOS, PROBS)  # warm-up: code objects, scratch of the context
            wall, phases = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                got = hip.scenario_ensemble(theta, SCENARIOS, PROBS)
                wall.append((time.perf_counter() - t0) * 1e3)
                t = hip.ensemble_timing()
                phases.append([t["integrator_ms"], t["metrics_ms"], t["sort_ms"]])
            med = np.median(np.array(phases), axis=0)
            bare = bare_launch(torch, hip, np.tile(theta, (K, 1)))
            row = {"tool": "bench_sir_ensemble", "problem": name, "n_age": pb.n, "n_times": pb.n_times, "K": K, "S": S, "chains": K * S,
                   "arith": a.arith, "solver": "dopri5", "device": torch.cuda.get_device_name(0),
                   "n_valid": [int(x) for x in got["n_valid"]],
                   "new_wall_ms": float(np.median(wall)), "new_wall_ms_runs": wall,
                   "new_device_ms": float(med.sum()), "new_integrator_ms": float(med[0]), "new_metrics_ms": float(med[1]),
                   "new_sort_ms": float(med[2]), "new_phase_ms_runs": phases,
                   "a_bare_eval_launch_ms": float(np.median(bare)), "a_bare_eval_launch_ms_runs": bare,
                   "integrator_over_bare": float(med[0] / np.median(bare)),
                   "a_is_the_parent_launch_because": "the shipped kernels are compiled from the tokens they were compiled from before the "
                                                     "ensemble build existed (every addition is under SEPAIHRD_SIR_ENSEMBLE); "
                                                     "tests/test_sir_ensemble_cpu.py holds their register figures to the parent's",
                   "series_bytes": K * 3 * pb.n_times * (pb.n + 1) * 8 * padded_samples(S)}
            if not a.skip_host_baseline:
                host_baseline(mm, hip, pb, theta[:256])  # warm-up of the staging path and of numpy's threads
                b = host_baseline(mm, hip, pb, theta)
                row.update({"b_one_scenario_host_ms": b["total_ms"], "b_eval_batch_traj_ms": b["eval_batch_traj_ms"],
                            "b_numpy_quantiles_ms": b["numpy_quantiles_ms"], "b_threads": THREADS,
                            "b_traj_bytes": int(S * pb.n_times * 3 * pb.n * 8),
                            "b_one_scenario_over_new_three": b["total_ms"] / float(np.median(wall))})
            hip.close()
            print(json.dumps(row))
            with open(out_path, "a") as fh:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
