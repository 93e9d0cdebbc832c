#!/usr/bin/env python3
"""Evaluations/s of the age-structured SIR likelihood kernel (diagnostic; not part of bench.py).

Runs on the GPU only (no fallback).  For BASELINE configs[0]'s three-age problem and a sixteen-age synthetic problem, at
4096 and 65 536 chains: device-resident theta, warm-up launches, then a window of launches between two device events
(device time of launch + kernel, no host copies).  Next to it the CPU oracle's Dopri5 run (oracle_py.sir_simulate,
trajectory only -- the likelihood terms are not included, which flatters the CPU) on 16 processes.
One JSON line per run is appended to profiles/sir_bench.jsonl.

    python tools/bench_sir.py [--arith fma|strict] [--solver dopri5|cash_karp|fehlberg78] [--min-seconds 0.5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def sixteen_age_problem(mm, oracle_py):
    rng = np.random.default_rng(16)
    n = 16
    N = rng.uniform(2e5, 1.5e6, n)
    Cm = rng.uniform(0.2, 1.0, (n, n)) * 12.0 / n
    gamma = rng.uniform(0.15, 0.25, n)
    I0 = np.round(rng.uniform(5, 25, n))
    init = np.concatenate([N - I0, I0, np.zeros(n)])
    times = np.arange(0.0, 201.0)
    names = ["q", "scale_C_total"] + [f"gamma_{i}" for i in range(n)]
    pb = mm.SIRProblem(N=N, C=Cm, gamma=gamma, q=0.03, scale_C_total=1.0, initial_state=init, times=times,
                       obs=np.zeros((len(times), n)), param_names=names)
    traj = oracle_py.sir_simulate(N, Cm, gamma, 0.03, 1.0, init, times)["traj"]
    return pb.with_(obs=rng.poisson(mm.workloads.sir_incidence(pb, traj)).astype(np.float64))


def _cpu_worker(args):
    import oracle_py
    pbd, thetas = args
    for th in thetas:
        q, scale, gamma = th[0], th[1], th[2:]
        oracle_py.sir_simulate(pbd["N"], pbd["C"], gamma, q, scale, pbd["init"], pbd["times"])
    return len(thetas)


def cpu_rate(pb, theta, procs=16, per_proc=2048):
    import multiprocessing as mp
    pbd = {"N": pb.N, "C": pb.C, "init": pb.initial_state, "times": pb.times}
    chunks = [(pbd, theta[(i * per_proc) % len(theta):][:per_proc]) for i in range(procs)]
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_cpu_worker, [(pbd, theta[:2])] * procs)  # warm the workers
        t0 = time.perf_counter()
        done = sum(pool.map(_cpu_worker, chunks))
        dt = time.perf_counter() - t0
    return done / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="fma", choices=["fma", "strict"])
    ap.add_argument("--solver", default="dopri5", choices=["dopri5", "cash_karp", "fehlberg78"])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    import oracle_py
    rates_cpu = {}
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    problems = {"config0_n3": mm.workloads.sir_config0(oracle_py.sir_simulate), "synthetic_n16": sixteen_age_problem(mm, oracle_py)}
    draws = {}
    for name, pb in problems.items():
        rng = np.random.default_rng(1)
        draws[name] = pb.current_parameters() * np.exp(rng.normal(0.0, 0.3, size=(65536, pb.n_params)))
        rates_cpu[name] = cpu_rate(pb, draws[name])  # before the GPU is opened: the workers are forked
    import torch
    assert torch.cuda.is_available(), "bench_sir.py needs a GPU"
    solver = {"dopri5": mm.SOLVER_DOPRI5, "cash_karp": mm.SOLVER_CASH_KARP54, "fehlberg78": mm.SOLVER_FEHLBERG78}[a.solver]
    arith = mm.ARITH_FMA if a.arith == "fma" else mm.ARITH_STRICT
    out_path = os.path.join(ROOT, "profiles", "sir_bench.jsonl")
    for name, pb in problems.items():
        hip = mm.HipSIRObjective(pb.with_(solver=solver, arith=arith))
        for B in (4096, 65536):
            d_theta = torch.tensor(draws[name][:B], dtype=torch.float64, device="cuda")
            d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
            d_st = torch.empty(B, dtype=torch.int32, device="cuda")
            d_na = torch.empty(B, dtype=torch.int32, device="cuda")
            for _ in range(5):
                hip.eval_batch_device(d_theta, d_ll, d_st, d_na)
            torch.cuda.synchronize()
            reps, windows = 4, []
            while True:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    hip.eval_batch_device(d_theta, d_ll, d_st, d_na)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
                if ms / 1e3 >= a.min_seconds:
                    windows.append(ms / reps)
                    if len(windows) == 3:
                        break
                else:
                    reps *= 2
            ms = float(np.median(windows))
            rec = {"tool": "bench_sir", "problem": name, "n_age": pb.n, "n_times": pb.n_times, "n_params": pb.n_params, "chains": B,
                   "solver": a.solver, "arith": a.arith, "ms_per_launch": ms, "ms_windows": windows, "launches_per_window": reps,
                   "evals_per_s": B / (ms / 1e3), "status_ok": int((d_st == 0).sum().item()),
                   "accepted_steps_mean": float(d_na.double().mean().item()),
                   "cpu_oracle_dopri5_16_procs_runs_per_s": rates_cpu[name], "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec))
            with open(out_path, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        hip.close()


if __name__ == "__main__":
    main()
