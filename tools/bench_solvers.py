#!/usr/bin/env python3
"""Dopri5 vs Cash-Karp vs Fehlberg 7(8) on one GPU, in the fma build, across tolerances: evaluations per second and the
mean accepted / rejected RK steps per chain.  Where does the order-8 method overtake Dopri5?

Problems (workloads.py): c1 = BASELINE configs[1] (n = 4, 400 days) at 4096 chains, c3 = configs[3]'s share per GPU (the
same problem at 32 768 chains), c5 = configs[4] (n = 16, 1000 days, 32 768 chains).  abs_err = rel_err = each tolerance.
One JSON line per (problem, tolerance, solver), then a summary line per problem with the measured crossover.

usage: tools/bench_solvers.py [--problems c1,c3,c5] [--tols 1e-6,1e-8,1e-10] [--steps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVERS = {"dopri5": 0, "cashkarp": 1, "fehlberg78": 2}
CHAINS = {"c1": 4096, "c3": 32768, "c5": 32768}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="c1,c3,c5")
    ap.add_argument("--tols", default="1e-6,1e-8,1e-10")
    ap.add_argument("--solvers", default="dopri5,cashkarp,fehlberg78")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()

    import torch
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    from mmid_amd import draws, workloads
    dev = torch.device("cuda:0")
    golden = os.path.join(ROOT, "tests", "golden")
    solvers = [s for s in a.solvers.split(",")]
    tols = [float(t) for t in a.tols.split(",")]

    for name in a.problems.split(","):
        base = workloads.build(name, golden, hip_factory=lambda p: mm.HipObjective(p, device=0))
        B = CHAINS[name]
        theta = torch.from_numpy(draws.jitter_draws(base, 1, B)).to(dev)
        d_ll = torch.empty(B, dtype=torch.float64, device=dev)
        d_st = torch.empty(B, dtype=torch.int32, device=dev)
        d_acc = torch.empty(B, dtype=torch.int32, device=dev)
        d_rej = torch.empty(B, dtype=torch.int32, device=dev)
        rate = {}
        for tol in tols:
            for s in solvers:
                pb = base.with_(solver=SOLVERS[s], arith=mm.ARITH_FMA, abs_err=tol, rel_err=tol)
                hip = mm.HipObjective(pb, device=0)
                hip.reserve(B)
                for _ in range(a.warmup):
                    hip.eval_batch_device(theta, d_ll, d_status=d_st, d_n_accept=d_acc, d_n_reject=d_rej)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    hip.eval_batch_device(theta, d_ll, d_status=d_st, d_n_accept=d_acc, d_n_reject=d_rej)
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) * 1e3 / a.steps
                st = d_st.cpu().numpy()
                info = hip.kernel_info(B)
                rate[(tol, s)] = B / ms * 1e3
                print(json.dumps({
                    "problem": name, "chains": B, "n_age": pb.n, "days": pb.n_times, "tol": tol, "solver": s,
                    "ms_per_step": round(ms, 3), "evals_per_s": round(B / ms * 1e3),
                    "mean_accepted": round(float(d_acc.double().mean()), 2),
                    "mean_rejected": round(float(d_rej.double().mean()), 2),
                    "failed_chains": int((st >= 2).sum()), "kernel": info["kernel_name"], "vgprs": info["vgprs"],
                    "scratch_bytes": info["scratch_bytes"]}), flush=True)
                hip.close()
        if "dopri5" in solvers and "fehlberg78" in solvers:
            faster = [t for t in tols if rate[(t, "fehlberg78")] > rate[(t, "dopri5")]]
            print(json.dumps({"problem": name, "summary": "fehlberg78 / dopri5 evals/s",
                              "ratio": {str(t): round(rate[(t, "fehlberg78")] / rate[(t, "dopri5")], 3) for t in tols},
                              "fehlberg78_faster_at": faster}), flush=True)
        del theta


if __name__ == "__main__":
    main()
