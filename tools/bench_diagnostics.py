#!/usr/bin/env python3
"""Convergence diagnostics of many chains (sepaihrd_chain_diagnostics, sepaihrd_mh_diagnostics) on one GPU, against the
numpy restatement (mmid_amd.diagnostics, 16 threads).  AR(1) draws x_t = phi x_{t-1} + e_t, P = 62 parameters plus the
values column, N = 1000 draws per chain.  Per (phi, C): the host-pointer call with its upload timed separately (the upload
alone: one host-to-device copy of the same bytes), the largest Geyer lag reached, and the numpy time where asked.  Then the
resident path: sepaihrd_mh_diagnostics after a short device-resident sampler run of C chains (N = 1000 stored samples).
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmid_amd_loader  # noqa: E402


def ar1(rng, C, N, P, phi):
    x = np.empty((C, N, P))
    x[:, 0] = rng.standard_normal((C, P)) / np.sqrt(1 - phi * phi)
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + rng.standard_normal((C, P))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[256, 4096, 16384])
    ap.add_argument("--phis", type=float, nargs="+", default=[0.0, 0.9, 0.99])
    ap.add_argument("--numpy-chains", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--resident-chains", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mm = mmid_amd_loader.load()
    import torch
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    hip = mm.HipObjective(pb)
    N, P = 1000, 62
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for phi in args.phis:
        for C in args.chains:
            if phi == 0.99 and C > 4096:
                continue  # the worst case at the two smaller sizes is enough
            rng = np.random.default_rng(int(1000 * phi) + C)
            s = ar1(rng, C, N, P + 1, phi)
            samples, values = np.ascontiguousarray(s[:, :, :P]), np.ascontiguousarray(s[:, :, P])
            hip.chain_diagnostics(samples, values)  # warm
            t0 = time.perf_counter()
            for _ in range(args.reps):
                r = hip.chain_diagnostics(samples, values)
            total = (time.perf_counter() - t0) / args.reps * 1e3
            both = np.concatenate([samples.ravel(), values.ravel()])
            torch.from_numpy(both).to("cuda:0")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                torch.from_numpy(both).to("cuda:0")
                torch.cuda.synchronize()
            upload = (time.perf_counter() - t0) / args.reps * 1e3
            rec = {"path": "chain_diagnostics", "phi": phi, "chains": C, "draws": N, "columns": P + 1, "call_ms": total,
                   "upload_ms": upload, "device_ms": total - upload, "max_geyer_lag": int(r["max_lag"].max()),
                   "median_ess_bulk": float(np.median(r["table"][:, 4])), "max_r_hat": float(np.max(r["table"][:, 6]))}
            if C in args.numpy_chains:
                t0 = time.perf_counter()
                ref = mm.diagnostics.chain_diagnostics(samples, values, threads=16)
                rec["numpy_ms"] = (time.perf_counter() - t0) * 1e3
                ok = ~np.isnan(ref["table"])
                rec["max_rel_diff_vs_numpy"] = float(np.max(np.abs(r["table"][ok] - ref["table"][ok]) / np.abs(ref["table"][ok])))
                rec["max_lag_equal"] = bool(np.array_equal(r["max_lag"], ref["max_lag"]))
            emit(rec)
    del hip

    for C in args.resident_chains:
        pbr = pb.with_(arith=mm.ARITH_FMA, constraint_mode=1)
        x0 = np.tile(pbr.base_theta, (C, 1))
        host = mm.HostObjective(pbr)
        host.set_mh_diagnostics(True)
        t0 = time.perf_counter()
        run = host.metropolis_hastings(x0, seed=5, iterations=2000, burn_in=0, adaptation_period=100, thinning=2,
                                       device_state=True, want_trace=False)
        wall = time.perf_counter() - t0
        table = host.mh_diagnostics()
        emit({"path": "mh_diagnostics (resident)", "chains": C, "draws": int(run["samples"].shape[1] - 1), "columns": int(table.shape[0]),
              "device_ms": float(host.lib.host_last_mh_diagnostics_seconds()) * 1e3, "sampler_run_s": wall,
              "sampler_loop_s": run["loop_seconds"], "max_r_hat": float(np.nanmax(table[:, 6])),
              "min_ess_bulk": float(np.nanmin(table[:, 4]))})
        del host
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
