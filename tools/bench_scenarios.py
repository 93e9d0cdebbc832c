#!/usr/bin/env python3
"""NPI scenario analysis (sepaihrd_scenario_ensemble) against its sequential form on one GPU: one K = 3 launch (baseline,
stricter and weaker lockdown over every sample) against three sepaihrd_ensemble_quantiles calls with the metric table,
one per scenario (the kappa scaling done there by rewriting theta, which is what a caller without the new entry point
would do -- close to, not exactly, the same numbers).  Host-pointer entry points, uploads and downloads
included.  One JSON line per (workload, samples)."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmid_amd_loader  # noqa: E402

PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]


def timed(fn, reps):
    fn()  # warm: buffers, code objects
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    return (time.perf_counter() - t0) / reps * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["c1", "c5"])
    ap.add_argument("--samples", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mm = mmid_amd_loader.load()
    lines = []
    for wl in args.workloads:
        pb = mm.workloads.build(wl, os.path.join(ROOT, "tests", "golden"), hip_factory=lambda q: mm.HipObjective(q)).with_(arith=mm.ARITH_FMA)
        nk = len(pb.kappa_values)
        scen = mm.config_io.default_lockdown_scenarios(nk)
        table = np.array([m for _, m in scen])
        kappa_cols = [p for p, nm in enumerate(pb.param_names) if nm == "kappa_2"]
        for S in args.samples:
            theta = mm.draws.jitter_draws(pb, 1, S)
            rec = {"workload": wl, "n_age": pb.n, "n_times": pb.n_times, "samples": S, "scenarios": len(scen)}
            try:
                hip = mm.HipObjective(pb)
                hip.set_initial_state_mode(1)
                thetas = []
                for _, m in scen:
                    t = theta.copy()
                    for p in kappa_cols:
                        t[:, p] *= m[1]
                    thetas.append(t)
                rec["three_ensemble_calls_ms"], _ = timed(
                    lambda: [hip.ensemble_quantiles(t, PROBS, want_sero=True, want_rt=True, want_metrics=True) for t in thetas], args.reps)
                del hip
                gc.collect()
                hip = mm.HipObjective(pb)
                hip.set_initial_state_mode(1)
                rec["one_scenario_launch_ms"], r = timed(lambda: hip.scenario_ensemble(theta, table, PROBS, want_sero=True, want_rt=True),
                                                         args.reps)
                rec["speedup"] = rec["three_ensemble_calls_ms"] / rec["one_scenario_launch_ms"]
                rec["n_valid"] = [int(v) for v in r["n_valid"]]
                rec["median_deaths_difference"] = [float(r["diff"][k, 7, 2]) for k in range(len(scen))]
                del hip
                gc.collect()
            except RuntimeError as e:  # e.g. a device allocation beyond HBM: reported, not retried
                rec["error"] = str(e)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
