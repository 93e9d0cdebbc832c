#!/usr/bin/env python3
"""The filtered state means and quantile bands of the particle filter (sepaihrd_particle_filter_states): what the per-row
summaries cost over the wide call they ride on, and where the simulated cloud leaves the data (diagnostic; not part of bench.py,
run by no test).  DESIGN.md section 6n.

The shipped problem (n = 4, 326 output times, x(t0) seeded from theta) with m = 4 steps per output interval, B = 16 vectors
around the base theta (the first of them the base theta itself), J = 1024 and 8192, probabilities (0.025, 0.5, 0.975), under
k = +inf (Poisson) and k = 1 for the three series.

  timing   the new call and particle_loglik_wide (with the same dispersion) on the same inputs, interleaved in one process: wall time
           and device time per call, medians of --reps after one warm-up round; the new call's device time split into the filter's
           launches and the summaries' launches.
  rows     for the base theta: the ten weighted rows of lowest ESS with the observed H, ICU and D totals and the 95 % bands of the
           filtered totals of H, ICU and D (the compartments the observed increments flow into), and the count of rows whose ESS is
           below J / 100.

Appends to profiles/particle_states_bench.jsonl.

    python tools/bench_particle_states.py [--particles 1024,8192] [--steps 4] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261020   # tools/bench_particle_wide.py's
INF = float("inf")
B = 16
PROBS = (0.025, 0.5, 0.975)
H_, ICU_, D_ = 5, 6, 8


def timing(mm, hip, theta, m, J, k, reps):
    disp = None if k == INF else (k, k, k)
    wall, dev = {"states": [], "wide": []}, {"states": [], "wide": []}
    split, got, ref = [], None, None
    for rep in range(reps + 1):   # the first round warms up
        t0 = time.perf_counter()
        got = hip.particle_filter_states(theta, J, m, SEED, PROBS, dispersion=disp)
        w = (time.perf_counter() - t0) * 1e3
        ms = hip.particle_states_timing()
        t0 = time.perf_counter()
        ref = hip.particle_loglik_wide(theta, J, m, SEED, dispersion=disp)
        w_ref = (time.perf_counter() - t0) * 1e3
        if rep > 0:
            wall["states"].append(w)
            wall["wide"].append(w_ref)
            dev["states"].append(float(ms[1]))
            dev["wide"].append(float(hip.particle_wide_timing()[1]))
            split.append([float(ms[1] - ms[2]), float(ms[2])])   # B = 16 is one chunk: ms[2] is every summary
    same = all(np.array_equal(got[key], ref[key], equal_nan=True) for key in ("loglik", "increments", "ess"))
    row = {"part": "timing", "B": len(theta), "J": J, "k": "inf" if k == INF else k, "reps": reps, "filter_outputs_equal_the_wide_call": bool(same)}
    for f in ("states", "wide"):
        row[f + "_wall_ms"] = float(np.median(wall[f]))
        row[f + "_device_ms"] = float(np.median(dev[f]))
        row[f + "_device_ms_runs"] = dev[f]
    row["states_filter_ms"], row["states_summary_ms"] = (float(v) for v in np.median(np.array(split), axis=0))
    row["states_over_wide_device"] = row["states_device_ms"] / row["wide_device_ms"]
    row["states_over_wide_wall"] = row["states_wall_ms"] / row["wide_wall_ms"]
    return row, got


def lowest_ess_rows(pb, got, J, k):
    """the base theta (position 0): the ten weighted rows of lowest ESS with their observed totals and filtered bands"""
    n, runup = pb.n, int(np.sum(np.asarray(pb.times) < 0.0))
    ess = got["ess"][0]
    order = [int(t) for t in np.argsort(np.where(np.isfinite(ess), ess, np.inf))[:10] if np.isfinite(ess[t])]
    rows = []
    for t in order:
        row = {"t": t, "time": float(pb.times[runup + t]), "ess": float(ess[t]), "increment": float(got["increments"][0, t])}
        for name, obs, c in (("H", pb.obs_H, H_), ("ICU", pb.obs_ICU, ICU_), ("D", pb.obs_D, D_)):
            cell = np.asarray(obs)[t] if t < len(obs) else np.full(n, np.nan)
            usable = np.isfinite(cell) & (cell >= 0)
            row["obs_" + name] = float(cell[usable].sum()) if usable.any() else None
            row["band_" + name] = [float(v) for v in got["state_quantiles"][0, runup + t, c, n]]
            row["mean_" + name] = float(got["state_mean"][0, runup + t, c, n])
        rows.append(row)
    finite = ess[np.isfinite(ess)]
    return {"part": "rows", "J": J, "k": "inf" if k == INF else k, "weighted_rows": int(finite.size), "rows_with_ess_below_J_over_100": int((finite < J / 100.0).sum()),
            "median_ess": float(np.median(finite)), "loglik": float(got["loglik"][0]), "lowest_ess_rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1024,8192", help="comma-separated J")
    ap.add_argument("--steps", type=int, default=4, help="steps per output interval")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    import torch
    assert torch.cuda.is_available(), "bench_particle_states.py needs a GPU"
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    out = a.out or os.path.join(ROOT, "profiles", "particle_states_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    head = {"tool": "bench_particle_states", "problem": "shipped", "n_age": pb.n, "n_times": pb.n_times, "steps_per_interval": a.steps, "seed": SEED,
            "probs": list(PROBS), "device": torch.cuda.get_device_name(0)}

    def emit(row):
        row = {**head, **row}
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_runs")}), flush=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    hip = mm.HipObjective(pb, device=0)
    theta = np.ascontiguousarray(mm.draws.jitter_draws(pb, 11, B))
    theta[0] = pb.base_theta
    for J in (int(x) for x in a.particles.split(",")):
        for k in (INF, 1.0):
            row, got = timing(mm, hip, theta, a.steps, J, k, a.reps)
            emit(row)
            emit(lowest_ess_rows(pb, got, J, k))
    hip.close()


if __name__ == "__main__":
    main()
