#!/usr/bin/env python3
"""The negative-binomial observation model of the particle filters (sepaihrd_particle_loglik_nb, sepaihrd_particle_loglik_wide_nb):
how noisy the log-likelihood estimate is once the observed series carry a dispersion, and what the dispersed kernels cost
(diagnostic; not part of bench.py, run by no test).  DESIGN.md section 6m.

The shipped problem (n = 4, 326 output times, x(t0) seeded from theta) at its base theta with m = 4 steps per output interval:
the problem, the point and the seeds of tools/bench_particle_wide.py, whose Poisson figures section 6l records.  For a common k of
the three series in {+inf, 100, 10, 1}: loglik over 32 seeds (mean, standard deviation) and the mean ESS over the rows of the
first seed.  Particle-marginal Metropolis-Hastings mixes when the standard deviation is of order 1.

  default  on the GPU, one process, one box: J = sepaihrd_particle_max_particles(4) = 136 through the LDS kernel, J = 1024 and 8192
           through the wide form; per J also the wall time and the filter's device time per call (medians of --reps, one warm-up)
           of the Poisson call, of the _nb call with every k = +inf (which must run the Poisson kernels) and of the _nb call at
           k = 10, in the same process.  Appends to profiles/particle_nb_bench.jsonl.
  --twin   the host twin on the CPU (the same text; bit for bit the device's results) at J = 136 and 1024 only -- J = 8192 is too
           slow there; the model values of the base theta are formed here from the parameter manager's row and the seeding rule of
           the decode kernel.  No timings.  Appends to profiles/particle_nb_spread_twin.jsonl.

    python tools/bench_particle_nb.py [--twin] [--particles 1024,8192] [--steps 4] [--reps 3] [--threads 16] [--out FILE]
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

SEED = 20261020   # tools/bench_particle_wide.py's
SD_SEEDS = 32
INF = float("inf")
DISPERSIONS = (INF, 100.0, 10.0, 1.0)
TIMED_K = 10.0
TIMING_B = 64


def summary(ll, ess):
    ll = np.asarray(ll)
    return {"seeds": len(ll), "loglik_mean": float(ll.mean()), "loglik_sd": float(ll.std(ddof=1)), "loglik_min": float(ll.min()),
            "loglik_max": float(ll.max()), "weighted_rows": int(np.isfinite(ess).sum()), "mean_ess_first_seed": float(np.nanmean(ess)),
            "min_ess_first_seed": float(np.nanmin(ess)), "loglik": ll.tolist()}


def base_model_values(mm, pb):
    """the model-values row of the base theta as the decode kernel forms it for a problem seeded from theta: the parameter manager's
    row, then per age class E = seed_exposed N_i / sum N, nobody in the other compartments, S by subtraction, every count rounded
    half away from zero"""
    host = mm.hostabi.HostObjective(pb, with_objective=False)
    theta = np.asarray(pb.base_theta, dtype=np.float64)
    con = host.apply_constraints(theta[None], 0)[0]
    names = list(pb.param_names)
    seed_exposed, runup_days = con[names.index("seed_exposed")], con[names.index("runup_days")]
    if not (runup_days > 0 and seed_exposed > 0):
        raise SystemExit("--twin forms the initial counts of a problem seeded from theta (runup_days > 0, seed_exposed > 0) only")
    N = np.asarray(pb.N, dtype=np.float64)
    total = 0.0
    for v in N:
        total += v
    x = np.zeros((11, pb.n))
    x[1] = seed_exposed * (N / total)
    x[0] = N - x[1]
    x = np.copysign(np.floor(np.abs(x) + 0.5), x)
    return np.concatenate([host.stochastic_manager_values(theta, 0), x.ravel()])[None]


def twin_spread(mm, pb, row, m, J, wide, k, threads):
    disp = None if k is None else (k, k, k)
    call = mm.hostabi.particle_wide_from_values if wide else mm.hostabi.particle_from_values
    status = np.zeros(1, dtype=np.int32)

    def one(s):
        return call(row, status, pb.times, pb.N, pb.M, pb.kappa_end_times, pb.obs_H, pb.obs_ICU, pb.obs_D, J, m, SEED + s,
                    beta_end_times=pb.beta_end_times, want_final=False, dispersion=disp)

    with ThreadPoolExecutor(threads) as pool:   # the library call releases the interpreter lock; one position per call, as on the device
        runs = list(pool.map(one, range(SD_SEEDS)))
    return summary([r["loglik"][0] for r in runs], runs[0]["ess"][0])


def device_spread(hip, pb, m, J, wide, k):
    call = hip.particle_loglik_wide if wide else hip.particle_loglik
    kw = {} if k is None else {"dispersion": (k, k, k)}
    ll, ess = [], None
    for s in range(SD_SEEDS):
        got = call(pb.base_theta, J, m, SEED + s, want_increments=False, want_ess=s == 0, **kw)
        assert got["status"][0] == 0
        ll.append(float(got["loglik"][0]))
        if s == 0:
            ess = got["ess"][0]
    return summary(ll, ess)


def device_timing(mm, hip, pb, m, J, wide, reps):
    """the Poisson call, the _nb call at +inf and the _nb call at TIMED_K on TIMING_B vectors around the base point, interleaved"""
    distinct = mm.draws.jitter_draws(pb, 11, TIMING_B)
    theta = np.ascontiguousarray(distinct)
    call = hip.particle_loglik_wide if wide else hip.particle_loglik
    clock = hip.particle_wide_timing if wide else hip.particle_timing
    forms = {"poisson": {}, "nb_inf": {"dispersion": (INF, INF, INF)}, "nb_k10": {"dispersion": (TIMED_K,) * 3}}
    wall, dev, ll = {f: [] for f in forms}, {f: [] for f in forms}, {}
    for rep in range(reps + 1):   # the first round warms up
        for f, kw in forms.items():
            t0 = time.perf_counter()
            got = call(theta, J, m, SEED, want_increments=False, want_ess=False, **kw)
            w = (time.perf_counter() - t0) * 1e3
            if rep > 0:
                wall[f].append(w)
                dev[f].append(float(clock()[1]))
            ll[f] = got["loglik"]
    row = {"part": "timing", "form": "wide" if wide else "lds", "B": TIMING_B, "J": J, "reps": reps,
           "nb_inf_equals_poisson": bool(np.array_equal(ll["poisson"], ll["nb_inf"]))}
    for f in forms:
        row[f + "_wall_ms"] = float(np.median(wall[f]))
        row[f + "_filter_ms"] = float(np.median(dev[f]))
        row[f + "_filter_ms_runs"] = dev[f]
    row["nb_inf_over_poisson"] = row["nb_inf_filter_ms"] / row["poisson_filter_ms"]
    row["nb_k10_over_poisson"] = row["nb_k10_filter_ms"] / row["poisson_filter_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--twin", action="store_true", help="the host twin on the CPU instead of the device")
    ap.add_argument("--particles", default=None, help="comma-separated J of the wide form (default 1024,8192; with --twin 1024)")
    ap.add_argument("--steps", type=int, default=4, help="steps per output interval")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="--twin: seeds in flight")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.twin:
        os.environ.setdefault("OMP_NUM_THREADS", "1")   # one position per call: the seeds run side by side instead
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    pb = mm.SEPAIHRDProblem.load(os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    out = a.out or os.path.join(ROOT, "profiles", "particle_nb_spread_twin.jsonl" if a.twin else "particle_nb_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    J_lds = mm.hostabi.particle_max_particles(pb.n)
    particles = [int(x) for x in (a.particles or ("1024" if a.twin else "1024,8192")).split(",")]
    head = {"tool": "bench_particle_nb", "problem": "shipped", "n_age": pb.n, "n_times": pb.n_times, "steps_per_interval": a.steps, "seed": SEED,
            "theta": "base"}

    def emit(row):
        row = {**head, **row}
        print(json.dumps({k: v for k, v in row.items() if k != "loglik" and not k.endswith("_runs")}), flush=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    shapes = [(J_lds, False)] + [(J, True) for J in particles]
    if a.twin:
        head["device"] = "host twin"
        row = base_model_values(mm, pb)
        for J, wide in shapes:
            for k in DISPERSIONS:
                t0 = time.perf_counter()
                got = twin_spread(mm, pb, row, a.steps, J, wide, k, a.threads)
                emit({"part": "sd", "J": J, "form": "wide" if wide else "lds", "k": "inf" if k == INF else k, **got,
                      "wall_s": time.perf_counter() - t0})
        return
    import torch
    assert torch.cuda.is_available(), "bench_particle_nb.py needs a GPU (or --twin)"
    head["device"] = torch.cuda.get_device_name(0)
    hip = mm.HipObjective(pb, device=0)
    for J, wide in shapes:
        for k in DISPERSIONS:
            emit({"part": "sd", "J": J, "form": "wide" if wide else "lds", "k": "inf" if k == INF else k, **device_spread(hip, pb, a.steps, J, wide, k)})
        emit(device_timing(mm, hip, pb, a.steps, J, wide, a.reps))
    hip.close()


if __name__ == "__main__":
    main()
