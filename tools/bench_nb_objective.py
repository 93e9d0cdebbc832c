#!/usr/bin/env python3
"""What the negative-binomial observation model of the deterministic objective costs (sepaihrd_set_dispersion; DESIGN.md section
6o): a dispersed against a Poisson evaluation of the same parameter vectors, in the same process (diagnostic; not part of bench.py,
run by no test).

Two workloads of BASELINE.json, in the arithmetic bench.py measures (fma): configs[1], 4096 chains, and 32 768 chains of configs[3]'s
share.  Per workload three contexts over one set of jittered draws on the device:
  poisson   the shipped objective (whatever form the launch code picks for the batch)
  nb_k10    k = 10 for the three series: the integrator in the form that parks its increments, then the negative-binomial pass
  nb_mixed  k = (10, +inf, 10): the same pass with one Poisson series
They are launched alternately, --steps launches each per round, --reps rounds after one warm-up round; the integrator and the
likelihood pass are timed separately with sepaihrd_set_timing (device events around each) and the round's wall time with a host
clock around launches that end in a synchronise.  Medians over the rounds; the runs are kept in the file.
Appends to profiles/nb_objective_bench.jsonl.

    python tools/bench_nb_objective.py [--steps 20] [--reps 5] [--workloads c1,c3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INF = float("inf")
FORMS = {"poisson": None, "nb_k10": (10.0, 10.0, 10.0), "nb_mixed": (10.0, INF, 10.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="launches per context and round")
    ap.add_argument("--reps", type=int, default=5, help="timed rounds (one more warms up)")
    ap.add_argument("--workloads", default="c1,c3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_nb_objective.py needs a GPU"
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    out = a.out or os.path.join(ROOT, "profiles", "nb_objective_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    dev = torch.device("cuda:0")
    for name in a.workloads.split(","):
        pb = mm.workloads.build(name, os.path.join(ROOT, "tests", "golden"))
        pb.arith = mm.ARITH_FMA
        B = mm.workloads.DEFAULT_CHAINS[name]
        theta = torch.from_numpy(np.ascontiguousarray(mm.draws.jitter_draws(pb, 1, B))).to(dev)
        ctx, res = {}, {}
        for f, k in FORMS.items():
            ctx[f] = mm.HipObjective(pb, device=0)
            if k is not None:
                ctx[f].set_dispersion(k)
            ctx[f].reserve(B)
            res[f] = {"loglik": torch.empty(B, dtype=torch.float64, device=dev), "status": torch.empty(B, dtype=torch.int32, device=dev),
                      "parts": torch.empty((B, 3), dtype=torch.float64, device=dev)}
        runs = {f: {"integrator_ms": [], "likelihood_ms": [], "wall_ms": []} for f in FORMS}
        for rep in range(a.reps + 1):   # the first round warms up
            for f in FORMS:
                hip = ctx[f]
                hip.set_timing(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    hip.eval_batch_device(theta, res[f]["loglik"], res[f]["status"], d_ll_parts=res[f]["parts"], B=B)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3 / a.steps
                t = hip.get_timing()
                hip.set_timing(0)
                if rep > 0:
                    runs[f]["integrator_ms"].append(t["integrator_ms"] / t["launches"])
                    runs[f]["likelihood_ms"].append(t["likelihood_ms"] / t["launches"])
                    runs[f]["wall_ms"].append(wall)
        row = {"tool": "bench_nb_objective", "workload": name, "chains": B, "n_age": pb.n, "n_times": pb.n_times, "arith": "fma",
               "steps": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        ok = {f: (res[f]["status"] == 0).cpu().numpy() for f in FORMS}
        for f in FORMS:
            info = ctx[f].kernel_info(B)
            row[f] = {"kernel": info["kernel_name"], "likelihood_form": info["likelihood_form"], "vgprs": info["vgprs"], "lds_bytes": info["lds_bytes"],
                      "valid_chains": int(ok[f].sum()), **{key: float(np.median(v)) for key, v in runs[f].items()},
                      **{key + "_runs": v for key, v in runs[f].items()}}
        # the mixed context's Poisson series has the Poisson run's bits
        pp, mp = res["poisson"]["parts"].cpu().numpy(), res["nb_mixed"]["parts"].cpu().numpy()
        row["mixed_icu_part_equals_poisson"] = bool(np.array_equal(pp[:, 1], mp[:, 1]))
        for f in ("nb_k10", "nb_mixed"):
            row[f + "_step_over_poisson"] = (row[f]["integrator_ms"] + row[f]["likelihood_ms"]) / (row["poisson"]["integrator_ms"] + row["poisson"]["likelihood_ms"])
        print(json.dumps({k: ({kk: vv for kk, vv in v.items() if not kk.endswith("_runs")} if isinstance(v, dict) else v) for k, v in row.items()}),
              flush=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        for hip in ctx.values():
            hip.close()


if __name__ == "__main__":
    main()
