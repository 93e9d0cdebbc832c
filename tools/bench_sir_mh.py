#!/usr/bin/env python3
"""Proposals/s of the Adaptive-Metropolis sampler on the age-structured SIR objective (diagnostic; not part of bench.py).

Runs on the GPU only, one process, one box.  For BASELINE configs[0]'s three-age problem (P = 5) and the sixteen-age synthetic
problem of tools/bench_sir.py (P = 18), Dopri5, at 4096 and 65 536 chains:
  (a) the bare evaluation step, tools/bench_sir.py's method (device-resident theta, launches between two device events);
  (b) the iteration of the self-contained device-resident sampler (sepaihrd_sir_mh_create, seed_streams +
      keep_scale_on_device: the host only queues iterations) with the block-per-chain form of its per-iteration kernels;
  (c) the same with the packed form -- (b) and (c) ALTERNATE on one sampler object, window by window;
  (d) the host loop MultiChainMetropolisHastings::optimizeChains on the same objective over a short fixed iteration count:
      what a user of the SIR path had before the sampler went to the device (wall time of the call, set-up included).
A window of (b) / (c) is at least --min-seconds long and runs from a drained stream to a drained stream (the sampler's
stream is its own, so the window's ends are host clock readings around sepaihrd_mh_read_run_state, which waits for it);
three windows per form, the median is reported and the windows are kept.
One JSON line per row is appended to profiles/sir_sampler_bench.jsonl.

    python tools/bench_sir_mh.py [--arith fma|strict] [--min-seconds 0.5] [--host-iterations 30]
    python tools/bench_sir_mh.py --only packed --problem config0_n3 --chains 65536 --iterations 300   # under a profiler
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

ADAPTATION_PERIOD = 100


class Sampler:
    """the self-contained sampler through the C ABI, queued the way optimizeChainsOnDevice queues it (burn-in 0)"""

    def __init__(self, mm, hip, x0, cov0, capacity, seed=1):
        from mmid_amd import hipabi
        self.hipabi, self.lib, self.hip = hipabi, hipabi.load_library(), hip
        self.C, self.P = x0.shape
        self.capacity = capacity
        self.mh = hipabi.sir_mh_create(self.lib, hip.ctx, self.C, capacity, x0, cov0, thinning=capacity, adaptation_window=ADAPTATION_PERIOD + 1)
        if not self.mh:
            raise RuntimeError("sepaihrd_sir_mh_create: " + self.lib.sepaihrd_sir_last_error(hip.ctx).decode())
        lp, st = np.empty(self.C), np.empty(self.C, dtype=np.int32)
        self.ok(self.lib.sepaihrd_mh_evaluate_current(self.mh, lp.ctypes.data, st.ctypes.data))
        lp = np.where((st >= 2) | ~np.isfinite(lp), -1e18, lp)
        self.ok(self.lib.sepaihrd_mh_keep_scale_on_device(self.mh, 1, 0.234, 0))
        self.ok(self.lib.sepaihrd_mh_set_values(self.mh, lp.ctypes.data))
        self.ok(self.lib.sepaihrd_mh_seed_streams(self.mh, seed))
        self.ok(self.lib.sepaihrd_mh_draw_first(self.mh))
        ones = np.ones(self.C)
        self.ok(self.lib.sepaihrd_mh_step(self.mh, None, ones.ctypes.data, None, None, 0, 10.0 / 101.0, self.adapt_mode(1)))
        self.t = 1

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.sepaihrd_sir_last_error(self.hip.ctx).decode())

    def adapt_mode(self, t):
        if t % ADAPTATION_PERIOD != 0:
            return 1
        return 3 if t >= self.P + 10 else 2

    def set_form(self, form):
        self.ok(self.hipabi.mh_set_kernel_form(self.lib, self.mh, form))

    def drain(self):
        acc = np.empty(self.C, dtype=np.int32)
        self.ok(self.lib.sepaihrd_mh_read_run_state(self.mh, None, None, None, acc.ctypes.data, None))
        return acc

    def run(self, n):
        """n iterations queued, then the stream drained; seconds from drained to drained"""
        if self.t + n + 1 >= self.capacity:
            raise RuntimeError("sampler capacity exhausted")
        self.drain()
        t0 = time.perf_counter()
        for _ in range(n):
            self.ok(self.lib.sepaihrd_mh_step_tested(self.mh, 10.0 / ((self.t + 1) + 100.0), self.adapt_mode(self.t + 1), 0))
            self.t += 1
        acc = self.drain()
        return time.perf_counter() - t0, acc

    def close(self):
        if self.mh:
            self.lib.sepaihrd_mh_destroy(self.mh)
            self.mh = None


def bare_step(torch, hip, theta, min_seconds):
    B = len(theta)
    d_theta = torch.tensor(theta, dtype=torch.float64, device="cuda")
    d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
    d_st = torch.empty(B, dtype=torch.int32, device="cuda")
    for _ in range(5):
        hip.eval_batch_device(d_theta, d_ll, d_st)
    torch.cuda.synchronize()
    reps, windows = 4, []
    while len(windows) < 3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            hip.eval_batch_device(d_theta, d_ll, d_st)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms / 1e3 >= min_seconds:
            windows.append(ms / reps)
        else:
            reps *= 2
    return windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="fma", choices=["fma", "strict"])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--host-iterations", type=int, default=30)
    ap.add_argument("--only", choices=["block", "packed"], help="one form, --iterations of it, nothing else (profiler runs)")
    ap.add_argument("--problem", default=None, choices=["config0_n3", "synthetic_n16"])
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=300)
    a = ap.parse_args()
    import oracle_py
    import mmid_amd_loader
    mm = mmid_amd_loader.load()
    from bench_sir import sixteen_age_problem
    from mmid_amd import hipabi
    import torch
    assert torch.cuda.is_available(), "bench_sir_mh.py needs a GPU"
    forms = {"block": hipabi.MH_FORM_BLOCK_PER_CHAIN, "packed": hipabi.MH_FORM_PACKED}
    arith = mm.ARITH_FMA if a.arith == "fma" else mm.ARITH_STRICT
    problems = {"config0_n3": mm.workloads.sir_config0(oracle_py.sir_simulate), "synthetic_n16": sixteen_age_problem(mm, oracle_py)}
    if a.problem:
        problems = {a.problem: problems[a.problem]}
    out_path = os.path.join(ROOT, "profiles", "sir_sampler_bench.jsonl")
    for name, pb0 in problems.items():
        pb = pb0.with_(solver=mm.SOLVER_DOPRI5, arith=arith)
        P = pb.n_params
        truth = pb.current_parameters()
        cov0 = np.diag((0.02 * truth) ** 2) * (2.38 * 2.38 / P) + 1e-6 * np.eye(P)
        for B in ((a.chains,) if a.chains else (4096, 65536)):
            rng = np.random.default_rng(1)
            x0 = truth * np.exp(rng.normal(0.0, 0.01, size=(B, P)))
            hip = mm.HipSIRObjective(pb)
            if a.only:
                s = Sampler(mm, hip, x0, cov0, a.iterations + 64)
                s.set_form(forms[a.only])
                dt, acc = s.run(a.iterations)
                print(json.dumps({"tool": "bench_sir_mh", "only": a.only, "problem": name, "chains": B, "iterations": a.iterations,
                                  "ms_per_iteration": dt / a.iterations * 1e3}))
                s.close()
                hip.close()
                continue
            base = {"tool": "bench_sir_mh", "problem": name, "n_age": pb.n, "n_params": P, "n_times": pb.n_times, "chains": B, "arith": a.arith,
                    "solver": "dopri5", "device": torch.cuda.get_device_name(0)}
            rows = []
            # (a): at the sampler's own states' neighbourhood (the starts), as the sampler evaluates them
            wa = bare_step(torch, hip, x0, a.min_seconds)
            step_ms = float(np.median(wa))
            rows.append(dict(base, row="a_bare_evaluation", ms=step_ms, ms_windows=wa, per_s=B / (step_ms / 1e3)))
            # (b) / (c), alternating on one sampler
            s = Sampler(mm, hip, x0, cov0, 400000)
            s.set_form(forms["block"])
            s.run(40)
            dt, _ = s.run(60)
            n = max(20, int(np.ceil(1.15 * a.min_seconds / (dt / 60))))
            win = {"block": [], "packed": []}
            accepted_before = s.drain().astype(np.int64).sum()
            t_before = s.t
            while len(win["packed"]) < 3:
                for f in ("block", "packed"):
                    s.set_form(forms[f])
                    dt, acc = s.run(n)
                    if dt < a.min_seconds:  # the estimate was short: this pair of windows is not kept
                        n = int(np.ceil(1.3 * n * a.min_seconds / dt))
                        win = {k: w[:len(win["packed"])] for k, w in win.items()}
                        break
                    win[f].append(dt / n * 1e3)
            rate = float((acc.astype(np.int64).sum() - accepted_before) / (B * (s.t - t_before)))
            med = {f: float(np.median(w)) for f, w in win.items()}
            spread = {f: float((max(w) - min(w)) / med[f]) for f, w in win.items()}
            for f, key in (("block", "b_sampler_block_per_chain"), ("packed", "c_sampler_packed")):
                rows.append(dict(base, row=key, ms=med[f], ms_windows=win[f], window_spread=spread[f], iterations_per_window=n,
                                 per_s=B / (med[f] / 1e3), vs_bare_step=med[f] / step_ms, acceptance=rate))
            rows.append(dict(base, row="c_over_b", ratio=med["packed"] / med["block"], spread_block=spread["block"], spread_packed=spread["packed"],
                             packed_wins_beyond_the_spread=bool(med["block"] - med["packed"] > max(spread.values()) * med["block"])))
            s.close()
            hip.close()
            # (d): the host loop, what a user of this objective had before
            h = mm.HostSIRObjective(pb)
            h.metropolis_hastings_ex(x0[:64], seed=1, iterations=4, device_state=False, want_trace=False, thinning=4)
            t0 = time.perf_counter()
            h.metropolis_hastings_ex(x0, seed=1, iterations=a.host_iterations, device_state=False, want_trace=False, thinning=a.host_iterations)
            dt = time.perf_counter() - t0
            ms_d = dt / (a.host_iterations - 1) * 1e3
            rows.append(dict(base, row="d_host_loop", ms=ms_d, iterations=a.host_iterations, per_s=B / (ms_d / 1e3), vs_bare_step=ms_d / step_ms,
                             host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")),
                             device_over_host=ms_d / min(med.values())))
            del h
            with open(out_path, "a") as fh:
                for r in rows:
                    print(json.dumps(r))
                    fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
