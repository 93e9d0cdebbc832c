#!/usr/bin/env python3
"""End-to-end calibration run on the device path, shaped like the reference's `main --algorithm hill` / `--algorithm
pso` (src/model/main.cpp:383-560): Hill-Climbing or particle-swarm phase -> conditioned covariance -> Adaptive-Metropolis chains ->
posterior trace files in the sampler's CSV format (MetropolisHastingsSampler.cpp:414-438) -> post-calibration
ensemble (posterior predictive quantiles, seroprevalence and Rt trajectories, per-sample metric table).

    python tools/run_calibration.py --problem tests/golden/shipped_problem.json --out gpurun_out/calibration

The problem is a fixture JSON (tests/golden/make_fixtures.py builds them from a reference-format configuration
directory through config_io.py).  Settings use the reference's keys and defaults
(data/configuration/{hill_climbing,mcmc}_settings.txt)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmid_amd_loader  # noqa: E402

PROBS = [0.025, 0.05, 0.5, 0.95, 0.975]
SERIES = ["daily_hospitalizations", "daily_icu_admissions", "daily_deaths", "cumulative_hospitalizations",
          "cumulative_icu_admissions", "cumulative_deaths"]
METRICS = ["R0", "overall_IFR", "overall_attack_rate", "peak_hospital", "peak_ICU", "time_to_peak_hospital",
           "time_to_peak_ICU", "total_deaths", "max_Rt", "min_Rt", "final_Rt", "seroprevalence_day64"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default=os.path.join(ROOT, "tests", "golden", "shipped_problem.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "calibration"))
    ap.add_argument("--algorithm", choices=["hill", "pso"], default="hill")
    ap.add_argument("--pso-iterations", type=int, default=100)
    ap.add_argument("--swarm-size", type=int, default=256)
    ap.add_argument("--pso-variant", type=int, default=0)
    ap.add_argument("--pso-topology", type=int, default=0)
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--hc-iterations", type=int, default=60)
    ap.add_argument("--hc-threads", type=int, default=16)
    ap.add_argument("--cloud-size-multiplier", type=int, default=8)
    ap.add_argument("--mcmc-iterations", type=int, default=2000)
    ap.add_argument("--burn-in", type=int, default=500)
    ap.add_argument("--adaptation-period", type=int, default=100)
    ap.add_argument("--thinning", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--arith", choices=["fma", "strict"], default="fma")
    ap.add_argument("--scenarios", action="store_true",
                    help="also the NPI scenario analysis (scenarios/scenario_comparison.csv, the reference's three rows from the "
                         "last analysed sample; scenarios/scenario_posterior.json, every pooled sample under every scenario) "
                         "and seroprevalence/ene_covid_validation.csv")
    ap.add_argument("--diagnostics", action="store_true",
                    help="also the chains' convergence diagnostics on the device (split R-hat, bulk / tail ESS over the post-burn-in "
                         "samples): parameter_posteriors/posterior_diagnostics.csv, and max_r_hat / min_ess_bulk / min_ess_tail in "
                         "run_summary.json")
    ap.add_argument("--predictive-replicates", type=int, default=0,
                    help="also the replicated-data check (posterior_predictive/<series>_predictive_*.csv, pit_*.csv, "
                         "predictive_coverage.csv, predictive_scores.csv): this many replicates per pooled sample, drawn under the "
                         "problem's observation model -- negative-binomial where the problem carries a dispersion (fixed or "
                         "calibrated), else Poisson -- and scored against the observations on the device")
    ap.add_argument("--predictive-levels", default="0.5,0.9,0.95",
                    help="central coverage levels of predictive_scores.csv (interval score and coverage per level, and the WIS over "
                         "them): up to 8 values inside (0, 1), comma-separated")
    ap.add_argument("--predictive-window", type=int, default=0,
                    help="with --predictive-replicates: also score the replicates on totals over windows of this many output rows (7 on "
                         "a daily grid: weekly totals) and on their running sums, on the device: "
                         "posterior_predictive/predictive_target_scores.csv")
    ap.add_argument("--predictive-age-groups", default=None,
                    help="the age groups those totals are summed over: all (one group, the default), each (a group per age) or lists "
                         "of ages such as '0,1;2,3' (';' between groups; an age in no list is left out).  Alone it scores every output "
                         "row on its own (a window of 1)")
    args = ap.parse_args()

    mm = mmid_amd_loader.load()
    pb = mm.SEPAIHRDProblem.load(args.problem)
    pb = pb.with_(arith=mm.ARITH_FMA if args.arith == "fma" else mm.ARITH_STRICT, constraint_mode=0)
    os.makedirs(args.out, exist_ok=True)
    host = mm.HostObjective(pb)

    if args.diagnostics:
        host.set_mh_diagnostics(True)
    t0 = time.perf_counter()
    if args.algorithm == "pso":
        cal = host.calibrate_pso(dict(iterations=args.pso_iterations, swarm_size=args.swarm_size, variant=args.pso_variant,
                                      topology=args.pso_topology, seed=args.seed),
                                 mh_seed=args.seed + 1, mh_iterations=args.mcmc_iterations, burn_in=args.burn_in,
                                 adaptation_period=args.adaptation_period, thinning=args.thinning, chains=args.chains)
    else:
        cal = host.calibrate(hc_seed=args.seed, mh_seed=args.seed + 1, hc_iterations=args.hc_iterations,
                           mh_iterations=args.mcmc_iterations, burn_in=args.burn_in,
                           cloud_size_multiplier=args.cloud_size_multiplier, threads=args.hc_threads,
                           adaptation_period=args.adaptation_period, thinning=args.thinning, chains=args.chains)
    t_cal = time.perf_counter() - t0
    diag = host.mh_diagnostics() if args.diagnostics else None
    if args.diagnostics and diag is None:
        raise SystemExit("--diagnostics: the run formed no diagnostics (fewer than 4 stored samples after burn-in?)")
    for c in range(args.chains):
        mm.config_io.write_posterior_trace_csv(os.path.join(args.out, f"posterior_trace_chain{c}.csv"), cal["samples"][c],
                                               cal["sample_values"][c], list(pb.param_names))
    with open(os.path.join(args.out, "calibrated_parameters_final.txt"), "w") as fh:
        fh.write(f"# best objective value: {cal['best_value']:.8e}\n")
        for name, v in zip(pb.param_names, cal["best"]):
            fh.write(f"{name} {v:.10g}\n")

    # post-calibration ensemble over the pooled post-burn-in samples of every chain, from the initial state
    # of the problem as given (SimulationRunner::runSimulation)
    first = args.burn_in // max(1, args.thinning) + 1
    pooled = cal["samples"][:, first:, :].reshape(-1, pb.n_params)
    pooled = pooled[:16384]
    t0 = time.perf_counter()
    hip = mm.HipObjective(pb.with_(constraint_mode=1))
    hip.set_initial_state_mode(1)
    ens = hip.ensemble_quantiles(pooled, PROBS, want_sero=True, want_rt=True, want_metrics=True)
    t_ens = time.perf_counter() - t0
    predictive = None
    if args.predictive_replicates > 0:
        # the context's dispersion, per sample: Poisson draws where the problem carries none (three +inf; a calibrated one reads NaN)
        dispersed = not np.all(np.isposinf(hip.get_dispersion()))
        levels = [float(c) for c in args.predictive_levels.split(",") if c.strip()]
        predictive = hip.ensemble_predictive_scores(pooled, args.predictive_replicates, args.seed + 2, PROBS, levels)
        if args.predictive_window > 0 or args.predictive_age_groups is not None:
            groups = mm.config_io.parse_age_groups(args.predictive_age_groups or "all", pb.n)
            targets = hip.ensemble_predictive_targets(pooled, args.predictive_replicates, args.seed + 2, PROBS, levels, groups,
                                                      args.predictive_window if args.predictive_window > 0 else 1)
            os.makedirs(os.path.join(args.out, "posterior_predictive"), exist_ok=True)
            mm.config_io.write_predictive_target_scores(os.path.join(args.out, "posterior_predictive", "predictive_target_scores.csv"), targets)
    elif args.predictive_window > 0 or args.predictive_age_groups is not None:
        raise SystemExit("--predictive-window and --predictive-age-groups need --predictive-replicates")
    times = np.asarray(pb.times)
    pos = times[times >= 0]
    # the reference's post-calibration output tree (file names, headers and number formats of AnalysisWriter.cpp; what
    # scripts/model/PostCalibrationAnalysis.py loads): posterior_predictive/, parameter_posteriors/, rt_trajectories/,
    # seroprevalence/, mcmc_batches/, mcmc_aggregated/ (and with --scenarios: scenarios/, seroprevalence/ene_covid_validation.csv)
    observed = {"daily_hospitalizations": pb.obs_H, "daily_icu_admissions": pb.obs_ICU, "daily_deaths": pb.obs_D,
                "cumulative_hospitalizations": np.cumsum(pb.obs_H, axis=0), "cumulative_icu_admissions": np.cumsum(pb.obs_ICU, axis=0),
                "cumulative_deaths": np.cumsum(pb.obs_D, axis=0)}
    scenario_rows = None
    if args.scenarios:
        # the reference's baseline: the last analysed sample after the constraints (PostCalibrationAnalyser.cpp:100-109,
        # 210-219), one run per scenario
        scen = mm.config_io.default_lockdown_scenarios(len(pb.kappa_values))
        table = np.array([m for _, m in scen])
        last = pooled[-1:]
        three = hip.scenario_ensemble(last, table, PROBS)
        c = hip.apply_constraints(last, 1)[0]
        scenario_rows = mm.config_io.scenario_comparison_rows(
            [name for name, _ in scen], three["metrics"][:, 0], three["status"][:, 0],
            [mm.config_io.scenario_kappa_values(pb, c, m) for _, m in scen], pb.n)
        # the posterior-wide form: every pooled sample under every scenario, paired differences against the baseline
        wide = hip.scenario_ensemble(pooled, table, PROBS)
        cols = mm.config_io.essential_metric_columns(pb.n)
        post = {name: {"n_valid": int(wide["n_valid"][k]),
                       "metrics": {col: dict(zip(["mean", "std_dev"] + [f"q{p}" for p in PROBS], map(float, wide["summary"][k, j])))
                                   for j, col in enumerate(cols)},
                       "difference_to_baseline": {col: dict(zip([f"q{p}" for p in PROBS], map(float, wide["diff"][k, j])))
                                                  for j, col in enumerate(cols)}}
                for k, (name, _) in enumerate(scen)}
        os.makedirs(os.path.join(args.out, "scenarios"), exist_ok=True)
        with open(os.path.join(args.out, "scenarios", "scenario_posterior.json"), "w") as fh:
            json.dump(post, fh, indent=1)
    mm.config_io.write_post_calibration_tree(args.out, times, ens, pooled, list(pb.param_names), pb.n, observed=observed,
                                             scenarios=scenario_rows, ene_covid=args.scenarios, diagnostics=diag,
                                             predictive=predictive)
    assert len(pos) == ens["ppc"].shape[2]

    evals = args.chains * args.mcmc_iterations
    summary = {"initial_value": cal["initial_value"], "phase1_best_value": cal["phase1_best_value"],
               "best_value": cal["best_value"], "algorithm": args.algorithm, "chains": args.chains, "mcmc_iterations": args.mcmc_iterations,
               "acceptance_rate_mean": float(cal["accept_trace"].mean()), "calibration_seconds": t_cal,
               "proposals_per_s": evals / t_cal, "ensemble_samples": int(len(pooled)), "ensemble_valid": int(ens["n_valid"]),
               "ensemble_seconds": t_ens, "predictive_noise": None if predictive is None else ("negative_binomial" if dispersed else "poisson"),
               "median_R0": float(np.nanmedian(ens["metrics"][:, 0])), "out": args.out}
    if diag is not None:
        summary.update(max_r_hat=float(np.nanmax(diag[:, 6])), min_ess_bulk=float(np.nanmin(diag[:, 4])),
                       min_ess_tail=float(np.nanmin(diag[:, 5])))
    with open(os.path.join(args.out, "run_summary.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
