/* =============================================================================
 * include/sepaihrd_hip.h -- C ABI of the MI355X (gfx950) SEPAIHRD likelihood path.
 *
 * This is the drop-in boundary: everything below it is hand-written HIP, everything
 * above it is host orchestration (C++ adapters in
 * mathematical-modeling-of-infectious-diseases-v1_amd/host/, a ctypes shim for the
 * tests).  Plain pointers and sizes only; no torch / Eigen / STL types.
 *
 * What each entry point replaces in the reference (paths under /root/reference):
 *
 *   sepaihrd_create            the construction done in
 *                              SEPAIHRDObjectiveFunction::SEPAIHRDObjectiveFunction
 *                              (src/model/objectives/SEPAIHRDObjectiveFunction.cpp:22-50)
 *                              + SEPAIHRDParameterManager's name->field resolution
 *                              (src/model/parameters/SEPAIHRDParameterManager.cpp:197-267),
 *                              done once instead of per evaluation.
 *   sepaihrd_eval_batch        B calls of IObjectiveFunction::calculate
 *   sepaihrd_eval_batch_device (include/sir_age_structured/interfaces/IObjectiveFunction.hpp:24;
 *                              body SEPAIHRDObjectiveFunction.cpp:62-235), i.e. per chain:
 *                              applyConstraints + updateModelParameters
 *                              (SEPAIHRDParameterManager.cpp:164-347), initial state
 *                              (:124-163), Simulator::run -> IOdeSolverStrategy::integrate
 *                              (src/sir_age_structured/Simulator.cpp:60-150,
 *                               solvers/Dopri5SolverStrategy.cpp:28-37,
 *                               solvers/CashKarpSolverStrategy.cpp:18-25 -> Boost.Odeint
 *                               integrate_times + make_controlled),
 *                              AgeSEPAIHRDModel::computeDerivatives
 *                              (src/model/AgeSEPAIHRDModel.cpp:101-228) with the
 *                              piecewise beta(t)/kappa(t) lookups
 *                              (PiecewiseConstantParameterStrategy.cpp:37-74,
 *                               PieceWiseConstantNPIStrategy.cpp:86-127),
 *                              incidence differencing (:191-215) and the 3-stream
 *                              Poisson log-likelihood (:241-279, serial row order).
 *   sepaihrd_apply_constraints IParameterManager::applyConstraints
 *                              (SEPAIHRDParameterManager.cpp:315-347)
 * The lock-step multi-chain MetropolisHastingsSampler::optimize
 * (src/sir_age_structured/optimizers/MetropolisHastingsSampler.cpp:201-412) is a
 * CALLER of this boundary and lives in the C++ host library (host/), not here.
 *
 * Error convention: functions return 0 on success or a negative SEPAIHRD_E_* code;
 * nothing throws across this boundary.  Per-chain model failures never fail the
 * call: they are reported like the reference reports them --
 * loglik[b] = -DBL_MAX (std::numeric_limits<double>::lowest()) and status[b] != 0.
 * The library has NO CPU fallback: without a usable HIP device every entry point
 * that computes returns SEPAIHRD_E_NO_DEVICE.
 * ============================================================================= */
#ifndef SEPAIHRD_HIP_H
#define SEPAIHRD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: sepaihrd_problem.reserved0 became `precision`; per-chain status SEPAIHRD_STATUS_PIPELINE; the accept byte of
 *    sepaihrd_mh_commit / _step is a bit field; sepaihrd_mh_create takes a struct sepaihrd_mh_config: ring of newest states,
 *    thinned samples and running co-moments instead of the whole chain history; sepaihrd_mh_read_samples /
 *    _sample_count / _summary_records / _read_moments added. */
/* 3: sepaihrd_kernel_info.phase_pass_applied; sepaihrd_device_libm_check (seed_streams / keep_scale_on_device refuse with
 *    SEPAIHRD_E_UNSUPPORTED when the device's log / exp are not this host's libm); sepaihrd_mh_read_failure_counts;
 *    sepaihrd_mh_snapshot_begin / _end (checkpoints without stalling the queue). */
#define SEPAIHRD_ABI_VERSION 3
#define SEPAIHRD_NUM_COMPARTMENTS 11 /* S,E,P,A,I,H,ICU,R,D,CumH,CumICU (ModelConstants.hpp:18) */
#define SEPAIHRD_MAX_AGE_CLASSES 64  /* one lane per (chain, age class); 64/n chains per wavefront */
#define SEPAIHRD_MAX_SCHEDULE 32     /* max beta / kappa periods */

/* error codes */
#define SEPAIHRD_OK 0
#define SEPAIHRD_E_INVALID_ARG (-1)
#define SEPAIHRD_E_NO_DEVICE (-2)
#define SEPAIHRD_E_HIP (-3)
#define SEPAIHRD_E_UNSUPPORTED (-4)

/* solver: the dynamic type of the reference's IOdeSolverStrategy */
#define SEPAIHRD_SOLVER_DOPRI5 0      /* Dopri5SolverStrategy  */
#define SEPAIHRD_SOLVER_CASH_KARP54 1 /* CashKarpSolverStrategy */
#define SEPAIHRD_SOLVER_FEHLBERG78 2  /* FehlbergSolverStrategy: controlled runge_kutta_fehlberg78 (one lane per
                                         (chain, age class) only: no QUAD form, no F32 precision) */

/* constraint mode: SEPAIHRDParameterManager.hpp ConstraintMode */
#define SEPAIHRD_CONSTRAINT_CLAMP 0   /* OPTIMIZATION_CLAMP */
#define SEPAIHRD_CONSTRAINT_REFLECT 1 /* MCMC_REFLECT       */

/* arithmetic mode of the fp64 kernels */
#define SEPAIHRD_ARITH_STRICT 0 /* no FMA contraction: same operation sequence as the CPU build */
#define SEPAIHRD_ARITH_FMA 1    /* mul+add fused where the source order allows (each a*b+c rounded once) */

/* number type of the ODE state (BASELINE configs[4]: "fp32 vs fp64 tolerance sweep").  F64 is the reference's
 * arithmetic and the only mode with a parity contract.  F32: state, stage derivatives and model coefficients in fp32;
 * the log-likelihood (terms, log, sums), time and theta stay fp64, and the cumulative compartments the likelihood
 * differences (D, CumH, CumICU; also R) are integrated as per-output-interval fp32 accumulators folded into fp64
 * totals, so that a day's increment keeps full fp32 relative precision.  Accuracy vs F64 per tolerance: DESIGN.md 6.
 * 3 to 16 age classes; no ensemble summaries in F32; Dopri5 and Cash-Karp only (Fehlberg 7(8): SEPAIHRD_E_UNSUPPORTED). */
#define SEPAIHRD_PRECISION_F64 0
#define SEPAIHRD_PRECISION_F32 1

/* per-chain status */
#define SEPAIHRD_STATUS_OK 0
#define SEPAIHRD_STATUS_INVALID 1      /* calculate() returned lowest(): bad theta / S<0 / NaN total */
#define SEPAIHRD_STATUS_STEP_FAILURE 2 /* odeint step_adjustment_error (500 rejections): the reference
                                          lets SimulationException propagate out of calculate() */
#define SEPAIHRD_STATUS_STEP_BUDGET 3  /* build-side guard: max_attempts exhausted */
#define SEPAIHRD_STATUS_PIPELINE 4     /* build-side guard: the hand-off between the integrating wave and the wave that
                                          evaluates its Poisson terms (batches of <= 4096 chains) timed out; no value was
                                          produced.  Like 2 and 3 the C++ adapter raises SimulationException for it */

/* theta -> model field map (what the reference resolves from parameter NAMES on every call) */
enum sepaihrd_field {
    SEPAIHRD_F_NONE = -1, /* unknown name: ignored with a warning in the reference */
    SEPAIHRD_F_BETA = 0,
    SEPAIHRD_F_THETA = 1,
    SEPAIHRD_F_SIGMA = 2,
    SEPAIHRD_F_GAMMA_P = 3,
    SEPAIHRD_F_GAMMA_A = 4,
    SEPAIHRD_F_GAMMA_I = 5,
    SEPAIHRD_F_GAMMA_H = 6,
    SEPAIHRD_F_GAMMA_ICU = 7,
    SEPAIHRD_F_E0_MULT = 8,
    SEPAIHRD_F_P0_MULT = 9,
    SEPAIHRD_F_A0_MULT = 10,
    SEPAIHRD_F_I0_MULT = 11,
    SEPAIHRD_F_H0_MULT = 12,
    SEPAIHRD_F_ICU0_MULT = 13,
    SEPAIHRD_F_R0_MULT = 14,
    SEPAIHRD_F_D0_MULT = 15,
    SEPAIHRD_F_RUNUP_DAYS = 16,
    SEPAIHRD_F_SEED_EXPOSED = 17,
    SEPAIHRD_F_BETA_VALUE = 18,  /* index k: beta_values[k]   ("beta_<k+1>") */
    SEPAIHRD_F_KAPPA_VALUE = 19, /* index k: kappa_values[k], k >= 1 (k = 0 is the fixed baseline) */
    SEPAIHRD_F_A = 20,           /* index = age class, likewise below */
    SEPAIHRD_F_H_INFEC = 21,
    SEPAIHRD_F_P = 22,
    SEPAIHRD_F_H = 23,
    SEPAIHRD_F_ICU = 24,
    SEPAIHRD_F_D_H = 25,
    SEPAIHRD_F_D_ICU = 26,
    SEPAIHRD_F_D_COMMUNITY = 27,
    SEPAIHRD_F_DISPERSION = 28   /* index 0, 1, 2: the negative-binomial dispersion of the H, ICU, D series (sepaihrd_set_dispersion) */
};

/* Everything calculate() reads that does not depend on theta.  All pointers are HOST
 * pointers, copied at create time. */
typedef struct sepaihrd_problem {
    int32_t abi_version; /* SEPAIHRD_ABI_VERSION */
    int32_t n_age;       /* n, 1..64 */
    int32_t n_times;     /* T output points, strictly increasing */
    int32_t n_obs;       /* rows of the observed matrices; must equal #times >= 0 or every
                            evaluation returns lowest() (SEPAIHRDObjectiveFunction.cpp:176) */
    int32_t n_beta;      /* beta schedule length, 0 = constant beta */
    int32_t n_kappa;     /* kappa schedule length incl. baseline, >= 1 */
    int32_t n_params;    /* P = length of theta */
    int32_t solver;
    int32_t constraint_mode;
    int32_t arith;
    int32_t max_attempts; /* 0 = default (1 000 000 step attempts per chain) */
    int32_t precision;    /* SEPAIHRD_PRECISION_F64 (0, default) or _F32 */

    const double *times;          /* [T] */
    const double *N;              /* [n] */
    const double *M;              /* [n*n] column-major like Eigen: M[j*n+i] = M(i,j) */
    const double *a, *h_infec, *p, *h, *icu, *d_H, *d_ICU, *d_community; /* [n]; d_community may be NULL */
    const double *beta_end_times, *beta_values;   /* [n_beta] */
    const double *kappa_end_times, *kappa_values; /* [n_kappa], baseline first */
    const double *initial_state;  /* [11 n] compartment-major, the objective's initial_state_ */
    const double *obs_H, *obs_ICU, *obs_D; /* [n_obs * n] row-major (row = day, col = age) */

    const int32_t *param_field;   /* [P] enum sepaihrd_field */
    const int32_t *param_index;   /* [P] element index for indexed fields, else 0 */
    const double *lower, *upper;  /* [P] */
    const uint8_t *has_bounds;    /* [P] 0 = no entry in param_bounds (abs()/max(0,.) rule) */

    double beta, theta, sigma, gamma_p, gamma_A, gamma_I, gamma_H, gamma_ICU;
    double multipliers[8];        /* E0,P0,A0,I0,H0,ICU0,R0,D0 */
    double runup_days, seed_exposed;
    double abs_err, rel_err, dt_hint;
} sepaihrd_problem;

typedef struct sepaihrd_ctx sepaihrd_ctx;

/* device < 0: current HIP device.  err (nullable) receives a message on failure. */
sepaihrd_ctx *sepaihrd_create(const sepaihrd_problem *problem, int device, char *err, int errlen);
void sepaihrd_destroy(sepaihrd_ctx *ctx);
const char *sepaihrd_last_error(const sepaihrd_ctx *ctx);
int sepaihrd_abi_version(void);

/* MCMC_REFLECT <-> OPTIMIZATION_CLAMP switch between calibration phases
 * (ModelCalibrator.cpp:64,90; MetropolisHastingsSampler.cpp:207-209). */
int sepaihrd_set_constraint_mode(sepaihrd_ctx *ctx, int mode);
int sepaihrd_set_arith(sepaihrd_ctx *ctx, int arith);
int sepaihrd_set_precision(sepaihrd_ctx *ctx, int precision);
/* Which form of the fp64 integrator a launch uses.  AUTO (default): by batch size -- up to 4096 chains of a problem with
 * 3 or 4 age classes sixteen lanes integrate a chain (a quad of lanes per age class, so that a batch too small to fill
 * the chip spreads over four times as many SIMDs), beyond that one lane per (chain, age class).  Both forms round every
 * operation alike: log-likelihood, status, step counts and trajectories are the same bits, and the parity suite proves it
 * by forcing each form on the same chains.  QUAD on other age counts or with the Fehlberg 7(8) solver (which AUTO never
 * runs in the QUAD form): SEPAIHRD_E_UNSUPPORTED. */
#define SEPAIHRD_FORM_AUTO 0
#define SEPAIHRD_FORM_LANE_PER_AGE 1
#define SEPAIHRD_FORM_QUAD 2
int sepaihrd_set_integrator_form(sepaihrd_ctx *ctx, int form);

/* Host-pointer form.  theta: B x P, chain-major (one Eigen::VectorXd after another).
 * Outputs (any may be NULL except loglik): loglik[B]; status[B]; n_accept[B]/n_reject[B] =
 * accepted / rejected RK step attempts; ll_parts[B*3] = (hosp, icu, deaths) stream sums;
 * traj[B*T*11n] = SimulationResult::solution per chain (row = time, 11n compartment-major).
 * Synchronous. */
int sepaihrd_eval_batch(sepaihrd_ctx *ctx, const double *theta, int B, double *loglik,
                        int32_t *status, int32_t *n_accept, int32_t *n_reject, double *ll_parts,
                        double *traj);

/* The same evaluation in two halves: begin uploads theta and launches on a stream of the context's own and returns
 * at once; end waits and downloads (any output may be NULL; no trajectory output in this form).  One begin per
 * context at a time.  For callers that hold several contexts and want their evaluations in flight together -- the
 * finite-difference objective runs its centre value and its P perturbed simulations this way. */
int sepaihrd_eval_batch_begin(sepaihrd_ctx *ctx, const double *theta, int B);
int sepaihrd_eval_batch_end(sepaihrd_ctx *ctx, double *loglik, int32_t *status, int32_t *n_accept, int32_t *n_reject,
                            double *ll_parts);

/* Forward-difference gradients of C parameter vectors in one pass (additive entry; the ABI version is unchanged).
 * For every row c the result is, bit for bit, what the host's finite-difference objective computes for theta[c] alone:
 *   value[c]   the objective at theta[c], evaluated by centre_ctx (which applies its own initial-state rule, by default
 *              SEPAIHRD_INIT_FROM_THETA: run-up / seed);
 *   grad[c][i] (f_i - value[c]) / eps_i with eps_i = fd_epsilon * max(|theta[c][i]|, fd_epsilon) -- a product rounded on
 *              its own, in either arithmetic mode, before it is added to theta[c][i] and before it divides (IEEE fp64
 *              division) -- and f_i the objective at theta[c] + eps_i e_i, evaluated by perturbed_ctx (the caller builds
 *              that context with SEPAIHRD_INIT_MULTIPLIERS, clamp mode, unbounded multipliers and base multipliers 1.0);
 *              0 where f_i is not finite; 0 where the perturbed initial state is invalid: for some age class k the sum over
 *              the compartments E..D of initial_state * multiplier lies outside [0, N_k], the multiplier of compartment j
 *              read UNCONSTRAINED from the perturbed vector at mult_index[j] (-1: not calibrated, 1.0);
 *              the whole row 0 where value[c] is not finite (lowest() is finite);
 *   status[c]  the largest per-evaluation status among the centre's and the row's P perturbed evaluations: the caller
 *              applies its rule for integration failures (>= SEPAIHRD_STATUS_STEP_FAILURE) to it.
 * want_grad (NULL = every row): rows with want_grad[c] == 0 get value[c] and the centre's status only; their rows of
 * `grad` are left untouched and no perturbed evaluation is run for them.
 * What stays with the caller: the rule for output grids with run-up rows (every quotient then uses lowest() for f_i and no
 * perturbed evaluation is needed: call with want_grad all zero) and the refusal of grids that start before t = 0.
 * The G P perturbed evaluations (G = rows wanted) run on perturbed_ctx's own stream and the C centre evaluations on
 * centre_ctx's, ordered by events; the call waits once, for the results.  Workspace: C P P + 2 C P doubles (perturbed
 * matrix, steps, perturbed values) plus the staging of inputs and results (2 C P + C doubles, C P + 3 C int32), held by
 * perturbed_ctx, grown on demand and kept.  All pointers are host pointers; theta [C][P], grad [C][P], mult_index [8].
 * Limits: C * n_params <= 2^22 (4 194 304 perturbed rows; 2.1 GB of workspace at 62 parameters) -- beyond it
 * SEPAIHRD_E_UNSUPPORTED, as for a context in SEPAIHRD_PRECISION_F32; both contexts on one device, of one problem, neither
 * with a sepaihrd_eval_batch_begin pending (SEPAIHRD_E_INVALID_ARG).  Errors are reported through perturbed_ctx. */
int sepaihrd_fd_gradient_batch(sepaihrd_ctx *centre_ctx, sepaihrd_ctx *perturbed_ctx, const double *theta,
                               const uint8_t *want_grad, int C, double fd_epsilon, const int32_t *mult_index,
                               double *value, double *grad, int32_t *status);

/* Device-pointer form: same arguments but every pointer is a DEVICE pointer on ctx's device,
 * and the launches (integrator kernel + two likelihood-pass kernels) are asynchronous on `stream`
 * (a hipStream_t, NULL = default stream).  No synchronisation.  The ctx-owned workspace
 * (D, CumH, CumICU of every chain at every output: T*3*n*8 bytes per chain) grows on the first call
 * for a larger batch; call sepaihrd_reserve first when the call must not allocate (stream capture).
 * Batches whose workspace would exceed 24 GiB (environment SEPAIHRD_WORKSPACE_MB at sepaihrd_create
 * overrides the budget) are evaluated in chunks of chains on the same stream. */
/* A context is single-thread and holds ONE evaluation in flight: the launches of every entry point of a context
 * share its workspace.  Calls on different streams are ordered by the library (the later launch waits for an event
 * the earlier one left, hipStreamWaitEvent: nothing blocks on the host and nothing is added when the stream is the
 * same); for evaluations that should overlap use one context per stream, as the grouped sampler and the
 * finite-difference objective do.  Under stream capture the library records no event: a captured graph must not run
 * concurrently with other launches of the same context. */
int sepaihrd_eval_batch_device(sepaihrd_ctx *ctx, const double *d_theta, int B, double *d_loglik,
                               int32_t *d_status, int32_t *d_n_accept, int32_t *d_n_reject,
                               double *d_ll_parts, double *d_traj, void *stream);

/* Per-kernel timing for benchmarks: while enabled every eval_batch_device launch (enable = 1) or every enable-th one
 * (enable > 1: three event records cost ~15 us of stream time per launch, 2.4 % of a 4096-chain step) is bracketed by HIP
 * events on its stream (before the integrator kernel, after it, after the likelihood pass).
 * sepaihrd_get_timing synchronises on them, returns the summed milliseconds of the integrator kernel
 * and of the likelihood pass over the launches since the last call, and resets the counters. */
int sepaihrd_set_timing(sepaihrd_ctx *ctx, int enable);
int sepaihrd_get_timing(sepaihrd_ctx *ctx, double *integrator_ms, double *likelihood_ms, int *launches);

/* Pre-allocate the workspace for batches of up to max_B chains. */
int sepaihrd_reserve(sepaihrd_ctx *ctx, int max_B);

/* ---- posterior ensemble (second consumer of the integrator) ----
 *
 * sepaihrd_set_initial_state_mode: SEPAIHRD_INIT_FROM_THETA (default) derives x(t0) from theta as
 * SEPAIHRDObjectiveFunction::calculate does (run-up / multiplier branch, S by subtraction,
 * src/model/objectives/SEPAIHRDObjectiveFunction.cpp:124-163); SEPAIHRD_INIT_FIXED integrates every
 * theta from problem.initial_state exactly as given, which is what
 * SimulationRunner::runSimulation(params, initial_state, time_points) does for the post-calibration
 * ensemble (src/model/SimulationRunner.cpp:24-104).
 *
 * sepaihrd_ensemble_quantiles: one simulation per posterior sample theta[s] (S x n_params, host),
 * then, for every output time t >= 0 and age class, the quantiles across samples of
 *   series 0..2  daily hospitalisations / ICU admissions / deaths  max(0, X(t) - X(t_prev))
 *   series 3..5  their running sums in time order
 * (ResultAggregator::aggregatePosteriorPredictives, src/model/ResultAggregator.cpp:297-345) and, if
 * sero_quantiles != NULL, of the seroprevalence (sum N - sum_a S_a(t)) / sum N at EVERY output time
 * (MetricsCalculator::calculateSeroprevalenceTrajectory, src/model/MetricsCalculator.cpp:199-226) and, if
 * rt_quantiles != NULL, of the effective reproduction number at every output time: the spectral radius of
 * the next-generation matrix F V^-1 over (E, P, A, I) x age built from S(t), beta(t), kappa(t)
 * (MetricsCalculator::calculateRtTrajectory :172-197, ReproductionNumberCalculator::calculateRt
 * src/model/ReproductionNumberCalculator.cpp:55-92,158-171), at most 16 age classes.
 * Quantile rule = exact sort + linear interpolation at q (n_valid - 1)
 * (PostCalibrationAnalyser.cpp:303-340); samples whose integration failed are skipped like the
 * reference's `if (!sim_result.isValid()) continue`.
 *   ppc_quantiles   [6][n_probs][T_pos][n_age]   T_pos = number of output times >= 0
 *   sero_quantiles  [n_probs][n_times] or NULL;  rt_quantiles  [n_probs][n_times] or NULL
 *   metrics         [S][12 + 4 n_age] or NULL: the per-sample table of MetricsCalculator::calculateEssentialMetrics
 *                   (src/model/MetricsCalculator.cpp:8-170) -- R0, overall_IFR, overall_attack_rate, peak_hospital,
 *                   peak_ICU, time_to_peak_hospital, time_to_peak_ICU, total_deaths, max_Rt, min_Rt, final_Rt,
 *                   seroprevalence at the output time closest to day 64, then per age IFR, IHR, IICUR, attack rate;
 *                   NaN rows for skipped samples
 *   status          [S] integrator status per sample, or NULL;  n_valid: count of status 0, or NULL
 * Up to 16384 samples a segment is sorted in LDS; larger ensembles sort their segments in global memory
 * (library segmented radix sort), sized only by HBM: 6 T_pos n_age + 2 n_times segments of S doubles. */
#define SEPAIHRD_INIT_FROM_THETA 0
#define SEPAIHRD_INIT_FIXED 1
/* the finite-difference objective's rule (SEPAIHRDGradientObjectiveFunction.cpp:55-99): always scale
 * problem.initial_state by the multipliers, S by subtraction, invalid when the non-S total exceeds N or is negative */
#define SEPAIHRD_INIT_MULTIPLIERS 2
int sepaihrd_set_initial_state_mode(sepaihrd_ctx *ctx, int mode);
int sepaihrd_ensemble_quantiles(sepaihrd_ctx *ctx, const double *theta, int S, const double *probs,
                                int n_probs, double *ppc_quantiles, double *sero_quantiles,
                                double *rt_quantiles, double *metrics, int32_t *status, int32_t *n_valid);

/* sepaihrd_scenario_ensemble: NPI scenario analysis over a posterior ensemble -- every sample theta[s] (S x n_params,
 * host) under each of K scenarios, in ONE integrator launch of K x S chains.  Scenario k integrates with
 * kappa_values[i] * kappa_mult[k n_kappa + i] (K x n_kappa, host; n_kappa must equal the problem's kappa count;
 * finite and >= 0), the multiplier applied on the device AFTER the constraints, as
 * PostCalibrationAnalyser::performScenarioAnalysis scales the already-constrained parameters
 * (src/model/PostCalibrationAnalyser.cpp:94-141).  Only the integration sees the scaled kappa: R0, Rt and the
 * attack-rate accumulation of the metric table read the unscaled kappa, as the reference's metrics, computed through
 * the template's NPI strategy, do (:163-168).  Per scenario, the outputs of sepaihrd_ensemble_quantiles stacked on a
 * leading scenario axis, and over the metric table:
 *   ppc_quantiles   [K][6][n_probs][T_pos][n_age] or NULL
 *   sero_quantiles  [K][n_probs][n_times] or NULL;  rt_quantiles  [K][n_probs][n_times] or NULL
 *   metrics         [K][S][12 + 4 n_age] or NULL (NaN rows for failed samples)
 *   metric_summary  [K][12 + 4 n_age][2 + n_probs] or NULL: mean, population std_dev, then the quantiles of each column
 *                   over the scenario's valid samples (HipPosteriorEnsemble::aggregateMetrics' rule)
 *   diff_quantiles  [K][12 + 4 n_age][n_probs] or NULL: quantiles of the paired differences metric[k][s] - metric[0][s]
 *                   over the samples valid in both scenario k and scenario 0 (e.g. deaths averted = -total_deaths diff)
 *   status          [K][S] or NULL;  n_valid [K] or NULL
 * Same quantile rule as sepaihrd_ensemble_quantiles (exact sort in LDS up to 16384 samples, global segmented sort
 * beyond).  K = 1 with all multipliers 1 reproduces sepaihrd_ensemble_quantiles bit for bit.
 * SEPAIHRD_E_INVALID_ARG for a bad multiplier table, a pending sepaihrd_eval_batch_begin or K x S beyond one launch:
 * more chains than a 32-bit count holds, or more device memory than the device has (the K S trajectories,
 * K S n_times 11 n_age doubles, dominate); SEPAIHRD_E_UNSUPPORTED in F32 or beyond 16 age classes.  A request that fits the
 * device but not its free memory fails with SEPAIHRD_E_HIP ("device allocation failed"). */
int sepaihrd_scenario_ensemble(sepaihrd_ctx *ctx, const double *theta, int S, const double *kappa_mult, int K,
                               int n_kappa, const double *probs, int n_probs, double *ppc_quantiles,
                               double *sero_quantiles, double *rt_quantiles, double *metrics,
                               double *metric_summary, double *diff_quantiles, int32_t *status, int32_t *n_valid);

/* ---- Adaptive-Metropolis chains with their state resident on the device ----
 *
 * MetropolisHastingsSampler (src/sir_age_structured/optimizers/MetropolisHastingsSampler.cpp:201-412)
 * keeps per chain: current state, proposal covariance and its Cholesky factor, running mean and the
 * whole chain history, from which the covariance is recomputed every adaptation period (:168-199,
 * O(t P^2) per refresh, t P doubles of history).  For C lock-step chains that state and that work live next to the
 * likelihood kernel -- but not the whole history: at the reference's own settings (100 000 iterations,
 * adaptation_period 100, data/configuration/mcmc_settings.txt) the walk over the history, not the likelihood,
 * would set the pace, and 4096 x 100 000 x 62 doubles are 203 GB.  The history is read in three places only
 * (its newest state :157, all of it :168-199, every thinning-th state :357-360), so the sampler keeps
 *   - a ring of the newest `adaptation_window` states (queued updates read it),
 *   - running sums of ALL states: their plain sum, added in the order of the reference's mean loop (:171-174: the
 *     refreshed running mean is the reference's bit for bit), and Welford's centred second moment
 *       n-th state x, d = x - mean:   m2_ij += ((n-1)/n) (d_i d_j),   mean_i += d_i (1/n)
 *     from which a refresh is cov = scaling m2 / (len - 1) + eps I in O(P^2) whatever len is (the reference forms the
 *     same matrix as centered^T centered through Eigen's GEMM, whose summation order nothing in its tree pins),
 *   - the thinned samples.
 * SEPAIHRD_MH_COV_TWO_PASS keeps every state in the ring and refreshes with the reference's two literal passes, for
 * comparison (the two covariances agree to ~1e-13 relative; the oracle restates both).
 * The caller keeps what must stay serial per chain: the std::mt19937 stream (its draw order depends on the accept
 * test) and the scalar scale adaptation.  Every sum runs in a fixed order without contraction: a host loop doing
 * the same arithmetic gets the same bits.
 *
 *   create    x0 [C][P] host; cov0 [P][P] row-major host = the initial covariance of EVERY chain,
 *             regularisation already added (:219-237); its Cholesky factor is taken on the device,
 *             0.1 I when it is not positive definite (:240-246); state 0 = x0, mean = x0.
 *   evaluate_current  log-likelihood of the current states (:257)
 *   propose   prop = applyConstraints(x + scale_c L_c z_c) for every chain, evaluated: z [C][P], scale [C],
 *             loglik [C], status [C] (nullable) host (:91-102,309-312).  loglik == NULL only launches: the
 *             caller overlaps its own work with the evaluation and collects the values with fetch
 *   commit    accept [C] host (bit 0 = accepted, bit 1 = best state of the chain so far): x <- prop where bit 0 is
 *             set, the state joins the ring and, every thinning-th one, the samples (:332-371)
 *   adapt     rank-one update (:154-166) with gamma, reading the NEWEST state (the last one committed); updates are
 *             queued with the state they read and applied in order when the covariance is next looked at, so any
 *             pattern of commit / adapt calls gives what immediate updates would.  refresh != 0: the
 *             adaptation-period step (:283-301): full recompute when recompute_full != 0 (caller checks
 *             history >= P + 10), then the Cholesky factor of cov + eps I, kept on success
 *   read_history   states still among the newest `window`, [C][n_rows][P];  read_samples  the thinned samples
 *             first .. first + count - 1, [C][count][P];  read_covariance  [C][P][P];  read_moments  Welford mean [C][P]
 *             and centred second moment [C][P][P] (entries j <= i) of all states so far
 *   summary_records   SURVEY 8(e)'s per-chain record [P means | P variances | best value | accepted proposals] over the
 *             samples first_sample .. (ResultAggregator.cpp:35-172 works on such per-chain / per-batch summaries):
 *             out [C][2 P + 2] host and / or d_out, the same on the device (for a collective); needs the accept test
 *             on the device (step_tested), which tracks best value and accept count
 * P <= 200 (the factorisation keeps a packed lower triangle in LDS).  A sampler object borrows its context: destroy it before the context, and use one sampler per
 * context at a time (it evaluates through the context's workspace on its own stream). */
#define SEPAIHRD_MH_COV_RUNNING 0   /* covariance refresh from running co-moments: O(P^2), no history */
#define SEPAIHRD_MH_COV_TWO_PASS 1  /* recomputeFullCovariance as written: two passes over every state of the chain */
typedef struct sepaihrd_mh_config {
    int32_t chains;            /* C */
    int32_t iterations;        /* states a chain will commit, state 0 included (mcmc_iterations) */
    int32_t thinning;          /* states t with t % thinning == 0 are kept as samples (:357); <= 0: no samples kept */
    int32_t adaptation_window; /* ring of newest states per chain; >= the adaptation period keeps every catch-up on the
                                  refresh itself (smaller only costs extra launches); <= 0: 128 */
    int32_t covariance_mode;   /* SEPAIHRD_MH_COV_* */
    int32_t reserved;          /* 0 */
    double reg_eps;            /* regularization_epsilon */
    double scaling_factor;     /* 2.38^2 / P */
} sepaihrd_mh_config;
typedef struct sepaihrd_mh sepaihrd_mh;
sepaihrd_mh *sepaihrd_mh_create(sepaihrd_ctx *ctx, const sepaihrd_mh_config *config, const double *x0, const double *cov0);
void sepaihrd_mh_destroy(sepaihrd_mh *mh);
int sepaihrd_mh_evaluate_current(sepaihrd_mh *mh, double *loglik, int32_t *status);
int sepaihrd_mh_propose(sepaihrd_mh *mh, const double *z, const double *scale, double *loglik, int32_t *status);
int sepaihrd_mh_fetch(sepaihrd_mh *mh, double *loglik, int32_t *status);
/* The iteration as ONE call, for callers that prepare the next proposal while the device evaluates this one:
 *   stage_normals  z [C][P] host: the NEXT proposal's normals, copied to a second device buffer on a copy stream
 *                  (call it while an evaluation is in flight; double-buffered, one staging per step)
 *   step           accept [C] of the iteration just decided (NULL before the first proposal: nothing to commit),
 *                  scale [C], and n_patch rows of the staged normals to replace (chains whose accept test took the
 *                  branch the staged draw did not assume: patch_chain [n] lists them, patch_z is a full [C][P] array of
 *                  which only the listed chains' rows are read); one packed upload, then
 *                  commit -> adapt (0 none, 1 rank-one update with gamma, 2 + Cholesky refresh, 3 + full two-pass
 *                  recompute before it) -> propose from the staged normals -> evaluation launch.  Returns at once;
 *                  collect the values with sepaihrd_mh_fetch. */
int sepaihrd_mh_stage_normals(sepaihrd_mh *mh, const double *z);
/* page-locked [C][P] host buffer of the sampler to draw the next normals into (two alternate: staging from it is an
 * asynchronous DMA, and the buffer returned after a staging is the other one) */
double *sepaihrd_mh_staging_buffer(sepaihrd_mh *mh);
int sepaihrd_mh_step(sepaihrd_mh *mh, const uint8_t *accept, const double *scale, const int32_t *patch_chain,
                     const double *patch_z, int n_patch, double gamma, int adapt);
/* The iteration with the accept test ON THE DEVICE (MetropolisHastingsSampler.cpp:318-331), so that nothing of the host
 * stands between one evaluation and the next.  While proposal t is being evaluated the caller fills
 *   test_buffer    page-locked doubles [log_u C][scale_reject C][scale_accept C][z_plain C*P]: the log of the uniform the
 *                  test would draw (from the chain's stream), the scale of the NEXT proposal for either outcome of the
 *                  test, and the next proposal's normals for the continuation that draws NO uniform (log_ratio >= 0);
 *   stage_normals  (as above) the next proposal's normals for the continuation that DOES draw it;
 * and calls
 *   step_tested    upload (copy stream, at once) -> [when evaluation t is done] test of every chain against its current
 *                  value (safeEvaluate's rule for failed / non-finite values, :65-74) -> commit -> adapt -> proposal t + 1
 *                  with the normals of the continuation taken and the scale selected -> evaluation t + 1.  last != 0:
 *                  test and commit only.  Returns at once;
 *   fetch_test     waits for THAT test: the values it compared [C] and flags [C] (bit 0 accepted, bit 1 best value of
 *                  the chain so far -- the device keeps the best states --, bit 2 no uniform was drawn): the caller's
 *                  bookkeeping for iteration t then runs while evaluation t + 1 does.  One test in flight at a time.
 *   set_values     the chains' current values before the first test (the values of x0). */
int sepaihrd_mh_set_values(sepaihrd_mh *mh, const double *values);
/* The chains' random streams ON THE DEVICE.  The reference draws from one std::mt19937 per chain: the normals of a proposal
 * (std::normal_distribution: polar method over generate_canonical<double, 53>, sqrt(-2 log(r2) / r2)) and, only when
 * log_ratio < 0, one uniform whose std::log the accept test compares (MetropolisHastingsSampler.cpp:93-97,327).  Drawn on the
 * host these set the pace at BASELINE chain counts (16 host threads: ~6.7 M proposals/s whatever the batch).  Every step of
 * that recipe is integer arithmetic or a correctly rounded IEEE operation except std::log, and glibc's log is written out
 * for the device (csrc/sepaihrd_rng.inc: bit-identical to the libm of this image on a CPU with FMA), so the device draws
 * the SAME values from the SAME stream positions:
 *   seed_streams  chain c gets std::mt19937(seed0 + c); from then on step_tested draws log(u) and the normals of both
 *                 continuations itself (the caller fills only the two scale candidates of the test buffer) and the stream
 *                 moves by what the continuation taken used;
 *   draw_first    the normals of proposal 1 from the start of every stream, staged for sepaihrd_mh_step. */
int sepaihrd_mh_seed_streams(sepaihrd_mh *mh, uint32_t seed0);
/* The device's log and exp restate ONE libm build (glibc 2.35, x86-64, the FMA ifunc variants).  On a host with another
 * glibc, or a CPU without FMA, the last bit may differ and device-drawn streams would silently stop being the host's.
 * device_libm_check evaluates both device functions on 4096 fixed arguments (the sampler's own ranges, the near-1 branch of
 * log, tiny arguments; log_scale_'s clamp range and beyond for exp) and compares them bit for bit with this process's
 * std::log / std::exp: the counts of differing arguments (0 / 0 = safe), computed once per context.  seed_streams and
 * keep_scale_on_device run it themselves and return SEPAIHRD_E_UNSUPPORTED on a difference; the C++ sampler then keeps
 * draws and scale adaptation on the host (MultiChainMetropolisHastings::deviceStreamsFellBack()).
 * Environment SEPAIHRD_LIBM_SELFCHECK=fail makes the check report a difference (test hook for that fall-back). */
int sepaihrd_device_libm_check(sepaihrd_ctx *ctx, int32_t *n_log_diff, int32_t *n_exp_diff);
/* The log of the Poisson term (SEPAIHRDObjectiveFunction.cpp:264-276 calls std::log) evaluated by the device on n host-resident
 * arguments x > 0, normal numbers: the table path of glibc's log on the same constants -- std::log's bits outside
 * [1 - 2^-4, 1 + 0x1.09p-4), within 1e-17 absolute inside.  Diagnostic for the parity tests; no evaluation path calls it. */
int sepaihrd_device_log_values(sepaihrd_ctx *ctx, const double *x, int32_t n, double *out);
int sepaihrd_mh_draw_first(sepaihrd_mh *mh);
/* ... and the scalar scale adaptation: adaptGlobalScale (MetropolisHastingsSampler.cpp:104-152; log_scale_, the window of the
 * last 1000 accept flags, the emergency branches, global_scale_ = std::exp(log_scale_) with glibc's exp written out like its
 * log) runs in the test kernel.  With the streams seeded too the sampler is SELF-CONTAINED: sepaihrd_mh_step_tested takes
 * nothing from the caller (the test buffer is not read, no outcome is sent back per iteration, a pending test is not an
 * error), so the caller can queue iterations as far ahead as it likes and the device goes from one evaluation to the next
 * whatever the host is doing.  What the caller used to keep is kept here and read at the end:
 *   keep_scale_on_device  adapt_scale / target_rate: the reference's settings; keep_trace != 0: the accept flag of every test
 *   read_run_state        current values, best values, scales, accepted proposals, emergency shrinks per chain (any may be NULL)
 *   read_sample_values    the chain's value at every stored sample (sampleObjectiveValues), [C][count]
 *   read_accept_trace     [iterations - 1][C] bytes */
int sepaihrd_mh_keep_scale_on_device(sepaihrd_mh *mh, int adapt_scale, double target_rate, int keep_trace);
int sepaihrd_mh_read_run_state(sepaihrd_mh *mh, double *values, double *best_values, double *scales, int32_t *accepted,
                               int32_t *emergency);
int sepaihrd_mh_read_sample_values(sepaihrd_mh *mh, int first, int count, double *out);
/* Progress reports and checkpoints WITHOUT draining the queue of a self-contained sampler.  The reference reports every
 * report_interval iterations -- LogPost, Best, AccRate, Scale -- and rewrites posterior_trace_checkpoint.csv with the chain's
 * last <= 5000 thinned samples (MetropolisHastingsSampler.cpp:363-383,440-469).
 *   snapshot_begin  call it right behind the sepaihrd_mh_step_tested of the iteration to report: for the n listed chains a
 *                   gather (on the sampler's stream: the values are that iteration's) of [value, best value, scale, accepted
 *                   proposals] and of samples first_sample .. first_sample + count - 1 with their values, then the copy to the
 *                   host on a stream of its own.  Returns at once; the run goes on.  One snapshot in flight at a time.
 *   snapshot_end    wait != 0: blocks until it has landed; wait == 0: returns 1 while it has not.  0: state [n][4],
 *                   samples [n][count][P], sample_values [n][count] are filled (any may be NULL).  May be called from another
 *                   host thread than the one that queues the iterations. */
int sepaihrd_mh_snapshot_begin(sepaihrd_mh *mh, const int32_t *chains, int n, int first_sample, int count);
int sepaihrd_mh_snapshot_end(sepaihrd_mh *mh, int wait, double *state, double *samples, double *sample_values);
/* evaluations the accept test saw FAIL, whole sampler: counts[0] status 2 (500 rejections), [1] status 3 (attempt budget),
 * [2] status 4 (SEPAIHRD_STATUS_PIPELINE).  They enter the test as -1e18 like a throwing objective and would otherwise look
 * like ordinary rejections; a non-zero PIPELINE count is a defect of this build, not of the model. */
int sepaihrd_mh_read_failure_counts(sepaihrd_mh *mh, int64_t counts[3]);
int sepaihrd_mh_read_accept_trace(sepaihrd_mh *mh, uint8_t *out);
double *sepaihrd_mh_test_buffer(sepaihrd_mh *mh);
int sepaihrd_mh_step_tested(sepaihrd_mh *mh, double gamma, int adapt, int last);
int sepaihrd_mh_fetch_test(sepaihrd_mh *mh, double *values, uint8_t *flags);
int sepaihrd_mh_commit(sepaihrd_mh *mh, const uint8_t *accept);
int sepaihrd_mh_adapt(sepaihrd_mh *mh, double gamma, int refresh, int recompute_full);
int sepaihrd_mh_read_history(sepaihrd_mh *mh, const int32_t *rows, int n_rows, double *out);
int sepaihrd_mh_sample_count(const sepaihrd_mh *mh);
int sepaihrd_mh_read_samples(sepaihrd_mh *mh, int first, int count, double *out);
int sepaihrd_mh_read_covariance(sepaihrd_mh *mh, double *cov);
int sepaihrd_mh_read_moments(sepaihrd_mh *mh, double *mean, double *m2);
int sepaihrd_mh_summary_records(sepaihrd_mh *mh, int first_sample, double *out, double *d_out);
/* commit / step read the accept byte as bit 0 = accepted, bit 1 = "this proposal is the chain's best state so far"
 * (the caller's bookkeeping): the best states are kept on the device, [C][P], initially x0 */
int sepaihrd_mh_read_best(sepaihrd_mh *mh, double *best);
/* 1 while launches of this sampler are still running (hipStreamQuery, no wait): lets the caller use the time */
int sepaihrd_mh_busy(sepaihrd_mh *mh);
/* the constrained proposals of the last propose call, [C][P] (callers that track the best state) */
int sepaihrd_mh_read_proposal(sepaihrd_mh *mh, double *prop);
int sepaihrd_mh_history_length(const sepaihrd_mh *mh);

/* ---- Convergence diagnostics of C chains x N draws ----
 *
 * The reference runs one chain and reports none.  Here, per column (a parameter, or the chains' log-likelihood values):
 * the rank-normalised split R-hat and the bulk / tail effective sample sizes of Vehtari, Gelman, Simpson, Carpenter,
 * Buerkner (2021), as the R package `posterior` (1.x) computes them: each chain split into its first and last floor(N/2)
 * draws (odd N: the middle draw dropped), ranks over all split draws with ties averaged, z = Phi^-1((r - 3/8) / (S + 1/4)),
 * folded draws |x - median|, Geyer's initial positive and monotone sequences over direct-sum autocovariances.  A row is
 *   mean, sd (over all C N draws, n - 1), mcse_mean = sd / sqrt(ess_mean), ess_mean (raw split draws), ess_bulk (their z),
 *   ess_tail = min(ESS of I[x <= q05], ESS of I[x <= q95]) (type-7 quantiles of all C N draws), r_hat = max(R(z), R(z folded))
 * and is all NaN when a draw is non-finite or max - min < DBL_EPSILON (posterior's should_return_NA; the same rule makes
 * one series NaN, e.g. a tail indicator that is constant).  ESS is NaN for floor(N/2) < 3.  Every sum runs in a fixed order:
 * the table has the same bits from call to call and through both entry points.  Ranks come from rocPRIM's segmented radix
 * sort on the device, autocovariances in blocks of 64 lags up to Geyer's truncation (one 4-byte read-back per block).
 *   chain_diagnostics   samples [C][N][P] host, values [C][N] host or NULL -> out [P + (values != NULL)][7] host, the values
 *                       row last; max_lag [P + 1][4] or NULL: Geyer's max_t of the raw, z, I05 and I95 series (-1: NaN ESS)
 *   mh_diagnostics      the same over the sampler's RESIDENT thinned samples first_sample .. first_sample + count - 1
 *                       (count <= 0: to the last stored) and, with with_values, the chains' values at them (stored with
 *                       sepaihrd_mh_keep_scale_on_device); nothing is read back but the table
 * SEPAIHRD_E_INVALID_ARG (sepaihrd_last_error says which) for C < 1, P < 1 or N < 4, C N >= 2^31, a range beyond the stored
 * samples, a sampler that stores no samples, with_values without stored values, or a pending sepaihrd_eval_batch_begin. */
#define SEPAIHRD_DIAG_COLUMNS 7 /* mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, r_hat */
int sepaihrd_chain_diagnostics(sepaihrd_ctx *ctx, const double *samples, const double *values, int C, int N, int P,
                               double *out, int32_t *max_lag);
int sepaihrd_mh_diagnostics(sepaihrd_mh *mh, int first_sample, int count, int with_values, double *out, int32_t *max_lag);

/* ---- per-chain summary records across devices (the one exchange of the path) ----
 *
 * After sampling, the post-calibration summary needs the records of ALL chains -- [P posterior means | P variances |
 * best value | accepted proposals] per chain, what sepaihrd_mh_summary_records writes -- the way the reference forms
 * its ensemble statistics serially in ResultAggregator::aggregateBatchMetrics / aggregateAllBatches
 * (src/model/ResultAggregator.cpp:35-172).  One process drives several devices (one context per device, one host
 * thread each: MultiChainMetropolisHastings::optimizeChainGroupsOnDevice), so the collective is RCCL's single-process
 * form: ncclCommInitAll over the contexts' devices, one ncclAllGather per device in a group call, over xGMI.
 *   records_buffer   a device buffer owned by the context (grown on demand, freed with it): which = 0 the table of the chains
 *                    this context ran (pass it to sepaihrd_mh_summary_records as d_out), which = 1 the gathered table
 *   allgather_records  rows[k] records of `width` doubles from every context's buffer 0 into EVERY context's buffer 1, in
 *                    context order.  backend AUTO: RCCL when librccl can be loaded (dlopen at first use: no link-time
 *                    dependency) and no two contexts share a device, else staging through the host; RCCL / HOST force one
 *                    (RCCL with two contexts on one device: SEPAIHRD_E_UNSUPPORTED).  *backend_used says which ran.
 *   read_records / write_records   a context's buffer to / from the host (write grows it) */
#define SEPAIHRD_GATHER_AUTO 0
#define SEPAIHRD_GATHER_RCCL 1
#define SEPAIHRD_GATHER_HOST 2
double *sepaihrd_records_buffer(sepaihrd_ctx *ctx, int which, size_t doubles);
int sepaihrd_allgather_records(sepaihrd_ctx *const *ctxs, int n, const int32_t *rows, int width, int backend,
                               int *backend_used);
int sepaihrd_read_records(sepaihrd_ctx *ctx, int which, double *out, size_t doubles);
int sepaihrd_write_records(sepaihrd_ctx *ctx, int which, const double *in, size_t doubles);

/* applyConstraints for B vectors on the host (exactly the device's arithmetic). */
int sepaihrd_apply_constraints(const sepaihrd_ctx *ctx, int mode, const double *in, int B, double *out);

/* Launch geometry / resource report of the evaluation kernel the ctx will use. */
#define SEPAIHRD_LL_INLINE 0          /* three logs per output inside the integrating wave; nothing parked */
#define SEPAIHRD_LL_SEPARATE_PASS 1   /* daily increments parked in the ctx workspace (T 3 n 8 B per evaluation), two kernels after */
#define SEPAIHRD_LL_CONSUMER_WAVES 2  /* a second wave of the integrator's SIMD, fed through LDS; nothing parked */
typedef struct sepaihrd_kernel_info {
    int32_t lanes_per_chain;   /* n rounded up to a power of two */
    int32_t chains_per_wave;
    int32_t block_threads;
    int32_t vgprs, sgprs, lds_bytes, scratch_bytes;
    int32_t max_blocks_per_cu; /* occupancy query */
    int32_t num_cus;
    int32_t likelihood_form;   /* SEPAIHRD_LL_*: where the Poisson terms of such a launch are evaluated */
    int32_t phase_pass_applied; /* 1: the kernel's code went through csrc/phase_pass.py at build time (the instruction-fetch
                                   phase of its RK body is set; worth 1-3 %); 0: the build fell back to the plain compile,
                                   or the kernel (fp32 state) does not use the pass */
    char kernel_name[128];
    char device_name[128];
} sepaihrd_kernel_info;
int sepaihrd_get_kernel_info(sepaihrd_ctx *ctx, sepaihrd_kernel_info *info);
/* The same report for a launch of `batch_chains` chains: batches of up to 4096
 * chains of a 4-age problem are integrated with sixteen lanes per chain (a quad of lanes per age class) instead of four, so that a
 * batch too small to fill the chip still spreads over four times as many SIMDs.  Results are bit-identical between
 * the two forms.  batch_chains <= 0: the large-batch kernel (what sepaihrd_get_kernel_info reports). */
int sepaihrd_get_kernel_info_for_batch(sepaihrd_ctx *ctx, int32_t batch_chains, sepaihrd_kernel_info *info);

/* ------------------------------------------------------------------------------------------------------------------
 * Age-structured SIR model: a batched PoissonLikelihoodObjective::calculate on the device (csrc/sepaihrd_sir.hip,
 * csrc/sepaihrd_sir_capi.cpp).  Additive: nothing above changes, SEPAIHRD_ABI_VERSION stays as it is.
 * Reference behaviour (paths under the reference tree):
 *   right-hand side          src/sir_age_structured/AgeSIRModel.cpp:106-139
 *   model validation         src/sir_age_structured/AgeSIRModel.cpp:66-77 (validate_parameters)
 *   constraints, theta       src/sir_age_structured/parameters/SIRParameterManager.cpp:98-156
 *   incidence                src/sir_age_structured/SimulationResultProcessor.cpp:144-189
 *   objective                src/sir_age_structured/objectives/PoissonLikelihoodObjective.cpp:46-144
 *   grid rules               src/sir_age_structured/Simulator.cpp:60-150
 * Per chain: theta -> max(1e-12, q) / max(0, scale_C_total) / max(0, gamma_i) (no bounds, no reflect mode in this
 * manager; fields that are not calibrated keep the problem's values) -> integrate_times from the FIXED initial_state
 * [S(n), I(n), R(n)] -> at EVERY output time incidence_i = lambda_i(x(t)) S_i(t), sim = max(incidence, 1e-9),
 * obs = max(observed, 0), loglik = sum_t sum_i (obs log(sim) - sim), added in (t, i) row order.
 * Failure convention (differs from the SEPAIHRD objective): this objective catches every exception, so a chain that
 * fails returns -INFINITY (not lowest()) with its status set -- SEPAIHRD_STATUS_INVALID for a non-finite observation,
 * incidence or total, _STEP_FAILURE, _STEP_BUDGET -- and nothing is raised.  A NaN observation counts as non-finite.
 * F64 state only, one lane per (chain, age class), 1 <= n_age <= 64; no quad-lane form.
 * ------------------------------------------------------------------------------------------------------------------ */
#define SEPAIHRD_SIR_NUM_COMPARTMENTS 3 /* S, I, R */
/* param_field codes of sepaihrd_sir_problem */
#define SEPAIHRD_SIR_F_Q 0             /* "q" */
#define SEPAIHRD_SIR_F_SCALE_C_TOTAL 1 /* "scale_C_total" */
#define SEPAIHRD_SIR_F_GAMMA 2         /* "gamma_<i>", i in param_index */

typedef struct sepaihrd_sir_problem {
    int32_t abi_version; /* SEPAIHRD_ABI_VERSION */
    int32_t n_age;       /* n */
    int32_t n_times;     /* T: output times = rows of obs (PoissonLikelihoodObjective.cpp:38-42) */
    int32_t n_params;    /* P */
    int32_t solver;      /* SEPAIHRD_SOLVER_* */
    int32_t arith;       /* SEPAIHRD_ARITH_* */
    int32_t max_attempts; /* step-attempt budget per chain; <= 0: 1000000 */
    int32_t reserved;
    const double *times;         /* [T] strictly increasing */
    const double *N;             /* [n] population sizes, >= 0 */
    const double *C;             /* [n*n] ROW-major baseline contact matrix, entries >= 0 */
    const double *gamma;         /* [n] recovery rates, >= 0 */
    const double *initial_state; /* [3n] S(n), I(n), R(n) */
    const double *obs;           /* [T*n] row-major observed incidence */
    const int32_t *param_field;  /* [P] SEPAIHRD_SIR_F_* */
    const int32_t *param_index;  /* [P] age class of a SEPAIHRD_SIR_F_GAMMA entry, ignored otherwise */
    double q;             /* transmissibility, >= 0 */
    double scale_C_total; /* contact scale factor, >= 0 */
    double abs_err, rel_err, dt_hint;
} sepaihrd_sir_problem;

typedef struct sepaihrd_sir_ctx sepaihrd_sir_ctx;

/* Validates the problem (Simulator::run grid rules; AgeSIRModel::validate_parameters: a negative N / gamma / q / scale / C
 * entry is refused with a message; field codes and gamma indices), uploads it once.  NULL + message on failure; there is no
 * CPU fallback (no device: the message says so).  Validation comes before the device is touched. */
sepaihrd_sir_ctx *sepaihrd_sir_create(const sepaihrd_sir_problem *pb, int device, char *err, int errlen);
void sepaihrd_sir_destroy(sepaihrd_sir_ctx *ctx);
const char *sepaihrd_sir_last_error(const sepaihrd_sir_ctx *ctx);
/* theta [B][P] host; loglik [B]; status / n_accept / n_reject [B] or NULL; traj [B][T][3n] or NULL.  Synchronous. */
int sepaihrd_sir_eval_batch(sepaihrd_sir_ctx *ctx, const double *theta, int B, double *loglik, int32_t *status,
                            int32_t *n_accept, int32_t *n_reject, double *traj);
/* The same on device-resident arrays, asynchronous on `stream` (a hipStream_t, NULL: the default stream); allocates nothing. */
int sepaihrd_sir_eval_batch_device(sepaihrd_sir_ctx *ctx, const double *d_theta, int B, double *d_loglik, int32_t *d_status,
                                   int32_t *d_n_accept, int32_t *d_n_reject, double *d_traj, void *stream);
/* Sizes the staging buffers of sepaihrd_sir_eval_batch for max_B chains ahead of time. */
int sepaihrd_sir_reserve(sepaihrd_sir_ctx *ctx, int max_B);
/* SIRParameterManager::applyConstraints on B host vectors (no device work). */
int sepaihrd_sir_apply_constraints(const sepaihrd_sir_ctx *ctx, const double *in, int B, double *out);
int sepaihrd_sir_set_arith(sepaihrd_sir_ctx *ctx, int arith);

/* ---- the device-resident Adaptive-Metropolis sampler on the SIR objective ----
 * sepaihrd_sir_mh_create returns the SAME opaque sepaihrd_mh as sepaihrd_mh_create: every sepaihrd_mh_* entry point above
 * works on it unchanged (propose / commit / adapt, step, step_tested, seed_streams, keep_scale_on_device, draw_first, the
 * read_* calls, summary_records, snapshot_begin / _end, read_failure_counts, mh_diagnostics, busy).  The errors of such a
 * sampler are read with sepaihrd_sir_last_error(ctx).  Proposals go through SIRParameterManager::applyConstraints
 * (max(1e-12, q), max(0, scale_C_total), max(0, gamma_i)): the kernels' clamp mode with lower = 1e-12 / 0 and upper = +inf
 * (sepaihrd_sir_constraint_bounds), equal to sepaihrd_sir_apply_constraints bit for bit on finite input.  A failed evaluation (-INFINITY with status 1 / 2 / 3) enters
 * the accept test by the rule of every sampler here: status >= 2, NaN or +-inf count as -1e18.  The context must outlive the
 * sampler.  NULL ctx: NULL, no device touched.
 * sepaihrd_sir_device_libm_check is sepaihrd_device_libm_check for a SIR context (same self-check, same
 * SEPAIHRD_LIBM_SELFCHECK=fail hook). */
sepaihrd_mh *sepaihrd_sir_mh_create(sepaihrd_sir_ctx *ctx, const sepaihrd_mh_config *config, const double *x0, const double *cov0);
int sepaihrd_sir_device_libm_check(sepaihrd_sir_ctx *ctx, int32_t *n_log_diff, int32_t *n_exp_diff);
/* The table such a sampler clamps its proposals with, for param_field[n_params] (SEPAIHRD_SIR_F_*): lower = 1e-12 for q and
 * 0 otherwise, upper = +inf; has_bounds (NULL: not wanted) = 1 for q -- clamp(v, lower, upper) -- and 0 otherwise -- the
 * kernels' unbounded clamp (0 < v) ? v : 0, which is std::max(0.0, v) with the sign of a zero.  Host only, no device and
 * no context needed. */
int sepaihrd_sir_constraint_bounds(const int32_t *param_field, int n_params, double *lower, double *upper, int32_t *has_bounds);

/* Which form of the per-iteration sampler kernels (the draws; L z ahead of the test; test + commit + proposal; their unfused
 * siblings) a sampler launches.  BLOCK_PER_CHAIN gives every chain a workgroup of one or two wavefronts (shaped for P = 62); PACKED
 * gives a chain a group of pow2(P) adjacent lanes, 64 / pow2(P) chains per wavefront (P <= 64 only: SEPAIHRD_E_UNSUPPORTED
 * beyond).  The two forms give the same bits: states, proposals, accept flags, scales, stored samples and values.  AUTO is
 * BLOCK_PER_CHAIN on a sampler made by sepaihrd_mh_create whatever P is; on a sepaihrd_sir_mh_create sampler it is whichever
 * form was measured faster for its (P, chains).  May be called between any two iterations.
 * NULL sampler or an unknown code: SEPAIHRD_E_INVALID_ARG, no device touched. */
#define SEPAIHRD_MH_FORM_AUTO 0
#define SEPAIHRD_MH_FORM_BLOCK_PER_CHAIN 1
#define SEPAIHRD_MH_FORM_PACKED 2
int sepaihrd_mh_set_kernel_form(sepaihrd_mh *mh, int form);
/* the form in use (AUTO resolved): SEPAIHRD_MH_FORM_BLOCK_PER_CHAIN or _PACKED; NULL: SEPAIHRD_E_INVALID_ARG */
int sepaihrd_mh_get_kernel_form(const sepaihrd_mh *mh);

/* ---- age-structured SIR: posterior ensemble and intervention scenarios (additive; SEPAIHRD_ABI_VERSION stays) --------------
 * S posterior samples under K intervention scenarios in ONE integrator launch of K x S chains (the ensemble build of
 * csrc/sepaihrd_sir.hip), then per-scenario quantile bands, a per-sample metric table, metric summaries and paired
 * differences against scenario 0.  Full trajectories are never materialised.
 *
 * A scenario is a list of at most SEPAIHRD_SIR_MAX_EVENTS events sorted by time_index (ties apply in listed order);
 * time_index is an index of the problem's output grid times[] -- interventions act on grid times only.  Kinds, after
 * AgeSIRModel::applyIntervention (src/sir_age_structured/AgeSIRModel.cpp:141-173):
 *   SEPAIHRD_SIR_EV_CONTACT       scale_C_total <- scale_C_total * value, value >= 0
 *                                 ("contact_reduction" / "social_distancing" / "lockdown")
 *   SEPAIHRD_SIR_EV_TRANSMISSION  q <- q * (1 - value), 0 <= value <= 1  ("mask_mandate" / "transmission_reduction")
 * Events compound as repeated applyIntervention calls do; after a contact event C_current is re-formed as C_ij * scale (what a
 * model constructed with the new scale_C_total holds).  An event at index k > 0: the chain integrates to times[k] with the old
 * parameters, the row observed there (state and incidence) is formed with the old parameters, then the parameters change
 * and the integrator restarts as a fresh integrate_times call would (dt = dt_hint, no consecutive failures, Dopri5's FSAL
 * derivative recomputed); max_attempts and the step counters run over the whole chain.  An event at index 0 is applied before
 * the first observation (= a plain run with the changed parameters); one at index T - 1 is legal and changes nothing.
 * Scenario 0 may be empty: the baseline. */
#define SEPAIHRD_SIR_MAX_EVENTS 8
#define SEPAIHRD_SIR_EV_CONTACT 0
#define SEPAIHRD_SIR_EV_TRANSMISSION 1
typedef struct sepaihrd_sir_event {
    int32_t time_index, kind;
    double value;
} sepaihrd_sir_event;
/* The check both entry points below run before any device work, host only (no device, no context): events
 * [K][SEPAIHRD_SIR_MAX_EVENTS], n_events [K], n_times = T.  SEPAIHRD_E_INVALID_ARG with a message naming the offending
 * scenario and event in err (NULL: not wanted) for: more than 8 events (or a negative count), a time_index outside [0, T),
 * unsorted events, an unknown kind, a value out of its kind's range or non-finite. */
int sepaihrd_sir_validate_events(const sepaihrd_sir_event *events, const int32_t *n_events, int K, int n_times, char *err, int errlen);
/* theta [S][P] (host).  Every output is host memory and may be NULL:
 *   quantiles      [K][3][n_probs][T][n_age + 1]  series 0 incidence max(q (C_current (I / N))_i, 0) S_i(t) with the
 *                  parameters in force for that row and none of the likelihood's 1e-9 floor
 *                  (SimulationResultProcessor.cpp:144-189), 1 prevalence I_i(t), 2 cumulative infections S_i(t0) - S_i(t);
 *                  column n_age is the age total (ages added in ascending order).  Quantile rule of
 *                  sepaihrd_ensemble_quantiles: exact sort, linear interpolation at q (n_valid - 1), failed samples of
 *                  that scenario skipped, NaN when none is valid
 *   metrics        [K][S][6 + 2 n_age]  0 R0 = spectral radius of K_ij = q scale C_ij N_i / (N_j gamma_j) with the sample's
 *                  parameters before any event (columns with N_j <= 1e-9 dropped, gamma_j = 0: +inf); 1 peak total
 *                  prevalence over the output times, 2 its output time (first maximal row); 3 peak total incidence, 4 its
 *                  output time; 5 overall attack rate sum_i (S_i(t0) - S_i(t_last)) / sum N; then per age: attack rate
 *                  (S_i(t0) - S_i(t_last)) / N_i (0 where N_i <= 0), peak prevalence.  NaN row for a failed sample
 *   metric_summary [K][W][2 + n_probs]  mean, population standard deviation, quantiles (W = 6 + 2 n_age)  } the rules of
 *   diff_quantiles [K][W][n_probs]  quantiles of metric[k][s] - metric[0][s] over samples valid in both     } sepaihrd_scenario_ensemble
 *   status         [K][S]  0, 1 (non-finite incidence), 2 (step failure), 3 (step budget)
 *   n_accept, n_reject [K][S]  step counts over the whole chain
 *   n_valid        [K]
 * K = 1 with no events gives the trajectories of sepaihrd_sir_eval_batch bit for bit.  A failed sample never fails the call.
 * SEPAIHRD_E_INVALID_ARG: a bad event table (sepaihrd_sir_validate_events; the device is not touched), probabilities outside
 * [0, 1], K x S beyond a 32-bit chain count or the device's memory (dominant: K 3 T (n_age + 1) S_pad doubles);
 * SEPAIHRD_E_HIP ("device allocation failed") when it fits the device but not its free memory.  Scratch stays with the
 * context and is reused.  Up to 16384 samples a segment is sorted in LDS, beyond by a segmented radix sort. */
int sepaihrd_sir_scenario_ensemble(sepaihrd_sir_ctx *ctx, const double *theta, int S, const sepaihrd_sir_event *events,
                                   const int32_t *n_events, int K, const double *probs, int n_probs, double *quantiles,
                                   double *metrics, double *metric_summary, double *diff_quantiles, int32_t *status,
                                   int32_t *n_accept, int32_t *n_reject, int32_t *n_valid);
/* K = 1, no events: quantiles [3][n_probs][T][n_age + 1], metrics [S][W], metric_summary [W][2 + n_probs], status [S],
 * n_valid [1] */
int sepaihrd_sir_ensemble_quantiles(sepaihrd_sir_ctx *ctx, const double *theta, int S, const double *probs, int n_probs,
                                    double *quantiles, double *metrics, double *metric_summary, int32_t *status, int32_t *n_valid);
/* Calls of the two entry points above that reached the device on this context (calls, NULL: not wanted) and the device time
 * of the last one in milliseconds (ms[3], NULL: not wanted): integrator; fix-up and metric passes; sorts, quantiles and
 * scenario summaries. */
int sepaihrd_sir_ensemble_timing(const sepaihrd_sir_ctx *ctx, int64_t *calls, double *ms);

/* ---- stochastic chain-binomial SIR ensembles (the reference's StochasticSIRModel, src/base/SIR_stochastic.cpp) ----
 * n_replicates independent replicates of each of n_groups parameter sets, one lane per replicate, the step loop inside the
 * kernel (csrc/sepaihrd_stoch_sir.hip), then per (group, compartment, step) the mean, median, 5 % and 95 % point across the
 * replicates.  No context: each call names its device.
 *
 * One step of one replicate, as the reference takes it (:152-207): S_int = (int)round(S), I_int = (int)round(I); if either
 * is <= 0 the next row is a copy of this one (so recoveries stop too once S reaches 0); otherwise
 * pI = 1 - exp(-(beta I h / N)) with the double I and the group's N, pR = 1 - exp(-gamma h), both clamped to [0, 1],
 * I_new ~ Binomial(S_int, pI) then R_new ~ Binomial(I_int, pR), S' = max(0, S_int - I_new), I' = max(0, I_int + I_new -
 * R_new), R' = max(0, R + R_new).  Row 0 is (S0, I0, R0); steps = (int)round((t_end - t_start) / h) + 1.
 *
 * The random stream is this build's own (the reference seeds one serial generator from the clock): every variate is a
 * function of (seed, group, replicate, step, transition, attempt) through Philox-4x32-10, csrc/sepaihrd_stoch.inc says how.
 * A replicate's path therefore depends on nothing else: not on n_replicates, keep, the launch or max_workspace_bytes. */
typedef struct sepaihrd_stoch_sir_group {
    double N, beta, gamma, S0, I0, R0;
} sepaihrd_stoch_sir_group;
typedef struct sepaihrd_stoch_sir_config {
    int32_t abi_version; /* SEPAIHRD_ABI_VERSION */
    int32_t n_groups, n_replicates;
    int32_t keep; /* replicates 0 .. keep - 1 of every group have their trajectories returned (0 <= keep <= n_replicates) */
    double t_start, t_end, h;
    uint64_t seed;
    /* Device memory the call may hold for trajectories at one time; the time axis is processed in chunks of whole steps
     * that fit (at least one step), the replicates' states carried between chunks.  Same results for every value.
     * 0: SEPAIHRD_STOCH_SIR_DEFAULT_WORKSPACE. */
    uint64_t max_workspace_bytes;
} sepaihrd_stoch_sir_config;
#define SEPAIHRD_STOCH_SIR_DEFAULT_WORKSPACE ((uint64_t)4 << 30) /* 4 GiB */
#define SEPAIHRD_STOCH_SIR_MAX_REPLICATES (1 << 24)
/* number of rows, or a negative code when the arguments give none (h <= 0, t_end <= t_start, not finite, beyond 2^31 - 1) */
int64_t sepaihrd_stoch_sir_num_steps(double t_start, double t_end, double h);
/* Host only.  SEPAIHRD_E_INVALID_ARG with a message in err (NULL: not wanted) unless, for every group: N > 0; beta, gamma,
 * S0, I0, R0 >= 0; |S0 + I0 + R0 - N| <= 1e-6 N (the reference's constructor, :29-34) -- and h > 0, t_end > t_start,
 * n_replicates >= 1.  This build adds, because the compartments are int: everything finite, N <= 2^31 - 1, round(S0) +
 * round(I0) <= 2^31 - 1, steps <= 2^31 - 1; and n_groups in [1, 2^30], n_replicates <= SEPAIHRD_STOCH_SIR_MAX_REPLICATES,
 * keep in [0, n_replicates], abi_version. */
int sepaihrd_stoch_sir_validate(const sepaihrd_stoch_sir_config *config, const sepaihrd_stoch_sir_group *groups, char *err, int errlen);
/* device: a HIP device index, -1 = the current one.  Outputs are host memory:
 *   stats        [n_groups][4][3][steps]  mean, median, 5 %, 95 % of S, I, R across the replicates: ascending sort, the mean by
 *                m += (x_i - m) / (i + 1) over the sorted values, the median the middle value or the mean of the two middle
 *                ones, quantile f as (1 - d) x[lhs] + d x[lhs + 1] with lhs = (int)(f (R - 1)), d its fraction
 *   traj         [n_groups][keep][3][steps], or NULL
 *   final_state  [n_groups][n_replicates][3], or NULL
 *   phase_ms     [3] device time in ms of the step kernels, of the segment sorts and of the summaries (up to 16384
 *                replicates sort and summary are one kernel, counted under the sorts), or NULL
 * Up to 16384 replicates a segment is sorted in LDS, beyond by a segmented radix sort.  Refused arguments
 * (sepaihrd_stoch_sir_validate, a NULL stats) return SEPAIHRD_E_INVALID_ARG before the device is touched. */
int sepaihrd_stoch_sir_run(int device, const sepaihrd_stoch_sir_config *config, const sepaihrd_stoch_sir_group *groups, double *stats,
                           double *traj, double *final_state, double *phase_ms, char *err, int errlen);
/* Probe of the device's sampler: out[i] ~ Binomial(n[i], p[i]), the variate at (seed, group 0, replicate i, step 0,
 * infection).  n [count] >= 0, p [count], out [count], host memory. */
int sepaihrd_stoch_sir_binomial_device(int device, uint64_t seed, const int32_t *n, const double *p, int count, int32_t *out, char *err,
                                       int errlen);

/* ---- posterior predictive draws with Poisson noise (additive; SEPAIHRD_ABI_VERSION stays) ----------------------------------
 * sepaihrd_ensemble_quantiles takes quantiles across samples of the model's EXPECTED daily counts, as
 * ResultAggregator::aggregatePosteriorPredictives does: bands of parameter uncertainty only.  The likelihood treats an
 * observed count as Poisson around that expectation (calculateSingleLogLikelihood: mean max(0, increment) + 1e-10), so the
 * replicated-data check needs y_rep ~ Poisson(mean).  The reference has no such output; this one is this build's own.
 *
 * sepaihrd_ensemble_predictive: one simulation per posterior sample theta[s] (S x n_params, host) as
 * sepaihrd_ensemble_quantiles runs it (same preconditions, initial-state mode and failure codes), then R replicates per sample:
 * for every output time j with t >= 0, age a and daily series k in {0 hospitalisations, 1 ICU admissions, 2 deaths}
 *   m = max(0, increment),  y = Poisson(m + 1e-10) at stream coordinates (seed, c0 = s, c1 = r, c2 = (k T_pos + j) n_age + a)
 * through Philox-4x32-10 and the sampler of csrc/sepaihrd_poisson.inc (inversion below 10, Hoermann's PTRS from 10 on); s is
 * the sample's position in theta.  Series 3..5 are the running sums of y in time order per (s, r, a), exact integers.
 *   pred_quantiles  [6][n_probs][T_pos][n_age]  quantiles over the n_valid R draws of the valid samples; the rule of
 *                   sepaihrd_ensemble_quantiles (exact sort, interpolation at q (count - 1)); sorted in LDS up to 16384 draws
 *                   per segment, by the segmented radix sort beyond
 *   pit             [3][T_pos][n_age] or NULL: the mid-PIT (#{draws < obs} + 0.5 #{draws == obs}) / (n_valid R) of every cell
 *                   of the daily series whose observation is usable (finite and >= 0, the likelihood's rule), NaN elsewhere
 *   means           [S][3][T_pos][n_age] or NULL: m as drawn from; NaN rows for failed samples
 *   draws           [S][R][3][T_pos][n_age] or NULL: the daily y; NaN for failed samples
 *   status          [S] or NULL;  n_valid: count of status 0, or NULL
 * A draw is a function of its coordinates and its mean alone: it does not depend on S, R, the launch, the sort path or on
 * which other samples failed.  The host twin (host/: hostPosteriorPredictive) reproduces draws, quantiles and PIT bit for bit
 * from `means` and `status`.
 * SEPAIHRD_E_INVALID_ARG: R < 1, S R >= 2^31 (or S R rounded up to whole wavefronts), 3 T_pos n_age >= 2^32, a probability
 * outside [0, 1], a pending sepaihrd_eval_batch_begin, or a segment table (6 T_pos n_age segments of S R doubles, plus the
 * optional outputs and the likelihood workspace) beyond the device's memory -- the rule of sepaihrd_scenario_ensemble. */
int sepaihrd_ensemble_predictive(sepaihrd_ctx *ctx, const double *theta, int S, int R, uint64_t seed, const double *probs, int n_probs,
                                 double *pred_quantiles, double *pit, double *means, double *draws, int32_t *status, int32_t *n_valid);
/* Host only: the argument rules above that need no context, with a message in err (NULL: not wanted). */
int sepaihrd_predictive_validate(int S, int R, int T_pos, int n_age, const double *probs, int n_probs, char *err, int errlen);
/* Device time of the context's last sepaihrd_ensemble_predictive, sepaihrd_ensemble_predictive_nb or
 * sepaihrd_ensemble_predictive_scores call in milliseconds, ms[3]: integrator; draws and mid-PIT counts (the scored call has no PIT
 * pass); segment sorts and quantiles (and, in the scored call, the scores).  sepaihrd_ensemble_predictive_targets reports the
 * same three phases over its targets. */
int sepaihrd_predictive_timing(const sepaihrd_ctx *ctx, double *ms);
/* Probe of the device's Poisson sampler: out[i] ~ Poisson(lambda[i]), the variate at (seed, c0 = i, c1 = 0, c2 = 0).
 * lambda [count], out [count], host memory; lambda <= 0 gives 0, NaN and +infinity give NaN. */
int sepaihrd_poisson_device(int device, uint64_t seed, const double *lambda, int count, double *out, char *err, int errlen);

/* ---- posterior predictive draws under the negative-binomial observation model (additive; SEPAIHRD_ABI_VERSION stays) ---------
 * After a calibration under the negative-binomial likelihood (sepaihrd_set_dispersion, SEPAIHRD_F_DISPERSION) the replicated
 * data must carry that model's noise: Poisson replicates give bands that are too narrow, the defect the replicated-data check
 * exists to avoid.  sepaihrd_ensemble_predictive_nb is sepaihrd_ensemble_predictive -- same preconditions, failure codes, memory
 * rule, outputs, stream coordinates, and what the context keeps -- with, for sample s and daily series k,
 *   y = NegativeBinomial(mean m + 1e-10, dispersion k_used[s][k])   (variance mean + mean^2 / k)
 * drawn as a gamma-Poisson mixture by the sampler of csrc/sepaihrd_nb_draw.inc: G ~ Gamma(k) by Cheng's algorithm GB (shape
 * below 1: the boost Gamma(k + 1) U^(1/k)) on the counters (c0, c1, c2, 0x80000000 + attempt) and (c0, c1, c2, 0xC0000000), then
 * Poisson(mean (G / k)) on the Poisson call's own counters.  A series with k = +inf has the Poisson call's draws, bit for bit;
 * with all three at +inf for every sample every output is that call's.
 *   dispersion  NULL: each sample's k is what the deterministic objective would use for that theta -- the constrained theta
 *               entry of a calibrated series, the context's fixed value otherwise.  [3]: these values for every sample, whatever
 *               the context holds; refused with sepaihrd_particle_nb_validate's message where that function refuses
 *   k_used      [S][3] or NULL: the dispersions drawn with.  A sample whose k is NaN (a NaN theta entry) counts as failed:
 *               status 1, no draws
 * The device maps one lane to a (sample, replicate, age, series) and walks its T_pos output times; the host twin
 * (hostPosteriorPredictive with k_used) reproduces draws, quantiles and PIT bit for bit from means, status and k_used.
 * sepaihrd_predictive_timing reports this call when it was the last of the two. */
int sepaihrd_ensemble_predictive_nb(sepaihrd_ctx *ctx, const double *theta, int S, int R, uint64_t seed,
                                    const double *dispersion /* [3] or NULL: the context's */, const double *probs, int n_probs,
                                    double *pred_quantiles, double *pit, double *means, double *draws, double *k_used /* [S][3] or NULL */,
                                    int32_t *status, int32_t *n_valid);
/* Probes of the device's gamma and negative-binomial samplers, host memory: out[i] ~ Gamma(shape[i], 1), and
 * out[i] ~ NegativeBinomial(mu[i], k[i]), the variates at (seed, c0 = i, c1 = 0, c2 = 0).  shape finite in [1e-3, 1e6]; k the
 * same or +inf (Poisson); mu <= 0 gives 0, NaN and +infinity give NaN. */
int sepaihrd_gamma_device(int device, uint64_t seed, const double *shape, int count, double *out, char *err, int errlen);
int sepaihrd_nb_draw_device(int device, uint64_t seed, const double *mu, const double *k, int count, double *out, char *err, int errlen);

/* ---- scores of the posterior predictive draws against data (additive; SEPAIHRD_ABI_VERSION stays) ---------------------------
 * Which observation model predicts the data better, and how well does a fit forecast days it never saw?  Proper scoring rules of
 * the predictive sample against the observation, cell by cell and averaged: CRPS, the interval score of each central interval
 * and their weighted sum (WIS), empirical coverage, the absolute error of the median.  The reference has none; this is this
 * build's own.  sepaihrd_ensemble_predictive_scores is sepaihrd_ensemble_predictive_nb -- same preconditions, failure codes,
 * memory rule, stream coordinates and failed-sample rule, the same draws bit for bit, and pred_quantiles, means, draws, k_used,
 * status, n_valid that call's for the same inputs (with observed == NULL so is pit) -- and scores every (time, age) cell of the
 * three daily series from the segment of m = n_valid R draws while it is still sorted for the quantiles: no segment is sorted
 * twice, and the mid-PIT comes from the sorted segment's counts instead of a pass of its own.
 *   observed     [3][T_pos][n_age] or NULL: the table every score and the PIT of this call are taken against; NULL: the context's
 *                observations.  A cell is usable when its value is finite and >= 0 (it need not be an integer).  A fit with the
 *                days after T0 set to NaN, scored with the full table, is a forecast check
 *   levels       [n_levels], 0 <= n_levels <= 8 (L below): central coverage levels c, each strictly inside (0, 1)
 *   cell_scores  [3][T_pos][n_age][5 + 4 L]: mean S1 / m; variance (S2 - S1 S1 / m) / (m - 1), NaN for m = 1; median q(0.5);
 *                CRPS A / m - G / (m m) with A = sum |x - y| and G = sum_i (2 i - m + 1) x(i) over the sorted draws;
 *                WIS (0.5 |y - median| + sum_l (alpha_l / 2) IS_l) / (L + 0.5), alpha_l = 1 - c_l; then per level
 *                lo = q(0.5 - 0.5 c), hi = q(0.5 + 0.5 c), IS = (hi - lo) + (2 / alpha)(max(0, lo - y) + max(0, y - hi)),
 *                covered (1.0 or 0.0).  q is the quantile rule of pred_quantiles.  Mean, variance, median, lo, hi for every cell
 *                with m > 0; CRPS, WIS, IS, covered NaN where the cell is not usable; every field NaN when m = 0
 *   summary      [3][n_age + 1][4 + 2 L], entry n_age pooling all ages: the number of usable cells, the means of CRPS, WIS and
 *                |y - median|, per level the coverage fraction and the mean IS; sums from 0.0 over the usable cells with time
 *                ascending (pooled: ages ascending within a time); a count of 0 gives NaN means
 *   pit          [3][T_pos][n_age] or NULL: (n_less + 0.5 n_eq) / m against `observed`
 *   exact        NULL or [1]: 1 when, for every daily cell, m x_max max(m, x_max) < 2^53.  The draws are integers, so every sum
 *                above is then exact and independent of the order it is formed in, and the host twin
 *                (hostPosteriorPredictiveScores, the text csrc/sepaihrd_predictive_score.inc) gives the same bits from means,
 *                status and k_used; 0: the scores are right to rounding but not promised equal to the twin's
 * SEPAIHRD_E_INVALID_ARG with a message that names the first wrong argument; sepaihrd_predictive_scores_validate is the same
 * check without a context (host only).  sepaihrd_predictive_timing reports this call when it was the last; its third phase is
 * sorts, quantiles and scores. */
int sepaihrd_ensemble_predictive_scores(sepaihrd_ctx *ctx, const double *theta, int S, int R, uint64_t seed,
                                        const double *dispersion /* [3] or NULL: the context's, as in _predictive_nb */,
                                        const double *observed /* [3][T_pos][n_age] or NULL: the context's observations */,
                                        const double *probs, int n_probs, const double *levels, int n_levels, double *pred_quantiles,
                                        double *pit, double *cell_scores, double *summary, double *means, double *draws, double *k_used,
                                        int32_t *status, int32_t *n_valid, int32_t *exact);
int sepaihrd_predictive_scores_validate(int S, int R, int T_pos, int n_age, const double *probs, int n_probs, const double *levels,
                                        int n_levels, char *err, int errlen);

/* ---- the same scores on window and age-group totals (additive; SEPAIHRD_ABI_VERSION stays) -----------------------------------
 * Forecasts of surveillance counts are judged on weekly totals, often summed over ages, and a weekday reporting artefact the model
 * has no term for spoils every daily interval of a fit whose weekly totals are right.  The distribution of a sum is no function of
 * the per-cell quantiles: it needs the joint draws.  sepaihrd_ensemble_predictive_targets draws the replicates of
 * sepaihrd_ensemble_predictive_scores -- same preconditions, failure codes, stream coordinates and failed-sample rule, and means,
 * draws (the daily table), k_used, status, n_valid that call's for the same inputs, bit for bit -- and sums them on the device into
 * targets (the rule: csrc/sepaihrd_predictive_targets.inc): an age group x a window of output rows, plus the running sums of those
 * window totals.  Every target segment is sorted once and gives quantiles, mid-PIT, scores and summaries for six series:
 * k = 0, 1, 2 the window totals of H, ICU, D, k = 3, 4, 5 their running sums over the windows.
 *   age_group        [n_age]: -1 leaves the age out, otherwise a group id; the ids in use must be exactly 0 .. G - 1, 1 <= G <= n_age
 *   window, origin   w >= 1 and o >= 0 in output rows with t >= 0: W = (T_pos - o) / w windows (integer division; W >= 1), window v
 *                    covers rows o + v w .. o + (v + 1) w - 1; rows before o and the incomplete tail belong to no target.  On a
 *                    daily grid w = 7 is a week
 *   observed         as in the scored call.  The observed target is the same sum of the table (rows ascending, ages ascending
 *                    within a row, from 0.0; the running sum adds the window totals in order).  A window target is usable when
 *                    every daily observation it sums is (finite and >= 0), a cumulative one when every window u <= v of its series
 *                    and group is; an unusable observed target is NaN
 *   target_quantiles [6][n_probs][W][G]: the quantile rule of pred_quantiles over the m = n_valid R values of the target
 *   pit              [6][W][G] or NULL;  target_obs [6][W][G] or NULL: the observed targets
 *   target_scores    [6][W][G][5 + 4 L], summary [6][G + 1][4 + 2 L] (entry G pools the groups): the fields of cell_scores and
 *                    summary above, a target in the place of a cell; summary order windows ascending, groups ascending within one
 *   target_draws     [S][R][3][W][G] or NULL: the window totals of the three daily series of every draw, NaN for failed samples
 *   exact            NULL or [1]: the scored call's criterion, m x_max max(m, x_max) < 2^53, over every one of the 6 W G segments;
 *                    the host twin (hostPosteriorPredictiveTargets) then gives the same bits and reports the same flag
 * Memory: 6 W G segments of S R doubles (padded as the other calls') plus the optional outputs; the scored call's 6 T_pos n_age
 * table is not allocated.  SEPAIHRD_E_INVALID_ARG with a message that names the first wrong argument: the scored call's refusals,
 * then age_group NULL, an id < -1 or >= n_age, a gap in the ids, no age in any group, window < 1, origin < 0, W < 1.
 * sepaihrd_predictive_targets_validate is the same check without a context (host only; W and G out, nullable).
 * sepaihrd_predictive_timing reports this call when it was the last: integrator; draws and their sums into the targets; sorts,
 * quantiles and scores. */
int sepaihrd_ensemble_predictive_targets(sepaihrd_ctx *ctx, const double *theta, int S, int R, uint64_t seed,
                                         const double *dispersion /* [3] or NULL */, const double *observed /* [3][T_pos][n_age] or NULL */,
                                         const int32_t *age_group /* [n_age] */, int window, int origin, const double *probs, int n_probs,
                                         const double *levels, int n_levels, double *target_quantiles /* [6][n_probs][W][G] */,
                                         double *pit /* [6][W][G] or NULL */, double *target_scores /* [6][W][G][5 + 4 L] */,
                                         double *summary /* [6][G + 1][4 + 2 L] */, double *target_obs /* [6][W][G] or NULL */,
                                         double *target_draws /* [S][R][3][W][G] or NULL */, double *means, double *draws, double *k_used,
                                         int32_t *status, int32_t *n_valid, int32_t *exact);
int sepaihrd_predictive_targets_validate(int S, int R, int T_pos, int n_age, const int32_t *age_group, int window, int origin,
                                         const double *probs, int n_probs, const double *levels, int n_levels, int *W, int *G, char *err,
                                         int errlen);

/* ---- stochastic chain-binomial SEPAIHRD ensembles over posterior samples (additive; SEPAIHRD_ABI_VERSION stays) -------------
 * Process noise for the age-structured model: the ensemble calls above give parameter uncertainty and observation noise, this
 * one simulates the epidemic itself as a chain-binomial process, R replicates per posterior sample.  The reference has no such
 * model; this one is this build's own.  csrc/sepaihrd_stoch_sepaihrd.inc states it (one text for the kernel and the host twin):
 *   - state: per age class the 11 compartments as int32; row 0 is the sample's deterministic initial state, built by the
 *     context's initial-state mode (S by subtraction included), every entry rounded with round();
 *   - a sample is SEPAIHRD_STATUS_INVALID when the deterministic rule rejects it or a rounded entry lies outside [0, 2^31 - 1];
 *     the counts of an age class whose total exceeds 2^31 - 1 wrap (no check: populations of that size are out of scope);
 *   - output interval k is cut into steps_per_interval = m steps h_k = (times[k+1] - times[k]) / m; step j has the global index
 *     k m + j and takes beta and kappa at its midpoint times[k] + (j + 0.5) h_k (the schedule lookup of the integrators);
 *   - lambda_i = max(0, (sum_j M(i,j) (P_j + A_j + theta I_j) h_infec_j / N_j) ((beta kappa) a_i)), from the state at the start
 *     of the step; 13 binomial draws per age class and step, all from that state (the table in the .inc file);
 *   - every variate is the binomial of csrc/sepaihrd_stoch.inc at Philox key = seed, counter = (s, r, (step 64 + age) 16 +
 *     transition, attempt), s the sample's position in theta, r the replicate.
 * A replicate's path is a function of (seed, s, r) and the sample's model values alone: it does not depend on S, R, keep, the
 * launch, the sort path or on which other samples are invalid.  The arithmetic mode of the context does not change the result.
 *   quantiles     [6][n_probs][T_pos][n_age] over the n_valid R replicates, output times t >= 0: series 0..2 the daily
 *                 increments of CumH, CumICU and D (hospitalisations, ICU admissions, deaths; the first row of the run has
 *                 increment 0), 3..5 their running sums over the output times >= 0; the quantile rule and the sorts of
 *                 sepaihrd_ensemble_predictive
 *   extinct       [S] or NULL: share of the sample's replicates with E + P + A + I = 0 in every age class at the last time;
 *                 NaN for an invalid sample
 *   model_values  [S][W] or NULL, W = sepaihrd_stochastic_values_width(n_age, n_beta, n_kappa): what the replicates ran with,
 *                 after the constraints of the context's constraint mode.  Row layout:
 *                   [0..7]  theta, sigma, gamma_p, gamma_A, gamma_I, gamma_H, gamma_ICU, beta
 *                   beta_values[n_beta], kappa_values[n_kappa]
 *                   [8][n_age]   a, h_infec, p, h, icu, d_H, d_ICU, d_community
 *                   [11][n_age]  the rounded initial counts S, E, P, A, I, H, ICU, R, D, CumH, CumICU (written for invalid
 *                                samples too, as rounded)
 *   traj          [S][keep][n_times][11][n_age] or NULL: every row of replicates 0 .. keep - 1; NaN for an invalid sample
 *   final_state   [S][R][11][n_age] or NULL: the last row of every replicate; NaN for an invalid sample
 *   status [S] or NULL; n_valid: count of status 0, or NULL
 * The host twin (host/: hostStochasticSEPAIHRD) reproduces quantiles, extinct, traj and final_state bit for bit from
 * model_values, status and the problem's fixed data.
 * SEPAIHRD_E_INVALID_ARG, before the device is touched: R < 1, steps_per_interval < 1, keep outside [0, R], keep > 0 without
 * traj, S R >= 2^31 (rounded up to whole wavefronts), n_times steps_per_interval >= 2^22, a probability outside [0, 1], a
 * pending sepaihrd_eval_batch_begin, or buffers (6 T_pos n_age segments of S R doubles plus the outputs asked for) beyond the
 * device's memory -- the rule of sepaihrd_ensemble_predictive.  SEPAIHRD_E_UNSUPPORTED in F32 precision or beyond 16 age
 * classes. */
int sepaihrd_ensemble_stochastic(sepaihrd_ctx *ctx, const double *theta, int S, int R, int steps_per_interval, uint64_t seed,
                                 const double *probs, int n_probs, int keep, double *quantiles, double *extinct, double *model_values,
                                 double *traj, double *final_state, int32_t *status, int32_t *n_valid);
/* Host only: the argument rules above that need no context, with a message in err (NULL: not wanted). */
int sepaihrd_stochastic_validate(int S, int R, int steps_per_interval, int keep, int n_times, int T_pos, int n_age, const double *probs,
                                 int n_probs, char *err, int errlen);
/* Host only: W, the width of a model_values row; SEPAIHRD_E_INVALID_ARG for n_age < 1 or a negative count. */
int sepaihrd_stochastic_values_width(int n_age, int n_beta, int n_kappa);
/* Device time of the context's last sepaihrd_ensemble_stochastic call in milliseconds, ms[2]: step kernel; segment sorts and
 * quantiles. */
int sepaihrd_stochastic_timing(const sepaihrd_ctx *ctx, double *ms);

/* ---- bootstrap particle filter of the stochastic SEPAIHRD model (additive; SEPAIHRD_ABI_VERSION stays) ----------------------
 * sepaihrd_ensemble_stochastic simulates the chain-binomial model forward; this call says how probable the observed
 * hospitalisations, ICU admissions and deaths are under it: an unbiased estimate of the marginal likelihood p(y | theta) under
 * process noise, by a bootstrap particle filter with systematic resampling (Gordon, Salmond & Smith 1993; Kitagawa 1996).  The
 * reference has no such filter; this one is this build's own.  csrc/sepaihrd_particle.inc states it (one text for the kernel and
 * the host twin):
 *   - particles: for theta[b], slot j (0 <= j < J) starts from the rounded initial counts of b's model_values row and advances
 *     with the model step of sepaihrd_ensemble_stochastic at stream coordinates (seed, s = b, r = j): until the first resampling,
 *     and so through the whole run-up, slot j IS replicate j of that call.  A slot keeps drawing at its own index after an
 *     ancestor has overwritten it;
 *   - log-weight at output row k, t = k - runup_offset >= 0: per age the increments of CumH, CumICU and D since the previous
 *     output row (0 at the run's first row), sim = max(0, inc) + 1e-10, term = obs log(sim) - sim where the observation is usable
 *     (finite and >= 0, the likelihood's rule) and 0 elsewhere; lw_j = sum over ages, ascending, of (term_H + term_ICU) + term_D;
 *   - a row without any usable cell is skipped: no weighting, no resampling, increment 0, ESS NaN;
 *   - M = max_j lw_j, w_j = exp(lw_j - M), C and Q the inclusive prefix sums of w and w^2 in the Kogge-Stone order;
 *     increment = M + log(C[J-1] / J), ESS = C[J-1]^2 / Q[J-1], loglik[b] = the sum of the increments in time order;
 *   - systematic resampling at EVERY weighted row from one uniform per (b, k) (Philox counter (b, 0xFFFFFFFF, (64 k) 16 + 13, 0),
 *     which no particle uses): the ancestor of slot i is the smallest j with C[j] > ((u + i) / J) C[J-1], clamped to J - 1; the
 *     slot takes the ancestor's counts and its previous-row CumH, CumICU, D.  Weights are equal after every resampling: none are
 *     carried, and there is no adaptive (ESS-threshold) rule.
 * One workgroup holds all particles of one theta in LDS: J <= sepaihrd_particle_max_particles(n_age) (464, 258, 136, 70, 35 for
 * up to 1, 2, 4, 8, 16 age classes).  The result for theta[b] is a function of (seed, b, J, steps_per_interval) and its model
 * values alone: it does not depend on B, on the outputs asked for or on which other vectors are invalid.  The arithmetic mode of
 * the context does not change the result.
 *   loglik        [B]; -DBL_MAX for an invalid theta (status SEPAIHRD_STATUS_INVALID), the objective's lowest()
 *   increments    [B][T_pos] or NULL: the increment of every output time >= 0 (0 for a skipped row; NaN for an invalid theta)
 *   ess           [B][T_pos] or NULL: NaN for a skipped row and for an invalid theta
 *   final_state   [B][J][11][n_age] or NULL: the particles after the last row's resampling; NaN for an invalid theta
 *   model_values  [B][W] or NULL: the layout of sepaihrd_ensemble_stochastic
 *   status [B] or NULL; n_valid: count of status 0, or NULL
 * The host twin (host/: hostParticleLoglik) reproduces loglik, increments, ess and final_state bit for bit from model_values,
 * status, the problem's fixed data and the observations.
 * SEPAIHRD_E_INVALID_ARG, before the device is touched and with the outputs untouched: B < 1, J < 1 or above
 * sepaihrd_particle_max_particles, steps_per_interval < 1, n_times steps_per_interval >= 2^22, a pending
 * sepaihrd_eval_batch_begin, or buffers beyond the device's memory.  SEPAIHRD_E_UNSUPPORTED in F32 precision or beyond 16 age
 * classes. */
int sepaihrd_particle_loglik(sepaihrd_ctx *ctx, const double *theta, int B, int J, int steps_per_interval, uint64_t seed,
                             double *loglik, double *increments, double *ess, double *final_state, double *model_values,
                             int32_t *status, int32_t *n_valid);
/* Host only: the argument rules above that need no context, with a message in err (NULL: not wanted). */
int sepaihrd_particle_validate(int B, int J, int steps_per_interval, int n_times, int T_pos, int n_age, char *err, int errlen);
/* Host only: the largest J the filter kernel takes for n_age classes; SEPAIHRD_E_INVALID_ARG outside 1..16. */
int sepaihrd_particle_max_particles(int n_age);
/* Device time of the context's last sepaihrd_particle_loglik or sepaihrd_particle_loglik_nb call (whichever came last) in
 * milliseconds, ms[2]: decode; filter kernel. */
int sepaihrd_particle_timing(const sepaihrd_ctx *ctx, double *ms);
/* Probe of the device's normalisation, scans and ancestor search: one weighted row with log-weights logw [J] (finite, J in
 * 1..512) at the resampling coordinates of (seed, b, row), through the device functions the filter kernel uses.  ancestors [J],
 * increment and ess: host memory. */
int sepaihrd_particle_resample_device(int device, uint64_t seed, uint32_t b, uint32_t row, const double *logw, int J,
                                      int32_t *ancestors, double *increment, double *ess, char *err, int errlen);

/* ---- the wide form of that filter: thousands of particles per theta (additive; SEPAIHRD_ABI_VERSION stays) -------------------
 * The same filter -- the particle coordinates, the log-weight, M, w, the Kogge-Stone order of the two prefix sums, the increment,
 * the ESS, the resampling uniform, the binary-search ancestor, resampling at every weighted row, skipped rows and invalid theta
 * are those of csrc/sepaihrd_particle.inc, unchanged -- with the particles in device memory and the work of every output row
 * spread over the whole device: J up to sepaihrd_particle_wide_max_particles() = 65536.  For J within
 * sepaihrd_particle_max_particles(n_age) the outputs are the bits of sepaihrd_particle_loglik; for every J they are the bits of the
 * host twin (host/: hostParticleLoglikWide).  Outputs, statuses and the rules for an invalid theta are word for word those of
 * sepaihrd_particle_loglik, and so is what the result for theta[b] depends on: (seed, b, J, steps_per_interval) and its model
 * values alone -- not B, not the outputs asked for, not the arithmetic mode, not theta_chunk.
 * The call runs as plain launches on one stream: per segment of output rows (the rows after a weighted row up to and including
 * the next, a row being weighted when its time is >= 0 and one of its cells is usable) one propagate-and-weight launch, per
 * weighted row one normalise-and-resample launch with one workgroup per theta.
 *   theta_chunk   the B vectors pass through the scratch theta_chunk at a time, chunk after chunk; b in the stream coordinates is
 *                 the position in the call.  0: as many as keep the scratch at or under 1 GiB (at least one).  The scratch is
 *                 theta_chunk J (88 lpc + 44) bytes, lpc = n_age rounded up to a power of two.
 * SEPAIHRD_E_INVALID_ARG, before the device is touched and with the outputs untouched: B < 1, J outside [1, 65536],
 * theta_chunk < 0, steps_per_interval < 1, n_times steps_per_interval >= 2^22, B J >= 2^31, a pending sepaihrd_eval_batch_begin,
 * or scratch and buffers beyond the device's memory.  SEPAIHRD_E_UNSUPPORTED in F32 precision or beyond 16 age classes. */
int sepaihrd_particle_loglik_wide(sepaihrd_ctx *ctx, const double *theta, int B, int J, int steps_per_interval, uint64_t seed,
                                  int theta_chunk, double *loglik, double *increments, double *ess, double *final_state,
                                  double *model_values, int32_t *status, int32_t *n_valid);
/* Host only: the argument rules above that need no context, with a message in err (NULL: not wanted). */
int sepaihrd_particle_wide_validate(int B, int J, int steps_per_interval, int theta_chunk, int n_times, int T_pos, int n_age,
                                    char *err, int errlen);
/* Host only: the largest J the wide form takes, 65536 for every n_age. */
int sepaihrd_particle_wide_max_particles(void);
/* Device time of the context's last sepaihrd_particle_loglik_wide or sepaihrd_particle_loglik_wide_nb call (whichever came last) in
 * milliseconds, ms[2]: decode; all filter launches. */
int sepaihrd_particle_wide_timing(const sepaihrd_ctx *ctx, double *ms);
/* Probe of the wide form's normalise-and-resample kernel: one weighted row with log-weights logw [J] (finite, J in 1..65536) at
 * the resampling coordinates of (seed, b, row).  ancestors [J], increment and ess: host memory. */
int sepaihrd_particle_wide_resample_device(int device, uint64_t seed, uint32_t b, uint32_t row, const double *logw, int J,
                                           int32_t *ancestors, double *increment, double *ess, char *err, int errlen);

/* ---- a negative-binomial observation model for both filters (additive; SEPAIHRD_ABI_VERSION stays) ---------------------------
 * The two calls above weigh a particle as if the observed counts were Poisson around the simulated increments.  These two give
 * each observed series a dispersion k: dispersion[3] = {k_H, k_ICU, k_D}, every entry +inf or finite in [1e-3, 1e6].  +inf keeps
 * the Poisson term of that series, untouched.  A finite k makes the series negative binomial with mean sim and size k (variance
 * sim + sim^2 / k; csrc/sepaihrd_particle.inc states the rule, one text for both kernels and the host twin):
 *   - the term of a usable cell is  obs log(sim) - (obs + k) log(1 + sim / k),  sim = max(0, inc) + 1e-10 as before, 0 where the
 *     cell is not usable; the sum over a class keeps its association (term_H + term_ICU) + term_D;
 *   - what is left of the log-pmf, g(obs, k) = lgamma(obs + k) - lgamma(k) - obs log(k), is shared by every particle of a row and
 *     never enters the weights: its sum G over the row's usable cells with a finite k (ascending age; H, ICU, D within an age;
 *     from 0.0; glibc's lgamma and log on the host) is added to the row's increment, increment = (M + log(C[J-1] / J)) + G;
 *   - the -lgamma(obs + 1) of the pmf is left out, as the Poisson term leaves it out.  With that convention term + g tends to the
 *     Poisson term as k grows: the difference is ((sim - obs)^2 - obs) / (2 k) + O(k^-2).  Above 1e6 the cancellation in these
 *     formulas costs more than 1e-8, hence the upper bound.
 * M, w, the scans, the ESS, the resampling uniform, the ancestors, skipped rows, invalid theta, the limits on J and every other
 * argument rule are those of the Poisson calls.  With all three entries +inf no table is formed and the Poisson kernels run: the
 * outputs are the bits of sepaihrd_particle_loglik and sepaihrd_particle_loglik_wide.  The host twins are hostParticleLoglikNB and
 * hostParticleLoglikWideNB (host/), bit for bit.
 * SEPAIHRD_E_INVALID_ARG, before the device is touched and with the outputs untouched: what the Poisson call refuses, and a
 * dispersion sepaihrd_particle_nb_validate refuses. */
int sepaihrd_particle_loglik_nb(sepaihrd_ctx *ctx, const double *theta, int B, int J, int steps_per_interval, uint64_t seed,
                                const double dispersion[3], double *loglik, double *increments, double *ess, double *final_state,
                                double *model_values, int32_t *status, int32_t *n_valid);
int sepaihrd_particle_loglik_wide_nb(sepaihrd_ctx *ctx, const double *theta, int B, int J, int steps_per_interval, uint64_t seed,
                                     const double dispersion[3], int theta_chunk, double *loglik, double *increments, double *ess,
                                     double *final_state, double *model_values, int32_t *status, int32_t *n_valid);
/* Host only: SEPAIHRD_E_INVALID_ARG with a message in err (NULL: not wanted) that names the entry for a NULL pointer, a NaN, -inf,
 * a value <= 0, a finite value below 1e-3 or a finite value above 1e6. */
int sepaihrd_particle_nb_validate(const double dispersion[3], char *err, int errlen);
/* Host only: G [T_pos], the row constants a call with this dispersion uploads (all 0 where every entry is +inf). */
int sepaihrd_particle_nb_row_constants(const sepaihrd_ctx *ctx, const double dispersion[3], double *G);
/* Probe of the device's negative-binomial term: out[i] = the term of obs[i] (double) and inc[i] (int32) under a finite k in
 * [1e-3, 1e6], count cells; host memory. */
int sepaihrd_particle_nb_term_device(int device, const double *obs, const int32_t *inc, int count, double k, double *out,
                                     char *err, int errlen);

/* ---- filtered state means and quantile bands of every output row (additive; SEPAIHRD_ABI_VERSION stays) ------------------------
 * The wide form of the filter with the other product of a particle filter: the filtering distribution of the latent state at
 * every output row k in 0 .. n_times - 1, run-up rows included, summarised over the J particles the next interval starts from
 * (after a weighted row slot i holds the state of its ancestor, so the set is equally weighted; after an unweighted row the
 * particles as propagated; row n_times - 1 is the set sepaihrd_particle_loglik_wide's final_state holds).  For each of the 11
 * counts there are n_age + 1 series: one per age class and, at index n_age, the particle's sum over its age classes.
 *   state_mean      [B][n_times][11][n_age + 1]            (double)(the sum of the J counts in 64-bit integers) / (double)J
 *   state_quantiles [B][n_times][11][n_age + 1][n_probs]   the ensemble's rule over the J values sorted ascending: pos = p (J - 1),
 *                   idx = (size_t)pos, frac = pos - idx, v[idx] (1 - frac) + v[idx + 1] frac where idx + 1 < J, else v[idx];
 *                   NULL: not wanted
 * csrc/sepaihrd_particle_states.inc states the rule, one text for the device and the host twin (hostParticleStates, bit for bit).
 * The filter is untouched: loglik, increments, ess, model_values, status and n_valid are those of sepaihrd_particle_loglik_wide
 * (dispersion NULL) or sepaihrd_particle_loglik_wide_nb (dispersion [3]), bit for bit; J is 1 to 65 536 for every n_age.  An
 * invalid theta has NaN in every row of both tables.  theta_chunk as in the wide form; the scratch of a chunk is the wide form's
 * plus a row table of 88 (n_age + 1) pad bytes per theta, pad = the power of two >= max(J, 64).
 * SEPAIHRD_E_INVALID_ARG, before the device is touched and with the outputs untouched: what sepaihrd_particle_states_validate
 * refuses, a dispersion sepaihrd_particle_nb_validate refuses, a NULL theta, loglik or state_mean, state_quantiles with
 * n_probs == 0. */
int sepaihrd_particle_filter_states(sepaihrd_ctx *ctx, const double *theta, int B, int J, int steps_per_interval, uint64_t seed,
                                    int theta_chunk, const double *dispersion /* [3] or NULL: Poisson */,
                                    const double *probs, int n_probs,
                                    double *loglik, double *increments, double *ess,
                                    double *state_mean      /* [B][T][11][n_age+1] */,
                                    double *state_quantiles /* [B][T][11][n_age+1][n_probs] or NULL */,
                                    double *model_values, int32_t *status, int32_t *n_valid);
/* Host only: the rules of sepaihrd_particle_wide_validate and, with a message that names this entry, n_probs outside [0, 64],
 * n_probs > 0 with NULL probs, a probability that is NaN or outside [0, 1]. */
int sepaihrd_particle_states_validate(int B, int J, int steps_per_interval, int theta_chunk, int n_times, int T_pos, int n_age,
                                      const double *probs, int n_probs, char *err, int errlen);
/* Device time of the context's last sepaihrd_particle_filter_states call in milliseconds, ms[3]: decode; all launches of the
 * filter and the summaries; of these the summaries' launches of the first chunk of parameter vectors -- the whole share of the
 * summaries where the call has one chunk (NaN on a grid of more than 1024 output rows). */
int sepaihrd_particle_states_timing(const sepaihrd_ctx *ctx, double *ms);

/* ---- negative-binomial observation model of the deterministic objective (additive; SEPAIHRD_ABI_VERSION stays) ----------------
 * The reference's objective is Poisson.  Here each observed series (H, ICU, D) may have a dispersion k, +inf (the default: that
 * series keeps the Poisson cell) or finite in [1e-3, 1e6], either fixed on the context (sepaihrd_set_dispersion) or calibrated: a
 * theta entry with field SEPAIHRD_F_DISPERSION and param_index 0, 1, 2 for H, ICU, D, constrained like every other entry.
 * For a usable cell (obs finite and >= 0) of a series with finite k, sim = max(0, increment) + 1e-10 as in the Poisson cell,
 *     term = obs log(sim) - (obs + k) log(1 + sim / k)        (nb_term of the particle filters, sim real-valued)
 *     g    = lgamma(obs + k) - lgamma(k) - obs log(k),        exactly 0 when obs == 0
 * and the cell is term + g; the -lgamma(obs + 1) of the pmf is left out, as the Poisson cell leaves it out.  An unusable cell is 0.
 * Sums as in the Poisson objective: the ages ascending within a day, the days ascending from 0.0 per series, total = (H + ICU) + D,
 * a NaN or Inf total gives status 1 and lowest(); ll_parts are the three series sums, g included.  lgamma is an explicit
 * operation sequence (csrc/sepaihrd_lgamma.inc) over the library's restatement of glibc's log: host twin and device agree in
 * everything but log(sim), which the device takes through its table path (sepaihrd_device_log_values) and the twin from std::log.
 * Every entry point that evaluates through the context follows: sepaihrd_eval_batch / _device / _begin / _end,
 * sepaihrd_fd_gradient_batch (set both contexts alike), sepaihrd_mh_*.  A dispersed context integrates in a form that parks its
 * increments (the likelihood_form SEPAIHRD_LL_SEPARATE_PASS) and runs the negative-binomial pass over them instead of the Poisson
 * pass; sepaihrd_reserve sizes the workspace for it.  With all three series at +inf nothing changes: the kernels and the bits
 * of the Poisson objective.  SEPAIHRD_PRECISION_F32 with a dispersed series: SEPAIHRD_E_UNSUPPORTED from the evaluation.
 * sepaihrd_ensemble_predictive_nb draws its replicates under this model.  The other ensemble entry points (sepaihrd_ensemble_predictive
 * among them) and the particle filters do not read the context's dispersion.
 *   create          refuses a SEPAIHRD_F_DISPERSION entry whose index is not 0, 1, 2, that has no bounds, whose bounds do not
 *                   satisfy 1e-3 <= lower <= upper <= 1e6, or that names a series another entry already calibrates
 *                   (sepaihrd_dispersion_validate's message in err)
 *   set_dispersion  k[3]: the fixed values of the series theta does not calibrate (the others' entries are ignored); refuses
 *                   what sepaihrd_particle_nb_validate refuses, with its message as the context's last error
 *   get_dispersion  k[3]: the fixed values, NaN for a calibrated series */
int sepaihrd_set_dispersion(sepaihrd_ctx *ctx, const double k[3]);
int sepaihrd_get_dispersion(const sepaihrd_ctx *ctx, double k[3]);
/* Host only: the rules sepaihrd_create applies to the SEPAIHRD_F_DISPERSION entries of a parameter map (lower / upper / has_bounds
 * as in sepaihrd_problem; has_bounds NULL: bounded where both arrays are given).  series_param [3] (nullable): the theta index
 * that calibrates each series, -1 for none. */
int sepaihrd_dispersion_validate(int n_params, const int32_t *param_field, const int32_t *param_index, const double *lower,
                                 const double *upper, const uint8_t *has_bounds, int32_t *series_param, char *err, int errlen);
/* Host only, the twin of the pass: increments [B][T][3][n_age] (series H, ICU, D; the daily differences of CumH, CumICU, D, not yet
 * clamped at 0), observations obs_* [T][n_age] (NaN where there is none), k [B][3] -> loglik [B], ll_parts [B][3] (nullable),
 * status [B] (nullable; 0 or 1).  Compiled from the text the device pass compiles, with std::log for log(sim). */
int sepaihrd_nb_objective_host(const double *increments, const double *obs_H, const double *obs_ICU, const double *obs_D,
                               const double *k, int B, int T, int n_age, double *loglik, double *ll_parts, int32_t *status);
/* lgamma of csrc/sepaihrd_lgamma.inc for x in [1e-3, 1e6 + the largest observation]: on the host, and a probe of the device's
 * (n values, host memory), bit for bit the same. */
double sepaihrd_lgamma_host(double x);
int sepaihrd_lgamma_device(int device, const double *x, int n, double *out, char *err, int errlen);

#ifdef __cplusplus
}
#endif
#endif /* SEPAIHRD_HIP_H */
