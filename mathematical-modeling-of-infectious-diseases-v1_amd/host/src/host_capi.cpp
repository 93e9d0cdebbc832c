// host_capi.cpp -- flat C entry points over the C++ host mirror, for the Python test-suite only.
// The layout of `sepaihrd_problem` is reused as the carrier of the model / data arrays.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "epidemic_hip/BatchedHillClimbing.hpp"
#include "epidemic_hip/HipChainDiagnostics.hpp"
#include "epidemic_hip/BatchedParticleSwarm.hpp"
#include "epidemic_hip/HipModelCalibrator.hpp"
#include "epidemic_hip/HipNUTSSampler.hpp"
#include "epidemic_hip/MultiChainNUTSSampler.hpp"
#include "epidemic_hip/HipPosteriorEnsemble.hpp"
#include "epidemic_hip/HipPosteriorPredictive.hpp"
#include "epidemic_hip/HipParticleFilter.hpp"
#include "epidemic_hip/HipStochasticSEPAIHRD.hpp"
#include "epidemic_hip/HipSEPAIHRD.hpp"
#include "epidemic_hip/HipSIR.hpp"
#include "epidemic_hip/HipSIRScenarioAnalysis.hpp"
#include "sepaihrd_hip.h"
#include "sepaihrd_rng.inc"
#include "sepaihrd_nb_objective.inc"

using namespace epidemic;

namespace {
struct HostHandle {
    std::unique_ptr<HipSEPAIHRDParameterManager> pm;
    std::unique_ptr<SimulationCache> cache;
    std::unique_ptr<CalibrationData> data;
    std::unique_ptr<HipSEPAIHRDObjectiveFunction> obj;
    std::string error;
    // host_objective_set_dispersion: kept for the gradient objectives the calls below build over this handle's manager
    bool has_dispersion = false;
    double dispersion[3] = {0.0, 0.0, 0.0};
    bool mh_diagnostics = false;        // host_set_mh_diagnostics: compute_diagnostics for the runs below
    ChainDiagnosticsTable last_diag;    // of the last host_mh_run / host_calibrate / host_calibrate_pso
};
std::vector<std::string> split_lines(const char* s) {
    std::vector<std::string> out;
    if (!s) return out;
    std::stringstream ss(s);
    std::string line;
    while (std::getline(ss, line, '\n'))
        if (!line.empty()) out.push_back(line);
    return out;
}
// the host strategy of a sepaihrd_problem solver code
std::shared_ptr<IOdeSolverStrategy> strategy_for(int solver) {
    if (solver == SEPAIHRD_SOLVER_CASH_KARP54) return std::make_shared<CashKarpSolverStrategy>();
    if (solver == SEPAIHRD_SOLVER_FEHLBERG78) return std::make_shared<FehlbergSolverStrategy>();
    return std::make_shared<Dopri5SolverStrategy>();
}
Eigen::VectorXd vec(const double* p, int n) {
    Eigen::VectorXd v(n);
    for (int i = 0; i < n; ++i) v[i] = p ? p[i] : 0.0;
    return v;
}
// the model parameters and the observation tables a sepaihrd_problem carries
SEPAIHRDParameters model_parameters(const sepaihrd_problem* pb) {
    const int n = pb->n_age;
    SEPAIHRDParameters mp;
    mp.N = vec(pb->N, n);
    mp.M_baseline = Eigen::MatrixXd(n, n);
    std::memcpy(mp.M_baseline.data(), pb->M, sizeof(double) * n * n);
    mp.a = vec(pb->a, n); mp.h_infec = vec(pb->h_infec, n); mp.p = vec(pb->p, n); mp.h = vec(pb->h, n);
    mp.icu = vec(pb->icu, n); mp.d_H = vec(pb->d_H, n); mp.d_ICU = vec(pb->d_ICU, n);
    mp.d_community = vec(pb->d_community, n);
    mp.beta = pb->beta; mp.theta = pb->theta; mp.sigma = pb->sigma; mp.gamma_p = pb->gamma_p;
    mp.gamma_A = pb->gamma_A; mp.gamma_I = pb->gamma_I; mp.gamma_H = pb->gamma_H; mp.gamma_ICU = pb->gamma_ICU;
    mp.beta_end_times.assign(pb->beta_end_times, pb->beta_end_times + pb->n_beta);
    mp.beta_values.assign(pb->beta_values, pb->beta_values + pb->n_beta);
    mp.kappa_end_times.assign(pb->kappa_end_times, pb->kappa_end_times + pb->n_kappa);
    mp.kappa_values.assign(pb->kappa_values, pb->kappa_values + pb->n_kappa);
    mp.E0_multiplier = pb->multipliers[0]; mp.P0_multiplier = pb->multipliers[1];
    mp.A0_multiplier = pb->multipliers[2]; mp.I0_multiplier = pb->multipliers[3];
    mp.H0_multiplier = pb->multipliers[4]; mp.ICU0_multiplier = pb->multipliers[5];
    mp.R0_multiplier = pb->multipliers[6]; mp.D0_multiplier = pb->multipliers[7];
    mp.runup_days = pb->runup_days; mp.seed_exposed = pb->seed_exposed;
    return mp;
}
CalibrationData calibration_data(const sepaihrd_problem* pb, const Eigen::VectorXd& N) {
    const int n = pb->n_age;
    auto mat = [&](const double* src) {
        Eigen::MatrixXd m(pb->n_obs, n);
        for (int r = 0; r < pb->n_obs; ++r)
            for (int c = 0; c < n; ++c) m(r, c) = src[static_cast<size_t>(r) * n + c];
        return m;
    };
    return CalibrationData(mat(pb->obs_H), mat(pb->obs_ICU), mat(pb->obs_D), N);
}
thread_local std::string g_error;
thread_local double g_last_mh_loop_seconds = 0.0;
thread_local double g_last_diag_seconds = 0.0;

// The error guard of the entry points: 0 after body(); a std::exception leaves its message for host_last_error and gives 1.
template <class Body>
int guarded(Body&& body) {
    try {
        body();
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
        return 1;
    }
}

// samples [n][P] as the vectors the posterior classes take
std::vector<Eigen::VectorXd> sample_vectors(const double* samples, int n, size_t P) {
    std::vector<Eigen::VectorXd> ps;
    for (int s = 0; s < n; ++s) ps.push_back(vec(samples + static_cast<size_t>(s) * P, static_cast<int>(P)));
    return ps;
}
// HipPosteriorEnsemble / HipPosteriorPredictive over the handle's parameter manager and data, on the problem's grid, solver and arithmetic
template <class Posterior>
Posterior posterior_over(const HostHandle& h, const sepaihrd_problem* pb, int device) {
    return Posterior(*h.pm, *h.data, std::vector<double>(pb->times, pb->times + pb->n_times), vec(pb->initial_state, 11 * pb->n_age),
                     strategy_for(pb->solver), pb->abs_err, pb->rel_err, device, pb->arith == SEPAIHRD_ARITH_FMA);
}
// an aggregate {time -> {quantile name -> value}} as out [5: q025, q05, median, q95, q975][T]; NaN where a time is missing
void put_quantile_rows(const std::map<double, AggregatedStats>& agg, const std::vector<double>& times, double* out) {
    const char* keys[5] = {"q025", "q05", "median", "q95", "q975"};
    size_t k = 0;
    for (double t : times) {
        const auto it = agg.find(t);
        for (int q = 0; q < 5; ++q)
            out[static_cast<size_t>(q) * times.size() + k] = it == agg.end() ? std::numeric_limits<double>::quiet_NaN() : it->second.at(keys[q]);
        ++k;
    }
}
// the parameter manager in another constraint mode (1: MCMC_REFLECT, else OPTIMIZATION_CLAMP) until the end of the scope
class ConstraintModeScope {
public:
    ConstraintModeScope(HipSEPAIHRDParameterManager& pm, int mode) : pm_(pm), keep_(pm.getConstraintMode()) {
        pm_.setConstraintMode(mode == 1 ? ConstraintMode::MCMC_REFLECT : ConstraintMode::OPTIMIZATION_CLAMP);
    }
    ~ConstraintModeScope() { pm_.setConstraintMode(keep_); }
    ConstraintModeScope(const ConstraintModeScope&) = delete;
    ConstraintModeScope& operator=(const ConstraintModeScope&) = delete;
private:
    HipSEPAIHRDParameterManager& pm_;
    ConstraintMode keep_;
};

// ---- lock-step No-U-Turn chains (MultiChainNUTSSampler): output plumbing shared by the device run and the analytic hook
struct NutsChainsOut {
    int iterations, P;
    double *samples, *values, *eps_trace;   // [C][iterations][P], [C][iterations] x 2; NaN beyond a chain's n_samples
    int32_t *depth_trace, *n_samples;       // [C][iterations] (-2 beyond n_samples), [C]
    double *best, *best_value;              // [C][P], [C]
    int64_t *gradient_calls, *rows_evaluated;  // [C] x 2
    int32_t *failure_status, *failure_iteration;  // [C] x 2
    void put(int c, const NUTSChainResult& r) const {
        const size_t N = static_cast<size_t>(iterations), Pz = static_cast<size_t>(P), base = static_cast<size_t>(c) * N;
        const double nan = std::nan("");
        const size_t ns = std::min(r.samples.size(), N);
        for (size_t s = 0; s < N; ++s) {
            for (size_t i = 0; i < Pz; ++i) samples[(base + s) * Pz + i] = s < ns ? r.samples[s][i] : nan;
            values[base + s] = s < ns ? r.sample_values[s] : nan;
            eps_trace[base + s] = s < ns ? r.epsilon_trace[s] : nan;
            depth_trace[base + s] = s < ns ? r.depth_trace[s] : -2;
        }
        n_samples[c] = static_cast<int32_t>(ns);
        for (size_t i = 0; i < Pz; ++i) best[static_cast<size_t>(c) * Pz + i] = r.best_parameters.size() == Pz ? r.best_parameters[i] : nan;
        best_value[c] = r.best_value;
        gradient_calls[c] = r.gradient_calls;
        rows_evaluated[c] = r.rows_evaluated;
        failure_status[c] = r.failure_status;
        failure_iteration[c] = r.failure_iteration;
    }
};
std::map<std::string, double> nuts_settings(int iterations, int adaptation_window, double delta_target, int max_tree_depth, uint32_t seed) {
    return {{"nuts_iterations", double(iterations)}, {"nuts_adaptation_window", double(adaptation_window)},
            {"nuts_delta_target", delta_target}, {"nuts_max_tree_depth", double(max_tree_depth)}, {"seed", double(seed)}};
}
std::vector<std::vector<double>> chain_starts(const double* theta0, int C, int P) {
    std::vector<std::vector<double>> starts(static_cast<size_t>(C));
    for (int c = 0; c < C; ++c) starts[static_cast<size_t>(c)].assign(theta0 + static_cast<size_t>(c) * P, theta0 + static_cast<size_t>(c + 1) * P);
    return starts;
}

// ---- Metropolis-Hastings chains (MultiChainMetropolisHastings): what every entry point that runs them shares
// The settings every run starts from; `own` adds the entry point's keys.  Reporting is the reference's three keys, on
// (progress lines every report_interval iterations, checkpoint and trace files) or off.  A key left out keeps the
// default of a freshly constructed sampler.
using MhSettings = std::map<std::string, double>;
MhSettings mh_settings(int iterations, int burn_in, bool reported, int report_interval, std::initializer_list<MhSettings::value_type> own) {
    MhSettings s{{"mcmc_iterations", double(iterations)}, {"burn_in", double(burn_in)}, {"report_interval", reported ? double(report_interval) : 0.0},
                 {"write_checkpoints", reported ? 1.0 : 0.0}, {"write_trace", reported ? 1.0 : 0.0}};
    s.insert(own);
    return s;
}
// Per-chain outputs, chain-major; a NULL destination is skipped.  n_samples is the same for every chain.
struct MhChainsOut {
    int iterations, P;
    int32_t* accepted;                  // [C]
    double *best_value, *best, *final_scale;  // [C], [C][P], [C]
    unsigned char* accept_trace;        // [C][iterations - 1]
    int32_t* n_samples;                 // one count
    double *samples, *sample_values, *final_cov;  // [C][n_samples][P], [C][n_samples], [C][P][P]
    void put(int c, const OptimizationResult& r, const std::vector<unsigned char>* trace) const {
        const size_t Pz = static_cast<size_t>(P), cz = static_cast<size_t>(c), ns = r.samples.size();
        if (accepted) accepted[c] = static_cast<int32_t>(r.additionalStats.at("accepted_count"));
        if (best_value) best_value[c] = r.bestObjectiveValue;
        if (final_scale) final_scale[c] = r.additionalStats.at("final_scale");
        if (best) for (size_t i = 0; i < Pz; ++i) best[cz * Pz + i] = r.bestParameters[static_cast<Eigen::Index>(i)];
        if (accept_trace && trace) std::copy(trace->begin(), trace->end(), accept_trace + cz * static_cast<size_t>(iterations - 1));
        if (n_samples) *n_samples = static_cast<int32_t>(ns);
        for (size_t s = 0; s < ns; ++s) {
            if (samples) for (size_t i = 0; i < Pz; ++i) samples[(cz * ns + s) * Pz + i] = r.samples[s][static_cast<Eigen::Index>(i)];
            if (sample_values) sample_values[cz * ns + s] = r.sampleObjectiveValues[s];
        }
        if (final_cov)
            for (size_t i = 0; i < Pz; ++i)
                for (size_t j = 0; j < Pz; ++j)
                    final_cov[(cz * Pz + i) * Pz + j] = r.finalCovariance(static_cast<Eigen::Index>(i), static_cast<Eigen::Index>(j));
    }
    // every chain of a lock-step run with the sampler's accept traces (looked at only when a trace is wanted: a run
    // without keep_accept_traces has none)
    void put(const std::vector<OptimizationResult>& res, const std::vector<std::vector<unsigned char>>& traces) const {
        for (size_t c = 0; c < res.size(); ++c) put(static_cast<int>(c), res[c], accept_trace ? &traces[c] : nullptr);
    }
};
// the scalar path: chain c alone through optimize() with seed + c
void mh_scalar_chains(MultiChainMetropolisHastings& mh, int C, const double* initial, uint32_t seed, IObjectiveFunction& objective,
                      IParameterManager& pm, const MhChainsOut& out) {
    for (int c = 0; c < C; ++c) {
        mh.setSeed(seed + static_cast<uint32_t>(c));
        const OptimizationResult r = mh.optimize(vec(initial + static_cast<size_t>(c) * out.P, out.P), objective, pm);
        out.put(c, r, out.accept_trace ? &mh.acceptTraces()[0] : nullptr);
    }
}
// the progress lines of a reported run, one per line, into a file of their own (a NULL path leaves the sampler's sink alone)
class ProgressLog {
public:
    ProgressLog(MultiChainMetropolisHastings& mh, const char* path) {
        if (!path) return;
        file_.open(path);
        mh.setProgressSink([this](const std::string& level, const std::string& msg) { file_ << level << " " << msg << std::endl; });
    }
    ProgressLog(const ProgressLog&) = delete;
    ProgressLog& operator=(const ProgressLog&) = delete;
private:
    std::ofstream file_;
};
// failures [3] of a device-resident run; a host-loop run counts none
void put_failures(const std::vector<long>& counts, long* failures) {
    if (failures)
        for (size_t k = 0; k < 3; ++k) failures[k] = k < counts.size() ? counts[k] : 0;
}
// the objectives behind G handles, one device context each
std::vector<HipSEPAIHRDObjectiveFunction*> group_objectives(void** handles, int G) {
    std::vector<HipSEPAIHRDObjectiveFunction*> objs;
    for (int g = 0; g < G; ++g) objs.push_back(static_cast<HostHandle*>(handles[g])->obj.get());
    return objs;
}

// The device objective behind a stopwatch: wall time inside the batched evaluation and, when asked, the evaluation
// kernels' time from the two contexts' event timers (collected every tick: the call has just waited for its results).
class TimedRows : public IBatchGradientObjective {
public:
    TimedRows(HipSEPAIHRDGradientObjectiveFunction& obj, bool kernel_timing) : obj_(obj), timing_(kernel_timing) {
        if (timing_) { sepaihrd_set_timing(obj_.deviceContext(), 1); sepaihrd_set_timing(obj_.gradientContext(), 1); }
    }
    ~TimedRows() override {
        if (timing_) { sepaihrd_set_timing(obj_.deviceContext(), 0); sepaihrd_set_timing(obj_.gradientContext(), 0); }
    }
    void evaluateRows(const double* thetas, const uint8_t* want, int B, int P, double* values, double* grads, int32_t* status) override {
        const auto t0 = std::chrono::steady_clock::now();
        obj_.evaluateRows(thetas, want, B, P, values, grads, status);
        call_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!timing_) return;
        double a = 0.0, b = 0.0;
        int n = 0;
        if (sepaihrd_get_timing(obj_.deviceContext(), &a, &b, &n) == SEPAIHRD_OK) centre_ms += a + b;
        if (sepaihrd_get_timing(obj_.gradientContext(), &a, &b, &n) == SEPAIHRD_OK) perturbed_ms += a + b;
    }
    double call_seconds = 0.0, centre_ms = 0.0, perturbed_ms = 0.0;
private:
    HipSEPAIHRDGradientObjectiveFunction& obj_;
    bool timing_;
};

// Test objective (no GPU): log-density of a correlated Gaussian, -1/2 (x - mean)' A (x - mean), with its exact gradient;
// inside the ball |x - fail_centre| < fail_radius (radius > 0) an evaluation reports an integration failure instead.
class AnalyticGaussian : public IGradientObjectiveFunction, public IBatchGradientObjective {
public:
    AnalyticGaussian(int D, const double* mean, const double* precision, const double* fail_centre, double fail_radius)
        : D_(D), mean_(mean, mean + D), A_(precision, precision + static_cast<size_t>(D) * D),
          fail_centre_(fail_centre ? std::vector<double>(fail_centre, fail_centre + D) : std::vector<double>()), fail_radius_(fail_radius) {
        for (int i = 0; i < D; ++i) names_.push_back("x" + std::to_string(i));
    }
    bool fails(const double* x) const {
        if (fail_centre_.empty() || !(fail_radius_ > 0.0)) return false;
        double sq = 0.0;
        for (int i = 0; i < D_; ++i) sq += (x[i] - fail_centre_[static_cast<size_t>(i)]) * (x[i] - fail_centre_[static_cast<size_t>(i)]);
        return sq < fail_radius_ * fail_radius_;
    }
    double density(const double* x, double* grad) const {
        double quad = 0.0;
        for (int i = 0; i < D_; ++i) {
            double row = 0.0;
            for (int j = 0; j < D_; ++j) row += A_[static_cast<size_t>(i) * D_ + j] * (x[j] - mean_[static_cast<size_t>(j)]);
            if (grad) grad[i] = -row;
            quad += (x[i] - mean_[static_cast<size_t>(i)]) * row;
        }
        return -0.5 * quad;
    }
    double calculate(const Eigen::VectorXd& x) const override {
        if (fails(x.data())) HipSEPAIHRDObjectiveFunction::throwIntegrationFailure(SEPAIHRD_STATUS_STEP_FAILURE);
        return density(x.data(), nullptr);
    }
    double evaluate_with_gradient(const Eigen::VectorXd& x, Eigen::VectorXd& grad) const override {
        if (fails(x.data())) HipSEPAIHRDObjectiveFunction::throwIntegrationFailure(SEPAIHRD_STATUS_STEP_FAILURE);
        grad.resize(D_);
        return density(x.data(), grad.data());
    }
    const std::vector<std::string>& getParameterNames() const override { return names_; }
    void evaluateRows(const double* thetas, const uint8_t* want, int B, int P, double* values, double* grads, int32_t* status) override {
        for (int b = 0; b < B; ++b) {
            const double* x = thetas + static_cast<size_t>(b) * P;
            status[b] = fails(x) ? SEPAIHRD_STATUS_STEP_FAILURE : SEPAIHRD_STATUS_OK;
            values[b] = density(x, !want || want[b] ? grads + static_cast<size_t>(b) * P : nullptr);
        }
    }
private:
    int D_;
    std::vector<double> mean_, A_, fail_centre_;
    double fail_radius_;
    std::vector<std::string> names_;
};
// the manager of the analytic objective: unconstrained, one sigma for every coordinate
class FreeManager : public IParameterManager {
public:
    FreeManager(int D, double sigma) : D_(D), sigma_(sigma) {
        for (int i = 0; i < D; ++i) names_.push_back("x" + std::to_string(i));
    }
    Eigen::VectorXd getCurrentParameters() const override { return Eigen::VectorXd(D_); }
    void updateModelParameters(const Eigen::VectorXd&) override {}
    const std::vector<std::string>& getParameterNames() const override { return names_; }
    size_t getParameterCount() const override { return static_cast<size_t>(D_); }
    double getSigmaForParamIndex(int) const override { return sigma_; }
    Eigen::VectorXd applyConstraints(const Eigen::VectorXd& x) const override { return x; }
    int getIndexForParam(const std::string&) const override { return -1; }
    double getLowerBoundForParamIndex(int) const override { return -std::numeric_limits<double>::infinity(); }
    double getUpperBoundForParamIndex(int) const override { return std::numeric_limits<double>::infinity(); }
private:
    int D_;
    double sigma_;
    std::vector<std::string> names_;
};
}  // namespace

namespace epidemic {
void canonical_queue_draw_sequence(uint32_t seed, int P, int rounds, const unsigned char* takes_uniform, double* normals, double* log_u);
}

extern "C" {

// test hook: see canonical_queue_draw_sequence (MultiChainMetropolisHastings.cpp)
void host_queue_draw_sequence(uint32_t seed, int P, int rounds, const unsigned char* takes_uniform, double* normals, double* log_u) {
    epidemic::canonical_queue_draw_sequence(seed, P, rounds, takes_uniform, normals, log_u);
}

const char* host_last_error(void) { return g_error.c_str(); }
// iteration loop of this thread's last device-resident sampler run, without set-up and read-back (seconds)
double host_last_mh_loop_seconds(void) { return g_last_mh_loop_seconds; }

// Test hook (no GPU needed): what the adapter raises for a per-chain status >= 2.  Returns 1 when it is the
// SimulationException the reference's solver wrapper throws (Dopri5SolverStrategy.cpp:38-42), 0 for any other type;
// the message goes to host_last_error.
int host_status_exception(int status) {
    try {
        HipSEPAIHRDObjectiveFunction::throwIntegrationFailure(status);
    } catch (const SimulationException& e) {
        g_error = e.what();
        return 1;
    } catch (const std::exception& e) {
        g_error = e.what();
        return 0;
    }
    return 0;
}

// names / npi_names: '\n'-joined; sigmas: [P].  Bounds come from pb->lower/upper.
// with_objective = 0 builds the parameter manager only (no device needed)
void* host_objective_create(const sepaihrd_problem* pb, const char* names, const char* npi_names,
                            const double* sigmas, int device, int cache_capacity, int with_objective) {
    try {
        const int n = pb->n_age;
        const SEPAIHRDParameters mp = model_parameters(pb);
        const std::vector<std::string> nm = split_lines(names);
        std::map<std::string, double> sg;
        std::map<std::string, std::pair<double, double>> bd;
        for (size_t i = 0; i < nm.size(); ++i) {
            sg[nm[i]] = sigmas[i];
            bd[nm[i]] = {pb->lower[i], pb->upper[i]};
        }
        auto h = std::make_unique<HostHandle>();
        h->pm = std::make_unique<HipSEPAIHRDParameterManager>(mp, nm, sg, bd, split_lines(npi_names));
        h->pm->setConstraintMode(pb->constraint_mode == SEPAIHRD_CONSTRAINT_REFLECT ? ConstraintMode::MCMC_REFLECT
                                                                                   : ConstraintMode::OPTIMIZATION_CLAMP);
        h->cache = std::make_unique<SimulationCache>(static_cast<size_t>(cache_capacity > 0 ? cache_capacity : 1000));
        if (!with_objective) return h.release();
        h->data = std::make_unique<CalibrationData>(calibration_data(pb, mp.N));
        const std::shared_ptr<IOdeSolverStrategy> solver = strategy_for(pb->solver);
        h->obj = std::make_unique<HipSEPAIHRDObjectiveFunction>(
            *h->pm, *h->cache, *h->data, std::vector<double>(pb->times, pb->times + pb->n_times),
            vec(pb->initial_state, 11 * n), solver, pb->abs_err, pb->rel_err, device, pb->arith == SEPAIHRD_ARITH_FMA);
        return h.release();
    } catch (const std::exception& e) {
        g_error = e.what();
        return nullptr;
    }
}

void host_objective_destroy(void* hv) { delete static_cast<HostHandle*>(hv); }

// HipPosteriorEnsemble over the handle's parameter manager / data.  samples: n_samples x P.
// ppc: [6 series][5: lower_95, lower_90, median, upper_90, upper_95][T_pos][n]; selected: capacity
// max(n_samples, num_for_ppc) indices actually simulated; sero / rt (nullable): [5: q025,q05,median,q95,q975][T]
// over samples burn_in, burn_in + thinning, ...
int host_ensemble(void* hv, const sepaihrd_problem* pb, int device, const double* samples, int n_samples,
                  int num_for_ppc, uint32_t seed, double* ppc, int32_t* selected, int32_t* n_selected,
                  int32_t* samples_used, int burn_in, int thinning, double* sero, double* rt) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int n = pb->n_age;
        const std::vector<double> times(pb->times, pb->times + pb->n_times);
        HipPosteriorEnsemble ens = posterior_over<HipPosteriorEnsemble>(*h, pb, device);
        const std::vector<Eigen::VectorXd> ps = sample_vectors(samples, n_samples, h->pm->getParameterCount());
        const std::vector<int> sel = HipPosteriorEnsemble::selectSamples(ps.size(), num_for_ppc, seed);
        for (size_t i = 0; i < sel.size(); ++i) selected[i] = sel[i];
        *n_selected = static_cast<int32_t>(sel.size());
        const PosteriorPredictiveData d = ens.aggregatePosteriorPredictives(ps, num_for_ppc, seed);
        *samples_used = d.samples_used;
        const PosteriorPredictiveData::IncidenceData* series[6] = {&d.daily_hospitalizations, &d.daily_icu_admissions,
                                                                   &d.daily_deaths, &d.cumulative_hospitalizations,
                                                                   &d.cumulative_icu_admissions, &d.cumulative_deaths};
        const size_t Tp = d.time_points.size();
        for (int ser = 0; ser < 6; ++ser) {
            const Eigen::MatrixXd* m[5] = {&series[ser]->lower_95, &series[ser]->lower_90, &series[ser]->median,
                                           &series[ser]->upper_90, &series[ser]->upper_95};
            for (int q = 0; q < 5; ++q)
                for (size_t t = 0; t < Tp; ++t)
                    for (int a = 0; a < n; ++a)
                        ppc[((static_cast<size_t>(ser) * 5 + q) * Tp + t) * n + a] =
                            (*m[q])(static_cast<Eigen::Index>(t), a);
        }
        if (sero) put_quantile_rows(ens.aggregateSeroprevalence(ps, burn_in, thinning), times, sero);
        if (rt) put_quantile_rows(ens.aggregateRt(ps, burn_in, thinning), times, rt);
    });
}

// PostCalibrationAnalyser::generateFullReport step 4 as the reference runs it (PostCalibrationAnalyser.cpp:94-141,210-219): the
// baseline is the LAST analysed sample (burn_in, burn_in + thinning, ...) after the constraints -- the parameters the batch loop
// left in the model template -- and the default lockdown scenarios.  Writes scenario_comparison.csv to path (if not null);
// metrics [n_rows][12 + 4 n] and kappa [n_rows][n_kappa] (nullable, capacity 3 rows) receive the rows.
int host_scenario_comparison(void* hv, const sepaihrd_problem* pb, int device, const double* samples, int n_samples, int burn_in,
                             int thinning, const char* path, double* metrics, double* kappa, int32_t* n_rows) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        *n_rows = 0;
        if (n_samples <= 0 || burn_in >= n_samples || thinning <= 0) return;  // nothing selected: no rows, no file, no error
        const int n = pb->n_age;
        const size_t P = h->pm->getParameterCount();
        HipPosteriorEnsemble ens = posterior_over<HipPosteriorEnsemble>(*h, pb, device);
        int last = burn_in;
        while (last + thinning < n_samples) last += thinning;
        const Eigen::VectorXd baseline = vec(samples + static_cast<size_t>(last) * P, static_cast<int>(P));
        const auto rows = ens.performScenarioAnalysis(baseline, HipPosteriorEnsemble::defaultLockdownScenarios(*h->pm));
        if (path) HipPosteriorEnsemble::writeScenarioComparison(path, rows);
        const size_t W = static_cast<size_t>(12 + 4 * n), nk = h->pm->modelParameters().kappa_values.size();
        for (size_t r = 0; r < rows.size(); ++r) {
            const EssentialMetrics& m = rows[r].second;
            if (metrics) {
                double* o = metrics + r * W;
                const double head[12] = {m.R0, m.overall_IFR, m.overall_attack_rate, m.peak_hospital_occupancy, m.peak_ICU_occupancy,
                                         m.time_to_peak_hospital, m.time_to_peak_ICU, m.total_cumulative_deaths, m.max_Rt, m.min_Rt,
                                         m.final_Rt, m.seroprevalence_at_target_day};
                for (int c = 0; c < 12; ++c) o[c] = head[c];
                for (int a = 0; a < n; ++a) {
                    o[12 + 4 * a + 0] = m.age_specific_IFR[static_cast<size_t>(a)];
                    o[12 + 4 * a + 1] = m.age_specific_IHR[static_cast<size_t>(a)];
                    o[12 + 4 * a + 2] = m.age_specific_IICUR[static_cast<size_t>(a)];
                    o[12 + 4 * a + 3] = m.age_specific_attack_rate[static_cast<size_t>(a)];
                }
            }
            if (kappa)
                for (size_t i = 0; i < nk; ++i) {
                    const auto it = m.kappa_values.find("kappa_" + std::to_string(i + 1));
                    kappa[r * nk + i] = it == m.kappa_values.end() ? std::numeric_limits<double>::quiet_NaN() : it->second;
                }
        }
        *n_rows = static_cast<int32_t>(rows.size());
    });
}

// seroprevalence/ene_covid_validation.csv from the metric summary of samples burn_in, burn_in + thinning, ...
// (PostCalibrationAnalyser.cpp:288-299)
int host_ene_covid_validation(void* hv, const sepaihrd_problem* pb, int device, const double* samples, int n_samples, int burn_in,
                              int thinning, const char* path) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        HipPosteriorEnsemble ens = posterior_over<HipPosteriorEnsemble>(*h, pb, device);
        const std::vector<Eigen::VectorXd> ps = sample_vectors(samples, n_samples, h->pm->getParameterCount());
        HipPosteriorEnsemble::writeEneCovidValidation(path, HipPosteriorEnsemble::aggregateMetrics(ens.calculateEssentialMetrics(ps, burn_in, thinning)));
    });
}

// returns 0 ok, 1 = exception thrown by calculate() (message in host_last_error)
int host_objective_calculate(void* hv, const double* theta, double* value) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        *value = h->obj->calculate(vec(theta, static_cast<int>(h->pm->getParameterCount())));
    });
}

int host_objective_calculate_batch(void* hv, const double* thetas, int B, double* out, int* status) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        h->obj->calculateBatch(thetas, B, out, status);
    });
}

// HipSEPAIHRDObjectiveFunction::setDispersion on the handle's objective; 0 ok, 1 = refused (message in host_last_error)
int host_objective_set_dispersion(void* hv, const double* k) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        h->obj->setDispersion(k);
        std::copy(k, k + 3, h->dispersion);
        h->has_dispersion = true;
    });
}

void host_cache_stats(void* hv, long* calls, long* hits, long* size) {
    auto* h = static_cast<HostHandle*>(hv);
    *calls = static_cast<long>(h->cache->getLikelihoodCalls());
    *hits = static_cast<long>(h->cache->getLikelihoodHits());
    *size = static_cast<long>(h->cache->size());
}

int host_apply_constraints(void* hv, int mode, const double* in, double* out) {
    auto* h = static_cast<HostHandle*>(hv);
    const ConstraintModeScope in_mode(*h->pm, mode);
    const int P = static_cast<int>(h->pm->getParameterCount());
    const Eigen::VectorXd c = h->pm->applyConstraints(vec(in, P));
    for (int i = 0; i < P; ++i) out[i] = c[i];
    return 0;
}

int host_current_parameters(void* hv, double* out) {
    auto* h = static_cast<HostHandle*>(hv);
    const Eigen::VectorXd c = h->pm->getCurrentParameters();
    for (Eigen::Index i = 0; i < c.size(); ++i) out[i] = c[i];
    return 0;
}

// C chains of Adaptive Metropolis through the batched objective.  Outputs per chain:
// accepted[C], best_value[C], best[C*P], final_scale[C], accept_trace[C*(iterations-1)],
// n_samples (same for all chains), samples[C*n_samples*P], sample_values[C*n_samples].
int host_mh_run(void* hv, int C, const double* initial, uint32_t seed, int iterations, int burn_in,
                int adaptation_period, int thinning, double reg_eps, double target_acc, int adapt_scale,
                int use_scalar_interface, int32_t* accepted, double* best_value, double* best, double* final_scale,
                unsigned char* accept_trace, int32_t* n_samples, double* samples, double* sample_values,
                int two_pass_covariance, double* final_cov, int adaptation_window, int device_streams) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        MultiChainMetropolisHastings mh;
        mh.configure(mh_settings(iterations, burn_in, false, 0,
                                 {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)},
                                  {"regularization_epsilon", reg_eps}, {"target_acceptance_rate", target_acc},
                                  {"adapt_scale", double(adapt_scale)}, {"store_samples", 1.0},
                                  {"two_pass_covariance", double(two_pass_covariance)}, {"adaptation_window", double(adaptation_window)},
                                  {"device_streams", double(device_streams)}, {"keep_accept_traces", accept_trace ? 1.0 : 0.0},
                                  {"compute_diagnostics", h->mh_diagnostics ? 1.0 : 0.0}}));
        h->last_diag = ChainDiagnosticsTable{};
        const MhChainsOut out{iterations, P, accepted, best_value, best, final_scale, accept_trace, n_samples, samples, sample_values, final_cov};
        if (use_scalar_interface == 1) {  // one chain at a time: no lock-step loop to time, no table of the chains
            mh_scalar_chains(mh, C, initial, seed, *h->obj, *h->pm, out);
            return;
        }
        mh.setSeed(seed);
        const std::vector<double> init(initial, initial + static_cast<size_t>(C) * P);
        out.put(use_scalar_interface == 2 ? mh.optimizeChainsOnDevice(init, C, *h->obj, *h->pm)  // device-resident state
                                          : mh.optimizeChains(init, C, *h->obj, *h->pm),
                mh.acceptTraces());
        g_last_mh_loop_seconds = mh.lastLoopSeconds();
        h->last_diag = mh.diagnostics();
        g_last_diag_seconds = mh.lastDiagnosticsSeconds();
    });
}

// BatchedHillClimbingOptimizer in the clamp mode ModelCalibrator sets for phase 1
// (ModelCalibrator.cpp:62-66).  use_scalar_interface hides calculateBatch from the optimizer, so that
// every objective value comes from IObjectiveFunction::calculate (one launch per value).
int host_hc_run(void* hv, const double* x0, uint32_t seed, int threads, int iterations, int cloud_size_multiplier,
                int use_scalar_interface, double* best, double* best_value, double* final_cov, double* trace,
                long* evaluations, long* launches) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        h->pm->setConstraintMode(ConstraintMode::OPTIMIZATION_CLAMP);
        BatchedHillClimbingOptimizer hc;
        hc.configure({{"iterations", double(iterations)}, {"cloud_size_multiplier", double(cloud_size_multiplier)},
                      {"threads", double(threads)}, {"seed", double(seed)}});
        struct ScalarOnly : IObjectiveFunction {
            IObjectiveFunction& inner;
            explicit ScalarOnly(IObjectiveFunction& o) : inner(o) {}
            double calculate(const Eigen::VectorXd& p) const override { return inner.calculate(p); }
            const std::vector<std::string>& getParameterNames() const override { return inner.getParameterNames(); }
        } scalar(*h->obj);
        const OptimizationResult r = use_scalar_interface ? hc.optimize(vec(x0, P), scalar, *h->pm)
                                                          : hc.optimize(vec(x0, P), *h->obj, *h->pm);
        for (int i = 0; i < P; ++i) best[i] = r.bestParameters[i];
        *best_value = r.bestObjectiveValue;
        for (int a = 0; a < P; ++a)
            for (int b = 0; b < P; ++b) final_cov[static_cast<size_t>(a) * P + b] = r.finalCovariance(a, b);
        if (trace) std::copy(hc.currentTrace().begin(), hc.currentTrace().end(), trace);
        if (evaluations) *evaluations = hc.evaluations();
        if (launches) *launches = hc.launches();
    });
}

// BatchedParticleSwarmOptimization.  settings: n_settings (key, value) pairs, keys as in pso_settings.txt plus `seed`.
int host_pso_run(void* hv, const double* x0, const char* const* keys, const double* values, int n_settings,
                 double* best, double* best_value, double* final_cov, double* trace, long* evaluations, long* launches) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        h->pm->setConstraintMode(ConstraintMode::OPTIMIZATION_CLAMP);
        std::map<std::string, double> settings;
        for (int i = 0; i < n_settings; ++i) settings[keys[i]] = values[i];
        BatchedParticleSwarmOptimization pso;
        pso.configure(settings);
        const OptimizationResult r = pso.optimize(x0 ? vec(x0, P) : Eigen::VectorXd(), *h->obj, *h->pm);
        for (int i = 0; i < P; ++i) best[i] = r.bestParameters[i];
        *best_value = r.bestObjectiveValue;
        if (final_cov)
            for (int a = 0; a < P; ++a)
                for (int b = 0; b < P; ++b) final_cov[static_cast<size_t>(a) * P + b] = r.finalCovariance(a, b);
        if (trace) std::copy(pso.bestTrace().begin(), pso.bestTrace().end(), trace);
        if (evaluations) *evaluations = pso.evaluations();
        if (launches) *launches = pso.launches();
    });
}

namespace {
void copy_calibration(const HipModelCalibrator& cal, int P, int mh_iterations, double* best, double* best_value,
                      double* initial_value, double* phase1_best_value, double* phase2_cov, unsigned char* accept_trace,
                      double* samples, double* sample_values, double* mcmc_objective_values, int32_t* n_samples) {
    for (int i = 0; i < P; ++i) best[i] = cal.getBestParameterVector()[i];
    *best_value = cal.getBestObjectiveValue();
    if (initial_value) *initial_value = cal.getInitialObjectiveValue();
    if (phase1_best_value) *phase1_best_value = cal.getPhase1Result().bestObjectiveValue;
    if (phase2_cov)
        for (int a = 0; a < P; ++a)
            for (int b = 0; b < P; ++b) phase2_cov[static_cast<size_t>(a) * P + b] = cal.getPhase2Covariance()(a, b);
    const MhChainsOut chains{mh_iterations, P, nullptr, nullptr, nullptr, nullptr, accept_trace, n_samples, samples, sample_values, nullptr};
    chains.put(cal.getPhase2Results(), cal.acceptTraces());
    if (mcmc_objective_values) std::copy(cal.getMCMCObjectiveValues().begin(), cal.getMCMCObjectiveValues().end(), mcmc_objective_values);
}
}  // namespace

// HipModelCalibrator: two-phase calibration.  Per-chain outputs are chain-major; n_samples is per chain.
int host_calibrate(void* hv, int hc_iterations, int cloud_size_multiplier, int threads, uint32_t hc_seed,
                   int mh_iterations, int burn_in, int adaptation_period, int thinning, uint32_t mh_seed, int chains,
                   double* best, double* best_value, double* initial_value, double* phase1_best_value,
                   double* phase2_cov, unsigned char* accept_trace, double* samples, double* sample_values,
                   double* mcmc_objective_values, int32_t* n_samples) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        h->pm->setConstraintMode(ConstraintMode::OPTIMIZATION_CLAMP);  // mode at construction time
        h->last_diag = ChainDiagnosticsTable{};
        HipModelCalibrator cal(*h->pm, *h->obj);
        cal.calibrate({{"iterations", double(hc_iterations)}, {"cloud_size_multiplier", double(cloud_size_multiplier)},
                       {"threads", double(threads)}, {"seed", double(hc_seed)}},
                      mh_settings(mh_iterations, burn_in, false, 0,
                                  {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)}, {"seed", double(mh_seed)},
                                   {"store_samples", 1.0}, {"compute_diagnostics", h->mh_diagnostics ? 1.0 : 0.0}}),
                      chains);
        h->last_diag = cal.diagnostics();
        copy_calibration(cal, P, mh_iterations, best, best_value, initial_value, phase1_best_value, phase2_cov, accept_trace,
                         samples, sample_values, mcmc_objective_values, n_samples);
    });
}

// SEPAIHRDModelCalibration::runPSOMCMC (SEPAIHRDModelCalibration.cpp:179-208): phase 1 = particle swarm.
int host_calibrate_pso(void* hv, const char* const* keys, const double* values, int n_settings, int mh_iterations,
                       int burn_in, int adaptation_period, int thinning, uint32_t mh_seed, int chains, double* best,
                       double* best_value, double* initial_value, double* phase1_best_value, double* phase2_cov,
                       unsigned char* accept_trace, double* samples, double* sample_values,
                       double* mcmc_objective_values, int32_t* n_samples) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        h->pm->setConstraintMode(ConstraintMode::OPTIMIZATION_CLAMP);
        std::map<std::string, double> phase1;
        for (int i = 0; i < n_settings; ++i) phase1[keys[i]] = values[i];
        h->last_diag = ChainDiagnosticsTable{};
        HipModelCalibrator cal(*h->pm, *h->obj);
        cal.setPhase1Algorithm(std::make_unique<BatchedParticleSwarmOptimization>());
        cal.calibrate(phase1,
                      mh_settings(mh_iterations, burn_in, false, 0,
                                  {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)}, {"seed", double(mh_seed)},
                                   {"store_samples", 1.0}, {"compute_diagnostics", h->mh_diagnostics ? 1.0 : 0.0}}),
                      chains);
        h->last_diag = cal.diagnostics();
        copy_calibration(cal, P, mh_iterations, best, best_value, initial_value, phase1_best_value, phase2_cov, accept_trace,
                         samples, sample_values, mcmc_objective_values, n_samples);
    });
}

// Convergence diagnostics (HipChainDiagnostics).  set_mh_diagnostics: host_mh_run (device-resident state), host_calibrate
// and host_calibrate_pso form the table of their chains (settings key compute_diagnostics); mh_diagnostics serves the last
// one: *rows = its rows (0: none), out [rows][7] when not NULL.  chain_diagnostics: over host draws samples [C][N][P] (+
// values [C][N] or NULL) on the handle's device, out [P + (values != NULL)][7], max_lag [..][4] or NULL.  0 ok, 1 error.
// wall time of sepaihrd_mh_diagnostics in this thread's last host_mh_run (seconds)
double host_last_mh_diagnostics_seconds(void) { return g_last_diag_seconds; }

void host_set_mh_diagnostics(void* hv, int on) { static_cast<HostHandle*>(hv)->mh_diagnostics = on != 0; }

int host_mh_diagnostics(void* hv, double* out, int32_t* rows) {
    const ChainDiagnosticsTable& t = static_cast<HostHandle*>(hv)->last_diag;
    if (rows) *rows = t.rows;
    if (out) std::copy(t.values.begin(), t.values.end(), out);
    return 0;
}

int host_chain_diagnostics(void* hv, const double* samples, const double* values, int C, int N, int P, double* out, int32_t* max_lag) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        if (!h->obj) throw InvalidParameterException("host_chain_diagnostics", "the handle has no objective (device context)");
        if (C < 1 || N < 1 || P < 1) throw InvalidParameterException("host_chain_diagnostics", "need C, N, P >= 1");
        std::vector<std::vector<Eigen::VectorXd>> chains(static_cast<size_t>(C));
        std::vector<std::vector<double>> vals;
        for (int c = 0; c < C; ++c)
            for (int n = 0; n < N; ++n) chains[static_cast<size_t>(c)].push_back(vec(samples + (static_cast<size_t>(c) * N + n) * P, P));
        if (values)
            for (int c = 0; c < C; ++c) vals.emplace_back(values + static_cast<size_t>(c) * N, values + static_cast<size_t>(c + 1) * N);
        const ChainDiagnosticsTable t = HipChainDiagnostics::compute(*h->obj, chains, vals);
        std::copy(t.values.begin(), t.values.end(), out);
        if (max_lag) std::copy(t.max_lag.begin(), t.max_lag.end(), max_lag);
    });
}

// HipSEPAIHRDGradientObjectiveFunction::evaluate_with_gradient over the handle's parameter manager / data.
// returns 0 ok, 1 = exception (message in host_last_error)
int host_gradient(void* hv, const sepaihrd_problem* pb, int device, const double* theta, double epsilon, double* value,
                  double* grad) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int n = pb->n_age;
        const int P = static_cast<int>(h->pm->getParameterCount());
        const std::shared_ptr<IOdeSolverStrategy> solver = strategy_for(pb->solver);
        SimulationCache cache(16);
        HipSEPAIHRDGradientObjectiveFunction obj(*h->pm, cache, *h->data, std::vector<double>(pb->times, pb->times + pb->n_times),
                                                 vec(pb->initial_state, 11 * n), solver, pb->abs_err, pb->rel_err, device,
                                                 pb->arith == SEPAIHRD_ARITH_FMA);
        obj.epsilon_ = epsilon;
        if (h->has_dispersion) obj.setDispersion(h->dispersion);
        Eigen::VectorXd g;
        IGradientObjectiveFunction& iface = obj;  // through the interface NUTS uses (NUTSSampler.cpp:80)
        *value = iface.evaluate_with_gradient(vec(theta, P), g);
        for (int i = 0; i < P; ++i) grad[i] = g[i];
    });
}

// HipNUTSSampler over a HipSEPAIHRDGradientObjectiveFunction built on the handle's parameter manager / data
// (SEPAIHRDModelCalibration::runNUTS runs it as phase 2: MCMC_REFLECT).  Outputs as oracle_nuts; returns the number
// of samples, or -1 on an exception (message in host_last_error).
int host_nuts_run(void* hv, const sepaihrd_problem* pb, int device, int iterations, int adaptation_window, double delta_target,
                  int max_tree_depth, double fd_epsilon, int constraint_mode, const double* theta0, uint32_t seed,
                  double* samples, double* values, double* eps_trace, int32_t* depth_trace, double* best, double* best_value,
                  long* gradient_calls, long* gradient_launches) {
    auto* h = static_cast<HostHandle*>(hv);
    int ns = 0;
    return guarded([&] {
        const int n = pb->n_age;
        const int P = static_cast<int>(h->pm->getParameterCount());
        h->pm->setConstraintMode(constraint_mode == 0 ? ConstraintMode::OPTIMIZATION_CLAMP : ConstraintMode::MCMC_REFLECT);
        const std::shared_ptr<IOdeSolverStrategy> solver = strategy_for(pb->solver);
        SimulationCache cache(1000);
        HipSEPAIHRDGradientObjectiveFunction obj(*h->pm, cache, *h->data, std::vector<double>(pb->times, pb->times + pb->n_times),
                                                 vec(pb->initial_state, 11 * n), solver, pb->abs_err, pb->rel_err, device,
                                                 pb->arith == SEPAIHRD_ARITH_FMA);
        obj.epsilon_ = fd_epsilon;
        if (h->has_dispersion) obj.setDispersion(h->dispersion);
        HipNUTSSampler nuts;
        nuts.configure({{"nuts_iterations", double(iterations)}, {"nuts_adaptation_window", double(adaptation_window)},
                        {"nuts_delta_target", delta_target}, {"nuts_max_tree_depth", double(max_tree_depth)},
                        {"seed", double(seed)}});
        IObjectiveFunction& iface = static_cast<HipSEPAIHRDObjectiveFunction&>(obj);
        const OptimizationResult r = nuts.optimize(vec(theta0, P), iface, *h->pm);
        ns = static_cast<int>(r.samples.size());
        for (int s = 0; s < ns; ++s) {
            for (int i = 0; i < P; ++i) samples[static_cast<size_t>(s) * P + i] = r.samples[static_cast<size_t>(s)][i];
            values[s] = r.sampleObjectiveValues[static_cast<size_t>(s)];
            eps_trace[s] = nuts.epsilonTrace()[static_cast<size_t>(s)];
            depth_trace[s] = nuts.depthTrace()[static_cast<size_t>(s)];
        }
        if (r.bestParameters.size() == P)
            for (int i = 0; i < P; ++i) best[i] = r.bestParameters[i];
        *best_value = r.bestObjectiveValue;
        if (gradient_calls) *gradient_calls = nuts.gradientCalls();
        if (gradient_launches) *gradient_launches = nuts.gradientLaunches();
    }) ? -1 : ns;
}

// MultiChainNUTSSampler over the handle's finite-difference objective: C chains in lock step, chain c from theta0[c] with
// std::mt19937(seed0 + c); the other arguments as host_nuts_run.  Outputs have a leading chain axis (see NutsChainsOut).
// stats [6]: ticks, rows evaluated, seconds of the whole run, seconds inside the batched evaluations, milliseconds of the
// evaluation kernels of the centre and of the perturbed context (0 unless kernel_timing).  Returns 0, or -1 on an
// exception (message in host_last_error).
int host_nuts_chains_run(void* hv, const sepaihrd_problem* pb, int device, int iterations, int adaptation_window, double delta_target,
                         int max_tree_depth, double fd_epsilon, int constraint_mode, int C, const double* theta0, uint32_t seed0,
                         int kernel_timing, double* samples, double* values, double* eps_trace, int32_t* depth_trace, int32_t* n_samples,
                         double* best, double* best_value, int64_t* gradient_calls, int64_t* rows_evaluated, int32_t* failure_status,
                         int32_t* failure_iteration, double* stats) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int n = pb->n_age;
        const int P = static_cast<int>(h->pm->getParameterCount());
        h->pm->setConstraintMode(constraint_mode == 0 ? ConstraintMode::OPTIMIZATION_CLAMP : ConstraintMode::MCMC_REFLECT);
        SimulationCache cache(16);  // the constructor's argument; the lock-step run never consults it
        HipSEPAIHRDGradientObjectiveFunction obj(*h->pm, cache, *h->data, std::vector<double>(pb->times, pb->times + pb->n_times),
                                                 vec(pb->initial_state, 11 * n), strategy_for(pb->solver), pb->abs_err, pb->rel_err,
                                                 device, pb->arith == SEPAIHRD_ARITH_FMA);
        obj.epsilon_ = fd_epsilon;
        if (h->has_dispersion) obj.setDispersion(h->dispersion);
        TimedRows rows(obj, kernel_timing != 0);
        MultiChainNUTSSampler nuts;
        nuts.configure(nuts_settings(iterations, adaptation_window, delta_target, max_tree_depth, seed0));
        const auto t0 = std::chrono::steady_clock::now();
        const MultiChainNUTSResult r = nuts.run(chain_starts(theta0, C, P), rows, *h->pm);
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const NutsChainsOut out{iterations, P, samples, values, eps_trace, depth_trace, n_samples, best, best_value,
                                gradient_calls, rows_evaluated, failure_status, failure_iteration};
        for (int c = 0; c < C; ++c) out.put(c, r.chains[static_cast<size_t>(c)]);
        const double st[6] = {double(r.ticks), double(r.rows_total), seconds, rows.call_seconds, rows.centre_ms, rows.perturbed_ms};
        if (stats) std::copy(st, st + 6, stats);
    }) ? -1 : 0;
}

// Test hook (no GPU): the same sampler over AnalyticGaussian (dimension D, mean [D], precision [D][D] row-major, optional
// failure ball).  lock_step != 0: MultiChainNUTSSampler; 0: chain by chain through HipNUTSSampler with seed0 + c on the
// same objective -- a chain whose evaluation fails there loses its samples with the exception (failure_status 2,
// n_samples 0; rows_evaluated = its launches otherwise).  stats [6] as host_nuts_chains_run, the clocks 0.
int host_nuts_chains_analytic(int D, const double* mean, const double* precision, double sigma, const double* fail_centre,
                              double fail_radius, int lock_step, int iterations, int adaptation_window, double delta_target,
                              int max_tree_depth, int C, const double* theta0, uint32_t seed0, double* samples, double* values,
                              double* eps_trace, int32_t* depth_trace, int32_t* n_samples, double* best, double* best_value,
                              int64_t* gradient_calls, int64_t* rows_evaluated, int32_t* failure_status, int32_t* failure_iteration,
                              double* stats) {
    return guarded([&] {
        AnalyticGaussian obj(D, mean, precision, fail_centre, fail_radius);
        FreeManager pm(D, sigma);
        const NutsChainsOut out{iterations, D, samples, values, eps_trace, depth_trace, n_samples, best, best_value,
                                gradient_calls, rows_evaluated, failure_status, failure_iteration};
        double st[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (lock_step) {
            MultiChainNUTSSampler nuts;
            nuts.configure(nuts_settings(iterations, adaptation_window, delta_target, max_tree_depth, seed0));
            const MultiChainNUTSResult r = nuts.run(chain_starts(theta0, C, D), obj, pm);
            for (int c = 0; c < C; ++c) out.put(c, r.chains[static_cast<size_t>(c)]);
            st[0] = double(r.ticks);
            st[1] = double(r.rows_total);
        } else {
            for (int c = 0; c < C; ++c) {
                NUTSChainResult one;
                HipNUTSSampler solo;
                solo.configure(nuts_settings(iterations, adaptation_window, delta_target, max_tree_depth, seed0 + static_cast<uint32_t>(c)));
                try {
                    const OptimizationResult r = solo.optimize(vec(theta0 + static_cast<size_t>(c) * D, D), obj, pm);
                    for (const Eigen::VectorXd& x : r.samples) one.samples.emplace_back(x.data(), x.data() + D);
                    one.sample_values = r.sampleObjectiveValues;
                    one.epsilon_trace = solo.epsilonTrace();
                    one.depth_trace = solo.depthTrace();
                    if (r.bestParameters.size() == D) one.best_parameters.assign(r.bestParameters.data(), r.bestParameters.data() + D);
                    one.best_value = r.bestObjectiveValue;
                } catch (const SimulationException&) {
                    one.failure_status = SEPAIHRD_STATUS_STEP_FAILURE;
                }
                one.gradient_calls = solo.gradientCalls();
                one.rows_evaluated = solo.gradientLaunches();
                out.put(c, one);
                st[1] += double(one.rows_evaluated);
            }
        }
        if (stats) std::copy(st, st + 6, stats);
    }) ? -1 : 0;
}

// Test hook (no GPU): the device's restatement of glibc's log (csrc/sepaihrd_rng.inc), compiled for the host
void host_glibc_log(const double* x, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = sepaihrd_rng::glibc_log(x[i]);
}

// the same for glibc's exp (the device's scale adaptation, exp(log_scale_))
void host_glibc_exp(const double* x, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = sepaihrd_rng::glibc_exp(x[i]);
}

// The device-resident sampler with the reference's reporting and trace files switched ON (MetropolisHastingsSampler.cpp:
// 363-383,399-411,440-469): progress lines into `log_path` (one per line), files into `dir`; device_streams = 0 draws on the
// host.  Outputs: every chain's samples [C][n_samples][P] and their values, *fell_back (the libm self-check refused the
// device streams), failure counts [3].
int host_mh_run_reported(void* hv, int C, const double* initial, uint32_t seed, int iterations, int burn_in, int adaptation_period,
                         int thinning, int report_interval, int checkpoint_chains, int device_state, int device_streams,
                         const char* dir, const char* log_path, double* samples, double* sample_values, int32_t* n_samples,
                         int* fell_back, long* failures) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        MultiChainMetropolisHastings mh;
        mh.configure(mh_settings(iterations, burn_in, true, report_interval,
                                 {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)},
                                  {"checkpoint_chains", double(checkpoint_chains)},  // as given: with 0 no chain reports or writes
                                  {"device_streams", double(device_streams)}, {"keep_accept_traces", 0.0}}));
        mh.setSeed(seed);
        mh.setOutputDirectory(dir ? dir : "");
        const ProgressLog log(mh, log_path);
        const std::vector<double> init(initial, initial + static_cast<size_t>(C) * P);
        const MhChainsOut out{iterations, P, nullptr, nullptr, nullptr, nullptr, nullptr, n_samples, samples, sample_values, nullptr};
        out.put(device_state ? mh.optimizeChainsOnDevice(init, C, *h->obj, *h->pm) : mh.optimizeChains(init, C, *h->obj, *h->pm), mh.acceptTraces());
        if (fell_back) *fell_back = mh.deviceStreamsFellBack() ? 1 : 0;
        put_failures(mh.failureCounts(), failures);  // not gated on device_state: what the sampler holds after either path
    });
}

// The host twin of sepaihrd_device_libm_check (no GPU): csrc/sepaihrd_rng.inc's log / exp compiled for the host, on the SAME
// fixed arguments, against this process's std::log / std::exp.  Counts of differing arguments.
void host_libm_selfcheck(int* n_args, int* n_log_diff, int* n_exp_diff) {
    int dl = 0, de = 0;
    for (int i = 0; i < sepaihrd_rng::LIBM_CHECK_N; ++i) {
        volatile double xl = sepaihrd_rng::libm_check_log_arg(i), xe = sepaihrd_rng::libm_check_exp_arg(i);
        const double a = sepaihrd_rng::glibc_log(xl), b = std::log(xl), c = sepaihrd_rng::glibc_exp(xe), d = std::exp(xe);
        if (std::memcmp(&a, &b, sizeof(double)) != 0) ++dl;
        if (std::memcmp(&c, &d, sizeof(double)) != 0) ++de;
    }
    if (n_args) *n_args = sepaihrd_rng::LIBM_CHECK_N;
    if (n_log_diff) *n_log_diff = dl;
    if (n_exp_diff) *n_exp_diff = de;
}
// the self-check arguments themselves (tests look at what they cover)
void host_libm_selfcheck_args(double* log_args, double* exp_args) {
    for (int i = 0; i < sepaihrd_rng::LIBM_CHECK_N; ++i) {
        log_args[i] = sepaihrd_rng::libm_check_log_arg(i);
        exp_args[i] = sepaihrd_rng::libm_check_exp_arg(i);
    }
}

// SEPAIHRD_ARITH_* the reference-shaped constructors select (environment SEPAIHRD_ARITH): what bench.py's default --arith
// must equal (tests/test_host_logic.py)
int host_default_arith() { return HipSEPAIHRDObjectiveFunction::defaultArithmeticIsFma() ? SEPAIHRD_ARITH_FMA : SEPAIHRD_ARITH_STRICT; }

// Pure host (no GPU): exact-sort quantiles across chains of every column of a summary table, out [n_probs][width].
int host_summary_quantiles(const double* table, int rows, int width, const double* probs, int n_probs, double* out) {
    return guarded([&] {
        const std::vector<double> q = MultiChainMetropolisHastings::summaryQuantiles(
            std::vector<double>(table, table + static_cast<size_t>(rows) * width), width, std::vector<double>(probs, probs + n_probs));
        std::copy(q.begin(), q.end(), out);
    });
}

// optimizeChainGroupsOnDevice with stored samples, then the all-gather of the per-chain summary records over the
// groups' devices.  records [C][2P+2] (host concatenation, chain order), gathered [G][C][2P+2] (what each group's device
// holds afterwards), samples [C][n_samples][P], best_value [C], accepted [C]; *backend_used: SEPAIHRD_GATHER_RCCL / _HOST.
int host_mh_groups_summaries(void** handles, int G, int C, const double* initial, uint32_t seed, int iterations, int burn_in,
                             int adaptation_period, int thinning, int backend, double* records, double* gathered, double* samples,
                             double* best_value, int32_t* accepted, int32_t* backend_used) {
    return guarded([&] {
        auto* h0 = static_cast<HostHandle*>(handles[0]);
        const int P = static_cast<int>(h0->pm->getParameterCount());
        const std::vector<HipSEPAIHRDObjectiveFunction*> objs = group_objectives(handles, G);
        MultiChainMetropolisHastings mh;
        mh.configure(mh_settings(iterations, burn_in, false, 0,
                                 {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)}, {"store_samples", 1.0}}));
        mh.setSeed(seed);
        const std::vector<OptimizationResult> res =
            mh.optimizeChainGroupsOnDevice(std::vector<double>(initial, initial + static_cast<size_t>(C) * P), C, objs, *h0->pm);
        const std::vector<double>& rec = mh.chainSummaries();
        if (records) std::copy(rec.begin(), rec.end(), records);
        const int used = mh.gatherChainSummaries(objs, backend);
        if (backend_used) *backend_used = used;
        if (gathered)
            for (int g = 0; g < G; ++g) {
                const std::vector<double> t = mh.gatheredSummaries(*objs[static_cast<size_t>(g)]);
                std::copy(t.begin(), t.end(), gathered + static_cast<size_t>(g) * rec.size());
            }
        // the traces are kept (the sampler's default) but no entry of this signature takes them
        const MhChainsOut out{iterations, P, accepted, best_value, nullptr, nullptr, nullptr, nullptr, samples, nullptr, nullptr};
        out.put(res, mh.acceptTraces());
    });
}

// optimizeChainGroupsOnDevice over G handles (one device context each; parameter manager of the first).
// Outputs as host_mh_run, without the samples.
int host_mh_run_groups(void** handles, int G, int C, const double* initial, uint32_t seed, int iterations, int burn_in,
                       int adaptation_period, int thinning, int32_t* accepted, double* best_value, double* best,
                       unsigned char* accept_trace) {
    return guarded([&] {
        auto* h0 = static_cast<HostHandle*>(handles[0]);
        const int P = static_cast<int>(h0->pm->getParameterCount());
        MultiChainMetropolisHastings mh;
        // keep_accept_traces stays at the sampler's default (on), with or without a destination for them
        mh.configure(mh_settings(iterations, burn_in, false, 0,
                                 {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)}, {"store_samples", 0.0}}));
        mh.setSeed(seed);
        const MhChainsOut out{iterations, P, accepted, best_value, best, nullptr, accept_trace, nullptr, nullptr, nullptr, nullptr};
        out.put(mh.optimizeChainGroupsOnDevice(std::vector<double>(initial, initial + static_cast<size_t>(C) * P), C, group_objectives(handles, G), *h0->pm),
                mh.acceptTraces());
        g_last_mh_loop_seconds = mh.lastLoopSeconds();
    });
}

// Test hook (no GPU): the scalar path of host_mh_run over AnalyticGaussian (dimension D, mean [D], precision [D][D] row-major)
// with FreeManager(sigma) -- chain c from initial[c] through optimize() with seed + c, through the settings builder and the
// output record of the entry points above.  Outputs as host_mh_run.
int host_mh_run_analytic(int D, const double* mean, const double* precision, double sigma, int C, const double* initial, uint32_t seed,
                         int iterations, int burn_in, int adaptation_period, int thinning, int32_t* accepted, double* best_value, double* best,
                         double* final_scale, unsigned char* accept_trace, int32_t* n_samples, double* samples, double* sample_values,
                         double* final_cov) {
    return guarded([&] {
        AnalyticGaussian obj(D, mean, precision, nullptr, 0.0);
        FreeManager pm(D, sigma);
        MultiChainMetropolisHastings mh;
        mh.configure(mh_settings(iterations, burn_in, false, 0,
                                 {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)},
                                  {"keep_accept_traces", accept_trace ? 1.0 : 0.0}}));
        const MhChainsOut out{iterations, D, accepted, best_value, best, final_scale, accept_trace, n_samples, samples, sample_values, final_cov};
        mh_scalar_chains(mh, C, initial, seed, obj, pm, out);
    });
}

}  // extern "C"

// The reference-shaped constructors (SEPAIHRDModelCalibration.cpp:84-118): model -> parameter manager -> objective,
// argument for argument, (a) with a HipSEPAIHRDParameterManager built from the model and (b) with an IParameterManager
// that is NOT one (forwards to a private manager: stands for the reference's own SEPAIHRDParameterManager), whose
// constraint mode is flipped behind the objective's back between evaluations.
// values: [2 managers][2 modes: clamp, reflect][B]; model_back: the calibrated entries read back from the MODEL after
// updateModelParameters(thetas[0]) in clamp mode, [P].
namespace {
class ForwardingManager : public IParameterManager {
public:
    explicit ForwardingManager(HipSEPAIHRDParameterManager& inner) : in_(inner) {}
    Eigen::VectorXd getCurrentParameters() const override { return in_.getCurrentParameters(); }
    void updateModelParameters(const Eigen::VectorXd& p) override { in_.updateModelParameters(p); }
    const std::vector<std::string>& getParameterNames() const override { return in_.getParameterNames(); }
    size_t getParameterCount() const override { return in_.getParameterCount(); }
    double getSigmaForParamIndex(int i) const override { return in_.getSigmaForParamIndex(i); }
    Eigen::VectorXd applyConstraints(const Eigen::VectorXd& p) const override { return in_.applyConstraints(p); }
    int getIndexForParam(const std::string& n) const override { return in_.getIndexForParam(n); }
    double getLowerBoundForParamIndex(int i) const override { return in_.getLowerBoundForParamIndex(i); }
    double getUpperBoundForParamIndex(int i) const override { return in_.getUpperBoundForParamIndex(i); }
    void setMode(ConstraintMode m) { in_.setConstraintMode(m); }
private:
    HipSEPAIHRDParameterManager& in_;
};
}  // namespace

extern "C" int host_reference_constructors(const sepaihrd_problem* pb, const char* names, const char* npi_names,
                                           const double* sigmas, const double* thetas, int B, double* values,
                                           double* model_back) {
    return guarded([&] {
        const int n = pb->n_age;
        SEPAIHRDParameters mp = model_parameters(pb);
        mp.kappa_end_times.clear();  // main.cpp:222-242: the schedule reaches the model through the NPI strategy
        mp.kappa_values.clear();
        const std::vector<std::string> nm = split_lines(names);
        std::map<std::string, double> sg;
        std::map<std::string, std::pair<double, double>> bd;
        for (size_t i = 0; i < nm.size(); ++i) {
            sg[nm[i]] = sigmas[i];
            bd[nm[i]] = {pb->lower[i], pb->upper[i]};
        }
        // the strategy takes the schedule after the baseline period
        auto npi = std::make_shared<PiecewiseConstantNpiStrategy>(
            std::vector<double>(pb->kappa_end_times + 1, pb->kappa_end_times + pb->n_kappa),
            std::vector<double>(pb->kappa_values + 1, pb->kappa_values + pb->n_kappa),
            std::map<std::string, std::pair<double, double>>{}, pb->kappa_values[0], pb->kappa_end_times[0], true,
            split_lines(npi_names));
        auto model = std::make_shared<AgeSEPAIHRDModel>(mp, npi);
        const CalibrationData data = calibration_data(pb, mp.N);
        const std::shared_ptr<IOdeSolverStrategy> solver = strategy_for(pb->solver);
        const std::vector<double> times(pb->times, pb->times + pb->n_times);
        const Eigen::VectorXd x0 = vec(pb->initial_state, 11 * n);
        const size_t P = nm.size();

        // (a) the two make_unique calls of setupCalibrator with the class names changed
        auto pm = std::make_unique<HipSEPAIHRDParameterManager>(model, nm, sg, bd);
        SimulationCache cache_a(4);
        auto objective = std::make_unique<HipSEPAIHRDObjectiveFunction>(model, *pm, cache_a, data, times, x0, solver,
                                                                         pb->abs_err, pb->rel_err);
        // (b) a manager of another type, mode changed without telling the objective
        HipSEPAIHRDParameterManager inner(model->getModelParameters(), nm, sg, bd, split_lines(npi_names));
        ForwardingManager foreign(inner);
        SimulationCache cache_b(4);
        HipSEPAIHRDObjectiveFunction objective_b(model, foreign, cache_b, data, times, x0, solver, pb->abs_err, pb->rel_err);
        for (int mode = 0; mode < 2; ++mode) {
            const ConstraintMode m = mode ? ConstraintMode::MCMC_REFLECT : ConstraintMode::OPTIMIZATION_CLAMP;
            pm->setConstraintMode(m);
            foreign.setMode(m);
            for (int b = 0; b < B; ++b) {
                const Eigen::VectorXd th = vec(thetas + static_cast<size_t>(b) * P, static_cast<int>(P));
                cache_a.clear();
                cache_b.clear();
                values[(0 * 2 + mode) * static_cast<size_t>(B) + b] = objective->calculate(th);
                values[(1 * 2 + mode) * static_cast<size_t>(B) + b] = objective_b.calculate(th);
            }
        }
        pm->setConstraintMode(ConstraintMode::OPTIMIZATION_CLAMP);
        pm->updateModelParameters(vec(thetas, static_cast<int>(P)));
        HipSEPAIHRDParameterManager readback(model, nm, sg, bd);  // reads the model the first manager wrote into
        const Eigen::VectorXd cur = readback.getCurrentParameters();
        for (size_t i = 0; i < P; ++i) model_back[i] = cur[static_cast<Eigen::Index>(i)];
    });
}

// Model-side holders without a device: kappa(t) of PiecewiseConstantNpiStrategy at nt times; the model's
// getModelParameters() schedule (baseline first), state size and first / last state names.
extern "C" int host_model_holders(const double* ends_after, const double* values_after, int n_after, double baseline,
                                  double baseline_end, const double* t, int nt, double* kappa_out, double* sched_ends,
                                  double* sched_values, int* state_size, char* first_last, int first_last_len) {
    try {
        auto npi = std::make_shared<PiecewiseConstantNpiStrategy>(std::vector<double>(ends_after, ends_after + n_after),
                                                                   std::vector<double>(values_after, values_after + n_after),
                                                                   std::map<std::string, std::pair<double, double>>{}, baseline,
                                                                   baseline_end);
        for (int i = 0; i < nt; ++i) kappa_out[i] = npi->getReductionFactor(t[i]);
        SEPAIHRDParameters mp;
        const int n = 3;
        mp.N = Eigen::VectorXd::Constant(n, 1000.0);
        mp.M_baseline = Eigen::MatrixXd::Identity(n, n);
        for (Eigen::VectorXd* v : {&mp.a, &mp.h_infec, &mp.p, &mp.h, &mp.icu, &mp.d_H, &mp.d_ICU}) *v = Eigen::VectorXd::Constant(n, 0.1);
        AgeSEPAIHRDModel model(mp, npi);
        const SEPAIHRDParameters back = model.getModelParameters();
        for (size_t k = 0; k < back.kappa_values.size(); ++k) { sched_ends[k] = back.kappa_end_times[k]; sched_values[k] = back.kappa_values[k]; }
        *state_size = model.getStateSize();
        const std::vector<std::string> names = model.getStateNames();
        std::snprintf(first_last, static_cast<size_t>(first_last_len), "%s %s %s %d", names.front().c_str(), names.back().c_str(),
                      npi->getNpiParamName(0).c_str(), static_cast<int>(model.clone()->getNumAgeClasses()));
        bool threw = false;
        try {
            std::vector<double> x(33, 0.0), dx(33, 0.0);
            model.computeDerivatives(x, dx, 0.0);
        } catch (const SimulationException&) { threw = true; }
        return threw ? 0 : 2;  // there is no host right-hand side
    } catch (const std::exception& e) {
        g_error = e.what();
        return 1;
    }
}

// ---- age-structured SIR: AgeSIRModel, HipSIRParameterManager, HipPoissonLikelihoodObjective (HipSIR.hpp) ----
namespace {
struct SirHandle {
    std::shared_ptr<AgeSIRModel> model;
    std::unique_ptr<HipSIRParameterManager> pm;
    std::unique_ptr<SimulationCache> cache;
    std::unique_ptr<HipPoissonLikelihoodObjective> obj;
    std::vector<double> times;  // the objective's output grid (host_sir_scenario_comparison)
};
std::shared_ptr<AgeSIRModel> sir_model(int n, const double* N, const double* C, const double* gamma, double q, double scale) {
    Eigen::MatrixXd Cm(n, n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Cm(i, j) = C[static_cast<size_t>(i) * n + j];  // row-major in
    return AgeSIRModel::create(vec(N, n), Cm, vec(gamma, n), q, scale);
}
}  // namespace

extern "C" {

// AgeSIRModel::computeDerivatives on the host (no device); C row-major.  0 ok, 1 = exception (host_last_error)
int host_sir_rhs(int n, const double* N, const double* C, const double* gamma, double q, double scale, const double* state, double* out) {
    return guarded([&] {
        auto m = sir_model(n, N, C, gamma, q, scale);
        std::vector<double> x(state, state + 3 * n), dx(static_cast<size_t>(3 * n));
        m->computeDerivatives(x, dx, 0.0);
        std::copy(dx.begin(), dx.end(), out);
    });
}

// names: '\n'-joined; sigma_names / sigma_values: n_sigmas explicit proposal sigmas (the rest take the defaults).
// with_objective = 0 builds model and parameter manager only (no device needed).  NULL + host_last_error on failure.
void* host_sir_create(const sepaihrd_sir_problem* pb, const char* names, const char* sigma_names, const double* sigma_values,
                      int device, int cache_capacity, int with_objective) {
    try {
        const int n = pb->n_age;
        auto h = std::make_unique<SirHandle>();
        h->model = sir_model(n, pb->N, pb->C, pb->gamma, pb->q, pb->scale_C_total);
        std::map<std::string, double> sg;
        const std::vector<std::string> sn = split_lines(sigma_names);
        for (size_t i = 0; i < sn.size(); ++i) sg[sn[i]] = sigma_values[i];
        h->pm = std::make_unique<HipSIRParameterManager>(h->model, split_lines(names), sg);
        h->cache = std::make_unique<SimulationCache>(static_cast<size_t>(cache_capacity > 0 ? cache_capacity : 1000));
        h->times.assign(pb->times, pb->times + pb->n_times);
        if (!with_objective) return h.release();
        Eigen::MatrixXd obs(pb->n_times, n);
        for (int r = 0; r < pb->n_times; ++r)
            for (int c = 0; c < n; ++c) obs(r, c) = pb->obs[static_cast<size_t>(r) * n + c];
        h->obj = std::make_unique<HipPoissonLikelihoodObjective>(
            h->model, *h->pm, *h->cache, obs, std::vector<double>(pb->times, pb->times + pb->n_times), vec(pb->initial_state, 3 * n),
            strategy_for(pb->solver), pb->dt_hint, pb->abs_err, pb->rel_err, device, pb->arith == SEPAIHRD_ARITH_FMA, pb->max_attempts);
        return h.release();
    } catch (const std::exception& e) {
        g_error = e.what();
        return nullptr;
    }
}

void host_sir_destroy(void* hv) { delete static_cast<SirHandle*>(hv); }

// sigma, lower and upper bound of every parameter; the manager's current parameters; 0 ok
int host_sir_manager_info(void* hv, double* sigmas, double* lower, double* upper, double* current) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        const Eigen::VectorXd cur = h->pm->getCurrentParameters();
        for (int i = 0; i < P; ++i) {
            sigmas[i] = h->pm->getSigmaForParamIndex(i);
            lower[i] = h->pm->getLowerBoundForParamIndex(i);
            upper[i] = h->pm->getUpperBoundForParamIndex(i);
            current[i] = cur[i];
        }
    });
}

int host_sir_index_for_param(void* hv, const char* name) { return static_cast<SirHandle*>(hv)->pm->getIndexForParam(name); }

int host_sir_apply_constraints(void* hv, const double* in, double* out) {
    auto* h = static_cast<SirHandle*>(hv);
    const int P = static_cast<int>(h->pm->getParameterCount());
    const Eigen::VectorXd c = h->pm->applyConstraints(vec(in, P));
    for (int i = 0; i < P; ++i) out[i] = c[i];
    return 0;
}

// updateModelParameters(theta), then the model's q, scale_C_total and gamma[n]; 0 ok, 1 = exception
int host_sir_update_model(void* hv, const double* theta, double* q, double* scale, double* gamma) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        h->pm->updateModelParameters(vec(theta, static_cast<int>(h->pm->getParameterCount())));
        *q = h->model->getTransmissibility();
        *scale = h->model->getContactScaleFactor();
        for (int i = 0; i < h->model->getNumAgeClasses(); ++i) gamma[i] = h->model->getRecoveryRate()[i];
    });
}

int host_sir_calculate(void* hv, const double* theta, double* value) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        *value = h->obj->calculate(vec(theta, static_cast<int>(h->pm->getParameterCount())));
    });
}

int host_sir_calculate_batch(void* hv, const double* thetas, int B, double* out, int* status) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        h->obj->calculateBatch(thetas, B, out, status);
    });
}

void host_sir_cache_stats(void* hv, long* calls, long* hits, long* size) {
    auto* h = static_cast<SirHandle*>(hv);
    *calls = static_cast<long>(h->cache->getLikelihoodCalls());
    *hits = static_cast<long>(h->cache->getLikelihoodHits());
    *size = static_cast<long>(h->cache->size());
}

// BatchedHillClimbingOptimizer on the SIR objective, unchanged
int host_sir_hc_run(void* hv, const double* x0, uint32_t seed, int threads, int iterations, int cloud_size_multiplier, double* best,
                    double* best_value) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        BatchedHillClimbingOptimizer hc;
        hc.configure({{"iterations", double(iterations)}, {"cloud_size_multiplier", double(cloud_size_multiplier)},
                      {"threads", double(threads)}, {"seed", double(seed)}});
        const OptimizationResult r = hc.optimize(vec(x0, P), *h->obj, *h->pm);
        for (int i = 0; i < P; ++i) best[i] = r.bestParameters[i];
        *best_value = r.bestObjectiveValue;
    });
}

// MultiChainMetropolisHastings::optimizeChains (the lock-step branch over any IBatchObjectiveFunction), unchanged:
// per chain best_value[C], best[C*P], accepted[C]
int host_sir_mh_run(void* hv, int C, const double* initial, uint32_t seed, int iterations, int burn_in, double* best_value, double* best,
                    int32_t* accepted) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        MultiChainMetropolisHastings mh;
        mh.configure(mh_settings(iterations, burn_in, false, 0, {{"store_samples", 0.0}}));  // adaptation and thinning: the sampler's defaults
        mh.setSeed(seed);
        const MhChainsOut out{iterations, P, accepted, best_value, best, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        out.put(mh.optimizeChains(std::vector<double>(initial, initial + static_cast<size_t>(C) * P), C, *h->obj, *h->pm), mh.acceptTraces());
    });
}

// The SIR sampler through EITHER path -- device_state = 0: the host loop optimizeChains above (every iteration through the
// host-pointer calculateBatch); 1: optimizeChainsOnDevice (sepaihrd_sir_mh_create) -- with what host_mh_run returns:
// accepted[C], best_value[C], best[C*P], final_scale[C], accept_trace[C*(iterations-1)] or NULL, n_samples, samples
// [C*n_samples*P], sample_values[C*n_samples], final_cov[C*P*P].  kernel_form: SEPAIHRD_MH_FORM_* (device_state only).
// dir != NULL switches the reference's progress reports and trace files on (lines into log_path, files into dir).
// fell_back: the libm self-check refused the device streams; failures[3]: evaluations the accept tests saw fail;
// diag_out [P + 1][7] with *diag_rows when compute_diagnostics (0 rows: no table).
int host_sir_mh_run_ex(void* hv, int C, const double* initial, uint32_t seed, int iterations, int burn_in, int adaptation_period, int thinning,
                       double reg_eps, double target_acc, int adapt_scale, int device_state, int device_streams, int two_pass_covariance,
                       int adaptation_window, int kernel_form, int compute_diagnostics, int report_interval, int checkpoint_chains,
                       const char* dir, const char* log_path, int32_t* accepted, double* best_value, double* best, double* final_scale,
                       unsigned char* accept_trace, int32_t* n_samples, double* samples, double* sample_values, double* final_cov,
                       int* fell_back, long* failures, double* diag_out, int32_t* diag_rows) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        const bool reported = dir != nullptr;
        MultiChainMetropolisHastings mh;
        mh.configure(mh_settings(iterations, burn_in, reported, report_interval,
                                 {{"checkpoint_chains", double(std::max(checkpoint_chains, 1))},  // at least chain 0
                                  {"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)},
                                  {"regularization_epsilon", reg_eps}, {"target_acceptance_rate", target_acc}, {"adapt_scale", double(adapt_scale)},
                                  {"store_samples", 1.0}, {"two_pass_covariance", double(two_pass_covariance)},
                                  {"adaptation_window", double(adaptation_window)}, {"device_streams", double(device_streams)},
                                  {"keep_accept_traces", accept_trace ? 1.0 : 0.0}, {"compute_diagnostics", compute_diagnostics ? 1.0 : 0.0},
                                  {"kernel_form", double(kernel_form)}}));
        mh.setSeed(seed);
        if (reported) mh.setOutputDirectory(dir);
        const ProgressLog log(mh, reported ? log_path : nullptr);
        const std::vector<double> init(initial, initial + static_cast<size_t>(C) * P);
        const MhChainsOut out{iterations, P, accepted, best_value, best, final_scale, accept_trace, n_samples, samples, sample_values, final_cov};
        out.put(device_state ? mh.optimizeChainsOnDevice(init, C, *h->obj, *h->pm) : mh.optimizeChains(init, C, *h->obj, *h->pm), mh.acceptTraces());
        g_last_mh_loop_seconds = mh.lastLoopSeconds();
        if (fell_back) *fell_back = mh.deviceStreamsFellBack() ? 1 : 0;
        // failure counts and the diagnostics table are the device-resident run's: the host loop reports none of either
        put_failures(device_state ? mh.failureCounts() : std::vector<long>(), failures);
        if (diag_rows) *diag_rows = device_state ? mh.diagnostics().rows : 0;
        if (diag_out && device_state) std::copy(mh.diagnostics().values.begin(), mh.diagnostics().values.end(), diag_out);
    });
}

// HipModelCalibrator on the SIR objective (CalibrationDemo.cpp's flow): Hill-Climbing, covariance conditioning, `chains`
// device-resident Metropolis-Hastings chains from the phase-1 optimum, the objective value of every stored sample.
// Outputs as host_calibrate.
int host_sir_calibrate(void* hv, int hc_iterations, int cloud_size_multiplier, int threads, uint32_t hc_seed, int mh_iterations, int burn_in,
                       int adaptation_period, int thinning, uint32_t mh_seed, int chains, int kernel_form, int device_streams, double* best,
                       double* best_value, double* initial_value, double* phase1_best_value, double* phase2_cov, unsigned char* accept_trace,
                       double* samples, double* sample_values, double* mcmc_objective_values, int32_t* n_samples) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        const int P = static_cast<int>(h->pm->getParameterCount());
        HipModelCalibrator cal(*h->pm, *h->obj);
        cal.calibrate({{"iterations", double(hc_iterations)}, {"cloud_size_multiplier", double(cloud_size_multiplier)},
                       {"threads", double(threads)}, {"seed", double(hc_seed)}},
                      mh_settings(mh_iterations, burn_in, false, 0,
                                  {{"adaptation_period", double(adaptation_period)}, {"thinning", double(thinning)}, {"seed", double(mh_seed)},
                                   {"store_samples", 1.0}, {"kernel_form", double(kernel_form)}, {"device_streams", double(device_streams)}}),
                      chains);
        copy_calibration(cal, P, mh_iterations, best, best_value, initial_value, phase1_best_value, phase2_cov, accept_trace, samples,
                         sample_values, mcmc_objective_values, n_samples);
    });
}

// ---- SIR scenario analysis (HipSIRScenarioAnalysis.hpp) ----
// One scenario built entry by entry through SIRScenario::addIntervention on the grid times[T]: entry e is (ev_times[e], the
// e-th line of names, n_params[e] values of params in sequence).  0 ok -- the events in schedule order in time_index / kind /
// value (room for n_entries) and their count in *n_events; 1 InvalidParameterException, 2 any other exception (message in
// host_last_error).  No device.
int host_sir_scenario_events(const double* times, int T, int n_entries, const double* ev_times, const char* names, const int* n_params,
                             const double* params, int32_t* time_index, int32_t* kind, double* value, int* n_events) {
    try {
        SIRScenario sc("scenario", std::vector<double>(times, times + T));
        const std::vector<std::string> nm = split_lines(names);
        if (static_cast<int>(nm.size()) != n_entries) throw ModelException("host_sir_scenario_events", "one name per entry expected");
        size_t at = 0;
        for (int e = 0; e < n_entries; ++e) {
            sc.addIntervention(ev_times[e], nm[static_cast<size_t>(e)], vec(params + at, n_params[e]));
            at += static_cast<size_t>(n_params[e]);
        }
        const auto& ev = sc.events();
        for (size_t e = 0; e < ev.size(); ++e) { time_index[e] = ev[e].time_index; kind[e] = ev[e].kind; value[e] = ev[e].value; }
        *n_events = static_cast<int>(ev.size());
        return 0;
    } catch (const InvalidParameterException& e) {
        g_error = e.what();
        return 1;
    } catch (const std::exception& e) {
        g_error = e.what();
        return 2;
    }
}

namespace {
std::vector<SIRScenario> sir_scenarios(const std::vector<double>& times, const char* scenario_names, int K, const int* counts, const double* ev_times,
                                       const char* ev_names, const double* ev_values) {
    const std::vector<std::string> sn = split_lines(scenario_names), en = split_lines(ev_names);
    if (static_cast<int>(sn.size()) != K) throw InvalidParameterException("host_sir_scenario_comparison", "one name per scenario expected");
    std::vector<SIRScenario> out;
    size_t at = 0;
    for (int k = 0; k < K; ++k) {
        out.emplace_back(sn[static_cast<size_t>(k)], times);
        for (int e = 0; e < counts[k]; ++e, ++at) out.back().addIntervention(ev_times[at], en.at(at), vec(ev_values + at, 1));
    }
    return out;
}
}  // namespace

// The two writers on a result given as arrays (no device): quantiles [K][3][n_probs][T][n_age + 1], metric_summary
// [K][W][2 + n_probs], diff_quantiles [K][W][n_probs].  A NULL path skips that file.  0 ok, 1 = exception.
int host_sir_write_scenario_csvs(const char* comparison_path, const char* bands_path, const char* scenario_names, int K, int n_age, int T,
                                 const double* times, const double* probs, int n_probs, const double* quantiles, const double* metric_summary,
                                 const double* diff_quantiles) {
    return guarded([&] {
        SIRScenarioResult r;
        r.scenario_names = split_lines(scenario_names);
        if (static_cast<int>(r.scenario_names.size()) != K) throw InvalidParameterException("host_sir_write_scenario_csvs", "one name per scenario expected");
        r.metric_names = HipSIRScenarioAnalysis::metricNames(n_age);
        r.probs.assign(probs, probs + n_probs);
        r.times.assign(times, times + T);
        r.n_age = n_age;
        const size_t W = r.metric_names.size();
        if (quantiles) r.quantiles.assign(quantiles, quantiles + static_cast<size_t>(K) * 3 * n_probs * T * (n_age + 1));
        if (metric_summary) r.metric_summary.assign(metric_summary, metric_summary + static_cast<size_t>(K) * W * (2 + n_probs));
        if (diff_quantiles) r.diff_quantiles.assign(diff_quantiles, diff_quantiles + static_cast<size_t>(K) * W * n_probs);
        if (comparison_path) HipSIRScenarioAnalysis::writeScenarioComparison(comparison_path, r);
        if (bands_path) HipSIRScenarioAnalysis::writePosteriorBands(bands_path, r);
    });
}

// HipSIRScenarioAnalysis::run on the handle's objective and both files.  Scenario k has counts[k] entries taken in sequence
// from ev_times / ev_names ('\n'-joined) / ev_values (one parameter each).  The outputs (any may be NULL) have the shapes
// of sepaihrd_sir_scenario_ensemble with S = the samples left after burn-in and thinning.  0 ok, 1 = exception.
int host_sir_scenario_comparison(void* hv, const double* samples, int n_samples, int burn_in, int thinning, const char* scenario_names, int K,
                                 const int* counts, const double* ev_times, const char* ev_names, const double* ev_values, const double* probs,
                                 int n_probs, const char* comparison_path, const char* bands_path, double* quantiles, double* metrics,
                                 double* metric_summary, double* diff_quantiles, int32_t* status, int32_t* n_valid) {
    auto* h = static_cast<SirHandle*>(hv);
    return guarded([&] {
        if (!h->obj) throw ModelException("host_sir_scenario_comparison", "the handle has no objective");
        const std::vector<double>& times = h->times;
        const HipSIRScenarioAnalysis analysis(*h->obj, times, h->model->getNumAgeClasses());
        const SIRScenarioResult r = analysis.run(samples, n_samples, burn_in, thinning,
                                                 sir_scenarios(times, scenario_names, K, counts, ev_times, ev_names, ev_values),
                                                 std::vector<double>(probs, probs + n_probs));
        if (comparison_path) HipSIRScenarioAnalysis::writeScenarioComparison(comparison_path, r);
        if (bands_path) HipSIRScenarioAnalysis::writePosteriorBands(bands_path, r);
        if (quantiles) std::copy(r.quantiles.begin(), r.quantiles.end(), quantiles);
        if (metrics) std::copy(r.metrics.begin(), r.metrics.end(), metrics);
        if (metric_summary) std::copy(r.metric_summary.begin(), r.metric_summary.end(), metric_summary);
        if (diff_quantiles) std::copy(r.diff_quantiles.begin(), r.diff_quantiles.end(), diff_quantiles);
        if (status) std::copy(r.status.begin(), r.status.end(), status);
        if (n_valid) std::copy(r.n_valid.begin(), r.n_valid.end(), n_valid);
    });
}

// ---- posterior predictive draws (HipPosteriorPredictive) ----
// the twin of sepaihrd_poisson_device and one variate of the sampler (no device)
void host_poisson_probe(uint64_t seed, const double* lambda, int count, double* out) { hostPoissonProbe(seed, lambda, count, out); }
double host_poisson_at(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, double lambda) { return hostPoisson(seed, c0, c1, c2, lambda); }

// hostPosteriorPredictive (no device): shapes as sepaihrd_ensemble_predictive, observed [3][T_pos][n_age] or NULL
int host_predictive_from_means(const double* means, const int32_t* status, const double* observed, int S, int R, int T_pos, int n_age,
                               uint64_t seed, const double* probs, int n_probs, double* pred_quantiles, double* pit, double* draws, char* err,
                               int errlen) {
    std::string error;
    const int rc = hostPosteriorPredictive(means, status, observed, S, R, T_pos, n_age, seed, probs, n_probs, pred_quantiles, pit, draws, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// the dispersed form (hostPosteriorPredictiveNB): k_used [S][3] next to means and status
int host_predictive_nb_from_means(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                                  int n_age, uint64_t seed, const double* probs, int n_probs, double* pred_quantiles, double* pit, double* draws,
                                  char* err, int errlen) {
    std::string error;
    const int rc = hostPosteriorPredictiveNB(means, status, k_used, observed, S, R, T_pos, n_age, seed, probs, n_probs, pred_quantiles, pit, draws, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}
// the gamma and negative-binomial samplers (no device): one variate, and the twins of sepaihrd_gamma_device / sepaihrd_nb_draw_device
double host_gamma_at(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, double shape) { return hostGamma(seed, c0, c1, c2, shape); }
double host_nb_draw_at(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, double mu, double k) { return hostNBDraw(seed, c0, c1, c2, mu, k); }
void host_gamma_probe(uint64_t seed, const double* shape, int count, double* out) { hostGammaProbe(seed, shape, count, out); }
void host_nb_draw_probe(uint64_t seed, const double* mu, const double* k, int count, double* out) { hostNBDrawProbe(seed, mu, k, count, out); }

// HipPosteriorPredictive::draw over the handle's parameter manager / data.  samples: n_samples x P, selected by the PPC rule
// (num_for_ppc, ppc_seed).  pred [6][n_probs][T_pos][n], pit [3][T_pos][n], observed [3][T_pos][n]; means / draws (nullable)
// [n_selected][3][T_pos][n] / [n_selected][R][3][T_pos][n]; selected and status: capacity max(n_samples, num_for_ppc).
// host_predictive_dispersed: the same with k_used (nullable; capacity as status, [n_selected][3]) and *dispersed = whether the draws
// ran through sepaihrd_ensemble_predictive_nb -- they do where the handle's objective is dispersed, through host_objective_set_dispersion
// or calibrated dispersion_* names.
int host_predictive_dispersed(void* hv, const sepaihrd_problem* pb, int device, const double* samples, int n_samples, int num_for_ppc,
                              uint32_t ppc_seed, int R, uint64_t seed, const double* probs, int n_probs, double* pred, double* pit, double* observed,
                              double* means, double* draws, double* k_used, int32_t* dispersed, int32_t* selected, int32_t* n_selected,
                              int32_t* status, int32_t* samples_used) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        HipPosteriorPredictive pp = posterior_over<HipPosteriorPredictive>(*h, pb, device);
        if (h->has_dispersion) pp.objective().setDispersion(h->dispersion);
        const std::vector<Eigen::VectorXd> ps = sample_vectors(samples, n_samples, h->pm->getParameterCount());
        const PosteriorPredictiveDraws d = pp.draw(ps, num_for_ppc, ppc_seed, R, seed, std::vector<double>(probs, probs + n_probs), means != nullptr,
                                                   draws != nullptr);
        std::copy(d.pred_quantiles.begin(), d.pred_quantiles.end(), pred);
        if (pit) std::copy(d.pit.begin(), d.pit.end(), pit);
        if (observed) {
            const std::vector<double> obs = pp.observed();
            std::copy(obs.begin(), obs.end(), observed);
        }
        if (means) std::copy(d.means.begin(), d.means.end(), means);
        if (draws) std::copy(d.draws.begin(), d.draws.end(), draws);
        if (k_used) std::copy(d.k_used.begin(), d.k_used.end(), k_used);
        if (dispersed) *dispersed = d.k_used.empty() ? 0 : 1;
        for (size_t i = 0; i < d.selected.size(); ++i) selected[i] = d.selected[i];
        *n_selected = static_cast<int32_t>(d.selected.size());
        if (status) std::copy(d.status.begin(), d.status.end(), status);
        *samples_used = d.samples_used;
    });
}

int host_predictive(void* hv, const sepaihrd_problem* pb, int device, const double* samples, int n_samples, int num_for_ppc, uint32_t ppc_seed,
                    int R, uint64_t seed, const double* probs, int n_probs, double* pred, double* pit, double* observed, double* means,
                    double* draws, int32_t* selected, int32_t* n_selected, int32_t* status, int32_t* samples_used) {
    return host_predictive_dispersed(hv, pb, device, samples, n_samples, num_for_ppc, ppc_seed, R, seed, probs, n_probs, pred, pit, observed, means,
                                     draws, nullptr, nullptr, selected, n_selected, status, samples_used);
}

// ---- scores of the posterior predictive draws (sepaihrd_ensemble_predictive_scores) ----
// hostPosteriorPredictiveScores (no device): shapes as sepaihrd_ensemble_predictive_scores; k_used NULL: Poisson draws
int host_predictive_scores_from_means(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R,
                                      int T_pos, int n_age, uint64_t seed, const double* probs, int n_probs, const double* levels, int n_levels,
                                      double* pred_quantiles, double* pit, double* cell_scores, double* summary, double* draws, int32_t* exact,
                                      char* err, int errlen) {
    std::string error;
    const int rc = hostPosteriorPredictiveScores(means, status, k_used, observed, S, R, T_pos, n_age, seed, probs, n_probs, levels, n_levels,
                                                 pred_quantiles, pit, cell_scores, summary, draws, exact, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// hostScoreCell (no device): one unsorted sample x [m] against y; scores [5 + 4 n_levels]
int host_score_cell(const double* x, int m, double y, const double* levels, int n_levels, double* scores, double* pit, int32_t* exact, char* err,
                    int errlen) {
    std::string error;
    const int rc = hostScoreCell(x, m, y, levels, n_levels, scores, pit, exact, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// HipPosteriorPredictive::score over the handle's parameter manager / data, as host_predictive_dispersed drives draw():
// observed_in [3][T_pos][n] (nullable: the handle's data), cell_scores [3][T_pos][n][5 + 4 L], summary [3][n + 1][4 + 2 L]
int host_predictive_scores(void* hv, const sepaihrd_problem* pb, int device, const double* samples, int n_samples, int num_for_ppc,
                           uint32_t ppc_seed, int R, uint64_t seed, const double* probs, int n_probs, const double* levels, int n_levels,
                           const double* observed_in, double* pred, double* pit, double* cell_scores, double* summary, double* means, double* draws,
                           double* k_used, int32_t* exact, int32_t* selected, int32_t* n_selected, int32_t* status, int32_t* samples_used) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        HipPosteriorPredictive pp = posterior_over<HipPosteriorPredictive>(*h, pb, device);
        if (h->has_dispersion) pp.objective().setDispersion(h->dispersion);
        const std::vector<Eigen::VectorXd> ps = sample_vectors(samples, n_samples, h->pm->getParameterCount());
        std::vector<double> obs;
        if (observed_in) obs.assign(observed_in, observed_in + pp.observed().size());
        const PosteriorPredictiveScores d =
            pp.score(ps, num_for_ppc, ppc_seed, R, seed, std::vector<double>(probs, probs + n_probs), std::vector<double>(levels, levels + n_levels),
                     observed_in ? &obs : nullptr, means != nullptr, draws != nullptr);
        std::copy(d.pred_quantiles.begin(), d.pred_quantiles.end(), pred);
        if (pit) std::copy(d.pit.begin(), d.pit.end(), pit);
        std::copy(d.cell_scores.begin(), d.cell_scores.end(), cell_scores);
        std::copy(d.summary.begin(), d.summary.end(), summary);
        if (means) std::copy(d.means.begin(), d.means.end(), means);
        if (draws) std::copy(d.draws.begin(), d.draws.end(), draws);
        if (k_used) std::copy(d.k_used.begin(), d.k_used.end(), k_used);
        if (exact) *exact = d.exact ? 1 : 0;
        for (size_t i = 0; i < d.selected.size(); ++i) selected[i] = d.selected[i];
        *n_selected = static_cast<int32_t>(d.selected.size());
        if (status) std::copy(d.status.begin(), d.status.end(), status);
        *samples_used = d.samples_used;
    });
}

// ---- the same scores on window and age-group totals (sepaihrd_ensemble_predictive_targets) ----
// hostPosteriorPredictiveTargets (no device): shapes as sepaihrd_ensemble_predictive_targets; k_used NULL: Poisson draws
int host_predictive_targets_from_means(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R,
                                       int T_pos, int n_age, uint64_t seed, const int32_t* age_group, int window, int origin, const double* probs,
                                       int n_probs, const double* levels, int n_levels, double* target_quantiles, double* pit,
                                       double* target_scores, double* summary, double* target_obs, double* target_draws, double* draws,
                                       int32_t* exact, char* err, int errlen) {
    std::string error;
    const int rc = hostPosteriorPredictiveTargets(means, status, k_used, observed, S, R, T_pos, n_age, seed, age_group, window, origin, probs, n_probs,
                                                  levels, n_levels, target_quantiles, pit, target_scores, summary, target_obs, target_draws, draws,
                                                  exact, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// HipPosteriorPredictive::scoreTargets over the handle's parameter manager / data, as host_predictive_scores drives score(); W and G
// are the caller's (sepaihrd_predictive_targets_validate), the outputs sized by them
int host_predictive_targets(void* hv, const sepaihrd_problem* pb, int device, const double* samples, int n_samples, int num_for_ppc,
                            uint32_t ppc_seed, int R, uint64_t seed, const double* probs, int n_probs, const double* levels, int n_levels,
                            const int32_t* age_group, int n_age, int window, int origin, const double* observed_in, double* target_quantiles,
                            double* pit, double* target_scores, double* summary, double* target_obs, double* target_draws, double* k_used,
                            int32_t* exact, int32_t* selected, int32_t* n_selected, int32_t* status, int32_t* samples_used) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        HipPosteriorPredictive pp = posterior_over<HipPosteriorPredictive>(*h, pb, device);
        if (h->has_dispersion) pp.objective().setDispersion(h->dispersion);
        const std::vector<Eigen::VectorXd> ps = sample_vectors(samples, n_samples, h->pm->getParameterCount());
        std::vector<double> obs;
        if (observed_in) obs.assign(observed_in, observed_in + pp.observed().size());
        const PosteriorPredictiveTargets d = pp.scoreTargets(
            ps, num_for_ppc, ppc_seed, R, seed, std::vector<double>(probs, probs + n_probs), std::vector<double>(levels, levels + n_levels),
            std::vector<int32_t>(age_group, age_group + n_age), window, origin, observed_in ? &obs : nullptr, false, false, target_draws != nullptr);
        std::copy(d.pred_quantiles.begin(), d.pred_quantiles.end(), target_quantiles);
        if (pit) std::copy(d.pit.begin(), d.pit.end(), pit);
        std::copy(d.target_scores.begin(), d.target_scores.end(), target_scores);
        std::copy(d.summary.begin(), d.summary.end(), summary);
        if (target_obs) std::copy(d.target_obs.begin(), d.target_obs.end(), target_obs);
        if (target_draws) std::copy(d.target_draws.begin(), d.target_draws.end(), target_draws);
        if (k_used) std::copy(d.k_used.begin(), d.k_used.end(), k_used);
        if (exact) *exact = d.exact ? 1 : 0;
        for (size_t i = 0; i < d.selected.size(); ++i) selected[i] = d.selected[i];
        *n_selected = static_cast<int32_t>(d.selected.size());
        if (status) std::copy(d.status.begin(), d.status.end(), status);
        *samples_used = d.samples_used;
    });
}

// ---- stochastic chain-binomial SEPAIHRD ensembles (HipStochasticSEPAIHRD) ----
// hostStochasticSEPAIHRD (no device): shapes as sepaihrd_ensemble_stochastic; M row-major, M[i n_age + j] = M(i, j)
int host_stochastic_from_values(int n_age, int n_times, int n_beta, int n_kappa, const double* times, const double* N, const double* M,
                                const double* beta_end_times, const double* kappa_end_times, const double* model_values, const int32_t* status,
                                int S, int R, int steps_per_interval, uint64_t seed, const double* probs, int n_probs, int keep, double* quantiles,
                                double* extinct, double* traj, double* final_state, char* err, int errlen) {
    StochasticSEPAIHRDFixedData fd;
    fd.n_age = n_age; fd.n_times = n_times; fd.n_beta = n_beta; fd.n_kappa = n_kappa;
    fd.times = times; fd.N = N; fd.M = M; fd.beta_end_times = beta_end_times; fd.kappa_end_times = kappa_end_times;
    std::string error;
    const int rc = hostStochasticSEPAIHRD(fd, model_values, status, S, R, steps_per_interval, seed, probs, n_probs, keep, quantiles, extinct, traj,
                                          final_state, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// HipStochasticSEPAIHRD::run over the handle's parameter manager / data.  samples: n_samples x P, selected by the PPC rule
// (num_samples, select_seed).  quantiles [6][n_probs][T_pos][n]; extinct, selected and status: capacity max(n_samples, num_samples).
int host_stochastic(void* hv, const sepaihrd_problem* pb, int device, int initial_state_mode, const double* samples, int n_samples, int num_samples,
                    uint32_t select_seed, int R, int steps_per_interval, uint64_t seed, const double* probs, int n_probs, double* quantiles,
                    double* extinct, int32_t* selected, int32_t* n_selected, int32_t* status, int32_t* samples_used) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        HipStochasticSEPAIHRD model(*h->pm, *h->data, std::vector<double>(pb->times, pb->times + pb->n_times), vec(pb->initial_state, 11 * pb->n_age),
                                    strategy_for(pb->solver), device, initial_state_mode);
        const std::vector<Eigen::VectorXd> ps = sample_vectors(samples, n_samples, h->pm->getParameterCount());
        const StochasticSEPAIHRDResult d = model.run(ps, num_samples, select_seed, R, steps_per_interval, seed, std::vector<double>(probs, probs + n_probs));
        std::copy(d.quantiles.begin(), d.quantiles.end(), quantiles);
        if (extinct) std::copy(d.extinct.begin(), d.extinct.end(), extinct);
        for (size_t i = 0; i < d.selected.size(); ++i) selected[i] = d.selected[i];
        *n_selected = static_cast<int32_t>(d.selected.size());
        if (status) std::copy(d.status.begin(), d.status.end(), status);
        *samples_used = d.samples_used;
    });
}

// The parameter part of a model_values row (everything before the initial counts) as the handle's parameter manager writes it:
// updateModelParameters(theta) in the given constraint mode, then the model parameters in the row's order.  0 ok, 1 = exception.
int host_stochastic_manager_values(void* hv, int mode, const double* theta, double* out) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        {
            const ConstraintModeScope in_mode(*h->pm, mode);
            h->pm->updateModelParameters(vec(theta, static_cast<int>(h->pm->getParameterCount())));
        }
        const SEPAIHRDParameters& mp = h->pm->modelParameters();
        size_t at = 0;
        for (double v : {mp.theta, mp.sigma, mp.gamma_p, mp.gamma_A, mp.gamma_I, mp.gamma_H, mp.gamma_ICU, mp.beta}) out[at++] = v;
        for (double v : mp.beta_values) out[at++] = v;
        for (double v : mp.kappa_values) out[at++] = v;
        for (const Eigen::VectorXd* f : {&mp.a, &mp.h_infec, &mp.p, &mp.h, &mp.icu, &mp.d_H, &mp.d_ICU, &mp.d_community})
            for (Eigen::Index i = 0; i < f->size(); ++i) out[at++] = (*f)[i];
    });
}

// ---- bootstrap particle filter of the stochastic SEPAIHRD model (HipParticleFilter) ----
// hostParticleLoglik (no device): shapes as sepaihrd_particle_loglik; obs_* [n_obs][n_age], the rows of the output times >= 0
namespace {
// the twin of one form: wide or not, negative-binomial (nb, with dispersion [3] = {k_H, k_ICU, k_D}) or Poisson
int particle_twin_from_values(bool wide, bool nb, int n_age, int n_times, int n_beta, int n_kappa, const double* times, const double* N, const double* M,
                              const double* beta_end_times, const double* kappa_end_times, int n_obs, const double* obs_H, const double* obs_ICU,
                              const double* obs_D, const double* model_values, const int32_t* status, int B, int J, int steps_per_interval,
                              uint64_t seed, const double* dispersion, double* loglik, double* increments, double* ess, double* final_state,
                              char* err, int errlen) {
    StochasticSEPAIHRDFixedData fd;
    fd.n_age = n_age; fd.n_times = n_times; fd.n_beta = n_beta; fd.n_kappa = n_kappa;
    fd.times = times; fd.N = N; fd.M = M; fd.beta_end_times = beta_end_times; fd.kappa_end_times = kappa_end_times;
    ParticleObservations ob;
    ob.n_obs = n_obs; ob.obs_H = obs_H; ob.obs_ICU = obs_ICU; ob.obs_D = obs_D;
    std::string error;
    const int rc = nb ? (wide ? hostParticleLoglikWideNB : hostParticleLoglikNB)(fd, ob, model_values, status, B, J, steps_per_interval, seed, dispersion,
                                                                                loglik, increments, ess, final_state, &error)
                      : (wide ? hostParticleLoglikWide : hostParticleLoglik)(fd, ob, model_values, status, B, J, steps_per_interval, seed, loglik,
                                                                            increments, ess, final_state, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}
}  // namespace

int host_particle_from_values(int n_age, int n_times, int n_beta, int n_kappa, const double* times, const double* N, const double* M,
                              const double* beta_end_times, const double* kappa_end_times, int n_obs, const double* obs_H, const double* obs_ICU,
                              const double* obs_D, const double* model_values, const int32_t* status, int B, int J, int steps_per_interval,
                              uint64_t seed, double* loglik, double* increments, double* ess, double* final_state, char* err, int errlen) {
    return particle_twin_from_values(false, false, n_age, n_times, n_beta, n_kappa, times, N, M, beta_end_times, kappa_end_times, n_obs, obs_H, obs_ICU,
                                     obs_D, model_values, status, B, J, steps_per_interval, seed, nullptr, loglik, increments, ess, final_state, err,
                                     errlen);
}

// hostParticleLoglikWide (no device): the same shapes, J up to 65 536
int host_particle_wide_from_values(int n_age, int n_times, int n_beta, int n_kappa, const double* times, const double* N, const double* M,
                                   const double* beta_end_times, const double* kappa_end_times, int n_obs, const double* obs_H, const double* obs_ICU,
                                   const double* obs_D, const double* model_values, const int32_t* status, int B, int J, int steps_per_interval,
                                   uint64_t seed, double* loglik, double* increments, double* ess, double* final_state, char* err, int errlen) {
    return particle_twin_from_values(true, false, n_age, n_times, n_beta, n_kappa, times, N, M, beta_end_times, kappa_end_times, n_obs, obs_H, obs_ICU,
                                     obs_D, model_values, status, B, J, steps_per_interval, seed, nullptr, loglik, increments, ess, final_state, err,
                                     errlen);
}

// hostParticleLoglikNB / hostParticleLoglikWideNB (no device): the same shapes with dispersion [3] = {k_H, k_ICU, k_D}
int host_particle_nb_from_values(int n_age, int n_times, int n_beta, int n_kappa, const double* times, const double* N, const double* M,
                                 const double* beta_end_times, const double* kappa_end_times, int n_obs, const double* obs_H, const double* obs_ICU,
                                 const double* obs_D, const double* model_values, const int32_t* status, int B, int J, int steps_per_interval,
                                 uint64_t seed, const double* dispersion, double* loglik, double* increments, double* ess, double* final_state,
                                 char* err, int errlen) {
    return particle_twin_from_values(false, true, n_age, n_times, n_beta, n_kappa, times, N, M, beta_end_times, kappa_end_times, n_obs, obs_H, obs_ICU,
                                     obs_D, model_values, status, B, J, steps_per_interval, seed, dispersion, loglik, increments, ess, final_state,
                                     err, errlen);
}

int host_particle_wide_nb_from_values(int n_age, int n_times, int n_beta, int n_kappa, const double* times, const double* N, const double* M,
                                      const double* beta_end_times, const double* kappa_end_times, int n_obs, const double* obs_H,
                                      const double* obs_ICU, const double* obs_D, const double* model_values, const int32_t* status, int B, int J,
                                      int steps_per_interval, uint64_t seed, const double* dispersion, double* loglik, double* increments, double* ess,
                                      double* final_state, char* err, int errlen) {
    return particle_twin_from_values(true, true, n_age, n_times, n_beta, n_kappa, times, N, M, beta_end_times, kappa_end_times, n_obs, obs_H, obs_ICU,
                                     obs_D, model_values, status, B, J, steps_per_interval, seed, dispersion, loglik, increments, ess, final_state,
                                     err, errlen);
}

// hostParticleStates (no device): the shapes of host_particle_wide_nb_from_values (dispersion NULL: Poisson) with probs [n_probs] and
// state_mean [B][n_times][11][n_age + 1], state_quantiles [B][n_times][11][n_age + 1][n_probs] (nullable) for final_state
int host_particle_states_from_values(int n_age, int n_times, int n_beta, int n_kappa, const double* times, const double* N, const double* M,
                                     const double* beta_end_times, const double* kappa_end_times, int n_obs, const double* obs_H,
                                     const double* obs_ICU, const double* obs_D, const double* model_values, const int32_t* status, int B, int J,
                                     int steps_per_interval, uint64_t seed, const double* dispersion, const double* probs, int n_probs,
                                     double* loglik, double* increments, double* ess, double* state_mean, double* state_quantiles, char* err,
                                     int errlen) {
    StochasticSEPAIHRDFixedData fd;
    fd.n_age = n_age; fd.n_times = n_times; fd.n_beta = n_beta; fd.n_kappa = n_kappa;
    fd.times = times; fd.N = N; fd.M = M; fd.beta_end_times = beta_end_times; fd.kappa_end_times = kappa_end_times;
    ParticleObservations ob;
    ob.n_obs = n_obs; ob.obs_H = obs_H; ob.obs_ICU = obs_ICU; ob.obs_D = obs_D;
    std::string error;
    const int rc = hostParticleStates(fd, ob, model_values, status, B, J, steps_per_interval, seed, dispersion, probs, n_probs, loglik, increments, ess,
                                      state_mean, state_quantiles, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// the twin of sepaihrd_particle_nb_term_device (no device): out[i] = nb_term(obs[i], inc[i], k)
void host_particle_nb_term(const double* obs, const int32_t* inc, int count, double k, double* out) { hostParticleNBTerm(obs, inc, count, k, out); }

// the twin of sepaihrd_particle_nb_row_constants (no device): G [T_pos] from obs_* [n_obs][n_age]
int host_particle_nb_row_constants(int n_age, int T_pos, int n_obs, const double* obs_H, const double* obs_ICU, const double* obs_D,
                                   const double* dispersion, double* G, char* err, int errlen) {
    ParticleObservations ob;
    ob.n_obs = n_obs; ob.obs_H = obs_H; ob.obs_ICU = obs_ICU; ob.obs_D = obs_D;
    std::string error;
    const int rc = hostParticleNBRowConstants(ob, n_age, T_pos, dispersion, G, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// the twin of sepaihrd_particle_resample_device (no device)
void host_particle_resample(uint64_t seed, uint32_t b, uint32_t row, const double* logw, int J, int32_t* ancestors, double* increment, double* ess) {
    hostParticleResample(seed, b, row, logw, J, ancestors, increment, ess);
}

// HipParticleLikelihood over the handle's parameter manager / data: n_calls successive calculateBatch calls on the same B
// parameter vectors (thetas B x P); values [n_calls][B], status [n_calls][B] (nullable).  0 ok, 1 = exception.
int host_particle_likelihood_nb(void* hv, const sepaihrd_problem* pb, int device, int initial_state_mode, int J, int steps_per_interval, uint64_t seed0,
                                const double* dispersion, const double* thetas, int B, int n_calls, double* values, int32_t* status);
int host_particle_likelihood(void* hv, const sepaihrd_problem* pb, int device, int initial_state_mode, int J, int steps_per_interval, uint64_t seed0,
                             const double* thetas, int B, int n_calls, double* values, int32_t* status) {
    return host_particle_likelihood_nb(hv, pb, device, initial_state_mode, J, steps_per_interval, seed0, nullptr, thetas, B, n_calls, values, status);
}

// the same after setDispersion(dispersion[0], dispersion[1], dispersion[2]); dispersion NULL: the adapter's default
int host_particle_likelihood_nb(void* hv, const sepaihrd_problem* pb, int device, int initial_state_mode, int J, int steps_per_interval, uint64_t seed0,
                                const double* dispersion, const double* thetas, int B, int n_calls, double* values, int32_t* status) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        HipParticleLikelihood lik(*h->pm, *h->data, std::vector<double>(pb->times, pb->times + pb->n_times), vec(pb->initial_state, 11 * pb->n_age),
                                  strategy_for(pb->solver), J, steps_per_interval, seed0, device, initial_state_mode);
        if (dispersion) lik.setDispersion(dispersion[0], dispersion[1], dispersion[2]);
        const IBatchObjectiveFunction& batch = lik;
        std::vector<int> st(static_cast<size_t>(B));
        for (int c = 0; c < n_calls; ++c) {
            batch.calculateBatch(thetas, B, values + static_cast<size_t>(c) * B, st.data());
            if (status) std::copy(st.begin(), st.end(), status + static_cast<size_t>(c) * B);
        }
    });
}

// HipParticleLikelihood::filterStates after n_calls_before calculateBatch calls on the same B parameter vectors, then one more
// calculateBatch: state_mean [B][n_times][11][n_age + 1], state_quantiles [B][n_times][11][n_age + 1][n_probs], loglik [B] (that
// of the filterStates call), next_values [B] (the calculateBatch after it), calls [2] (the call count before and after
// filterStates).  0 ok, 1 = exception.
int host_particle_filter_states(void* hv, const sepaihrd_problem* pb, int device, int initial_state_mode, int J, int steps_per_interval, uint64_t seed0,
                                const double* dispersion, const double* thetas, int B, int n_calls_before, const double* probs, int n_probs,
                                double* state_mean, double* state_quantiles, double* loglik, double* next_values, uint64_t* calls) {
    auto* h = static_cast<HostHandle*>(hv);
    return guarded([&] {
        HipParticleLikelihood lik(*h->pm, *h->data, std::vector<double>(pb->times, pb->times + pb->n_times), vec(pb->initial_state, 11 * pb->n_age),
                                  strategy_for(pb->solver), J, steps_per_interval, seed0, device, initial_state_mode);
        if (dispersion) lik.setDispersion(dispersion[0], dispersion[1], dispersion[2]);
        std::vector<double> scratch(static_cast<size_t>(B)), mean, quant, ll;
        for (int c = 0; c < n_calls_before; ++c) lik.calculateBatch(thetas, B, scratch.data(), nullptr);
        calls[0] = lik.calls();
        lik.filterStates(thetas, B, std::vector<double>(probs, probs + n_probs), mean, quant, &ll, nullptr);
        calls[1] = lik.calls();
        std::copy(mean.begin(), mean.end(), state_mean);
        std::copy(quant.begin(), quant.end(), state_quantiles);
        std::copy(ll.begin(), ll.end(), loglik);
        lik.calculateBatch(thetas, B, next_values, nullptr);
    });
}

// ---- the negative-binomial observation model of the deterministic objective, this library's compile of
// csrc/sepaihrd_lgamma.inc and csrc/sepaihrd_nb_objective.inc
double host_lgamma_pos(double x) { return sepaihrd_lgamma::lgamma_pos(x); }

// the twin of the device pass (sepaihrd_nb_objective_host's arguments): increments [B][T][3][n_age], obs_* [T][n_age], k [B][3]
// -> loglik [B], ll_parts [B][3] (nullable), status [B] (nullable)
int host_nb_objective(const double* increments, const double* obs_H, const double* obs_ICU, const double* obs_D, const double* k, int B, int T,
                      int n_age, double* loglik, double* ll_parts, int32_t* status) {
    if (!increments || !obs_H || !obs_ICU || !obs_D || !k || !loglik || B < 0 || T < 0 || n_age < 1) return SEPAIHRD_E_INVALID_ARG;
    const size_t Tn = static_cast<size_t>(T) * static_cast<size_t>(n_age);
    std::vector<double> obs(3 * Tn);
    std::copy(obs_H, obs_H + Tn, obs.begin());
    std::copy(obs_ICU, obs_ICU + Tn, obs.begin() + static_cast<std::ptrdiff_t>(Tn));
    std::copy(obs_D, obs_D + Tn, obs.begin() + static_cast<std::ptrdiff_t>(2 * Tn));
    for (int b = 0; b < B; ++b) {
        double parts[3];
        const int st = sepaihrd_nb_objective::chain_loglik(increments + static_cast<size_t>(b) * 3 * Tn, obs.data(), k + 3 * static_cast<size_t>(b), T,
                                                           n_age, [](double sim) { return std::log(sim); }, loglik + b, parts);
        if (status) status[b] = st;
        if (ll_parts)
            for (int s = 0; s < 3; ++s) ll_parts[3 * static_cast<size_t>(b) + s] = parts[s];
    }
    return SEPAIHRD_OK;
}

}  // extern "C"
