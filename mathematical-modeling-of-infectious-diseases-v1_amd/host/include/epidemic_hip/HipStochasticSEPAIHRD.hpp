// host/include/epidemic_hip/HipStochasticSEPAIHRD.hpp
//
// Stochastic chain-binomial SEPAIHRD ensembles over posterior samples, above sepaihrd_ensemble_stochastic.  The reference has
// no stochastic form of its age-structured model: this one is this build's own (csrc/sepaihrd_stoch_sepaihrd.inc states it;
// include/sepaihrd_hip.h describes the call).  Every selected sample is replicated R times from a stateless stream; bands of
// the daily hospitalisations, ICU admissions and deaths and of their running sums follow, and per sample the share of
// replicates in which the infection died out.  The CPU twin of the device's step, sort and quantile passes (the same model
// text, OpenMP) is hostStochasticSEPAIHRD.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "epidemic_hip/HipPosteriorEnsemble.hpp"
#include "sepaihrd_hip.h"

namespace epidemic {

// the problem's fixed data, as the twin needs it
struct StochasticSEPAIHRDFixedData {
    int n_age = 0, n_times = 0, n_beta = 0, n_kappa = 0;
    const double* times = nullptr;            // [n_times]
    const double* N = nullptr;                // [n_age]
    const double* M = nullptr;                // [n_age][n_age] row-major: M[i n_age + j] = M(i, j)
    const double* beta_end_times = nullptr;   // [n_beta]
    const double* kappa_end_times = nullptr;  // [n_kappa]
};

// From model_values [S][W] and status [S] as sepaihrd_ensemble_stochastic returns them: the same quantiles
// [6][n_probs][T_pos][n_age], extinct [S] (nullable), traj [S][keep][n_times][11][n_age] (nullable unless keep > 0) and
// final_state [S][R][11][n_age] (nullable), bit for bit.  Returns SEPAIHRD_OK or SEPAIHRD_E_INVALID_ARG with
// sepaihrd_stochastic_validate's message.
int hostStochasticSEPAIHRD(const StochasticSEPAIHRDFixedData& pb, const double* model_values, const int32_t* status, int S, int R,
                           int steps_per_interval, std::uint64_t seed, const double* probs, int n_probs, int keep, double* quantiles,
                           double* extinct, double* traj, double* final_state, std::string* error = nullptr);

struct StochasticSEPAIHRDResult {
    std::vector<double> time_points;  // the output times >= 0
    int n_age = 0, replicates = 0, steps_per_interval = 0;
    int samples_used = 0;             // valid samples; every segment holds samples_used x replicates values
    std::vector<int> selected;        // indices of the simulated samples (HipPosteriorEnsemble::selectSamples)
    std::vector<double> probs;
    std::vector<double> quantiles;    // [6][n_probs][T_pos][n_age]
    std::vector<double> extinct;      // [S]
    std::vector<int32_t> status;      // [S]
};

class HipStochasticSEPAIHRD {
public:
    HipStochasticSEPAIHRD(HipSEPAIHRDParameterManager& parameterManager, const CalibrationData& observed_data,
                          const std::vector<double>& time_points, const Eigen::VectorXd& initial_state,
                          std::shared_ptr<IOdeSolverStrategy> solver_strategy, int device = -1,
                          int initial_state_mode = SEPAIHRD_INIT_FIXED);

    // The device call over stored samples, selected by the PPC rule of HipPosteriorEnsemble::selectSamples
    // (num_samples draws with replacement from mt19937(random_seed) when 0 < num < size, else every sample in order).
    StochasticSEPAIHRDResult run(const std::vector<Eigen::VectorXd>& param_samples, int num_samples, unsigned int random_seed,
                                 int replicates, int steps_per_interval, std::uint64_t seed, const std::vector<double>& probs);

private:
    HipSEPAIHRDParameterManager& pm_;
    const CalibrationData& data_;
    std::vector<double> time_points_;
    SimulationCache cache_;
    std::unique_ptr<HipSEPAIHRDObjectiveFunction> objective_;
    int n_ = 0, t_pos_ = 0;
};

}  // namespace epidemic
