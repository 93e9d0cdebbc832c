// host/include/epidemic_hip/HipParticleFilter.hpp
//
// The bootstrap particle filter of the stochastic chain-binomial SEPAIHRD model, above sepaihrd_particle_loglik: an unbiased
// estimate of the marginal likelihood p(y | theta) under process noise.  The reference has no such filter: this one is this
// build's own (csrc/sepaihrd_particle.inc states it; include/sepaihrd_hip.h describes the call).  The CPU twin of the device's
// filter kernel (the same text, OpenMP over theta) is hostParticleLoglik.
#pragma once
#include <cstdint>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "epidemic_hip/HipStochasticSEPAIHRD.hpp"
#include "sepaihrd_hip.h"

namespace epidemic {

// the observed daily counts of the output times >= 0, in time order: row r belongs to output row runup_offset + r; output rows
// beyond n_obs have no observation
struct ParticleObservations {
    int n_obs = 0;
    const double* obs_H = nullptr;    // [n_obs][n_age]
    const double* obs_ICU = nullptr;  // [n_obs][n_age]
    const double* obs_D = nullptr;    // [n_obs][n_age]
};

// From model_values [B][W] and status [B] as sepaihrd_particle_loglik returns them: the same loglik [B], increments
// [B][T_pos] (nullable), ess [B][T_pos] (nullable) and final_state [B][J][11][n_age] (nullable), bit for bit.  Returns
// SEPAIHRD_OK or SEPAIHRD_E_INVALID_ARG with sepaihrd_particle_validate's message.
int hostParticleLoglik(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                       const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, double* loglik, double* increments,
                       double* ess, double* final_state, std::string* error = nullptr);

// The twin of sepaihrd_particle_loglik_wide: the same walk behind sepaihrd_particle_wide_validate's rules (J up to 65 536; the
// twin has no chunks, theta_chunk does not change a result).
int hostParticleLoglikWide(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                           const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, double* loglik, double* increments,
                           double* ess, double* final_state, std::string* error = nullptr);

// The twins of sepaihrd_particle_loglik_nb and sepaihrd_particle_loglik_wide_nb: the same walk with the dispersion dispersion[3] =
// {k_H, k_ICU, k_D} of the observed series (csrc/sepaihrd_particle.inc; +inf keeps a series Poisson) and the row constants, formed
// by the text the device call forms them with (csrc/sepaihrd_particle_nb_host.h).  SEPAIHRD_E_INVALID_ARG with
// sepaihrd_particle_nb_validate's message for a dispersion that call refuses.
int hostParticleLoglikNB(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                         const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, const double* dispersion, double* loglik,
                         double* increments, double* ess, double* final_state, std::string* error = nullptr);
int hostParticleLoglikWideNB(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                             const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, const double* dispersion, double* loglik,
                             double* increments, double* ess, double* final_state, std::string* error = nullptr);
// The twin of sepaihrd_particle_filter_states: the same walk (dispersion NULL: Poisson) with the per-row summaries of
// csrc/sepaihrd_particle_states.inc taken from every row's cloud by std::sort and the ensemble's quantile expression.
// state_mean [B][n_times][11][n_age + 1], state_quantiles [B][n_times][11][n_age + 1][n_probs] (nullable), bit for bit; loglik,
// increments and ess are hostParticleLoglikWide's / hostParticleLoglikWideNB's.  SEPAIHRD_E_INVALID_ARG with
// sepaihrd_particle_states_validate's or sepaihrd_particle_nb_validate's message.
int hostParticleStates(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values, const int32_t* status,
                       int B, int J, int steps_per_interval, std::uint64_t seed, const double* dispersion, const double* probs, int n_probs,
                       double* loglik, double* increments, double* ess, double* state_mean, double* state_quantiles, std::string* error = nullptr);
// the row constants G [T_pos] such a call adds (the twin of sepaihrd_particle_nb_row_constants) and the twin of
// sepaihrd_particle_nb_term_device: out[i] = nb_term(obs[i], inc[i], k)
int hostParticleNBRowConstants(const ParticleObservations& obs, int n_age, int T_pos, const double* dispersion, double* G, std::string* error = nullptr);
void hostParticleNBTerm(const double* obs, const int32_t* inc, int count, double k, double* out);

// the twin of sepaihrd_particle_resample_device and of sepaihrd_particle_wide_resample_device (any J): one weighted row with log-weights logw [J] at the coordinates (seed, b, row)
void hostParticleResample(std::uint64_t seed, std::uint32_t b, std::uint32_t row, const double* logw, int J, int32_t* ancestors,
                          double* increment, double* ess);

// The filter as an objective: calculateBatch evaluates B parameter vectors in one device call with seed = seed0 + (calls so
// far), so that successive proposals of a sampler see fresh noise.  The samplers of this library (and the reference's
// MetropolisHastingsSampler) keep the value of the current point and do not evaluate it again: run over this objective, the
// existing Adaptive-Metropolis loop is therefore particle-marginal Metropolis-Hastings (Andrieu, Doucet & Holenstein 2010) and
// targets the exact posterior of the stochastic model.  Nothing in the samplers changes.  An invalid theta gives lowest(), as
// the ODE objective does.  With `particles` at or below sepaihrd_particle_max_particles(n_age) the call is
// sepaihrd_particle_loglik; above it, sepaihrd_particle_loglik_wide with theta_chunk = 0 (up to 65 536 particles).  After
// setDispersion with a finite entry the call is the _nb call of the same form (the negative-binomial observation model).
class HipParticleLikelihood : public virtual IObjectiveFunction, public IBatchObjectiveFunction {
public:
    HipParticleLikelihood(HipSEPAIHRDParameterManager& parameterManager, const CalibrationData& observed_data,
                          const std::vector<double>& time_points, const Eigen::VectorXd& initial_state,
                          std::shared_ptr<IOdeSolverStrategy> solver_strategy, int particles, int steps_per_interval, std::uint64_t seed0,
                          int device = -1, int initial_state_mode = SEPAIHRD_INIT_FROM_THETA);

    double calculate(const Eigen::VectorXd& parameters) const override;
    const std::vector<std::string>& getParameterNames() const override { return pm_.getParameterNames(); }
    void calculateBatch(const double* thetas, int B, double* out, int* status = nullptr) const override;
    std::uint64_t calls() const { return calls_; }
    // The filtered state means [B][n_times][11][n_age + 1] and quantile bands [B][n_times][11][n_age + 1][probs.size()] of
    // sepaihrd_particle_filter_states for B parameter vectors, at the seed the next calculateBatch would use and under the
    // dispersion set; the call count does not advance, so that next call is what it would have been.  loglik (optional): the
    // estimates of that call; status (optional) as in calculateBatch.
    void filterStates(const double* thetas, int B, const std::vector<double>& probs, std::vector<double>& state_mean,
                      std::vector<double>& state_quantiles, std::vector<double>* loglik = nullptr, int* status = nullptr) const;
    // the dispersion of the observed series, each +inf (Poisson, the default) or finite in [1e-3, 1e6]; throws
    // InvalidParameterException with sepaihrd_particle_nb_validate's message for anything else
    void setDispersion(double k_H, double k_ICU, double k_D);

private:
    HipSEPAIHRDParameterManager& pm_;
    const CalibrationData& data_;
    std::vector<double> time_points_;
    SimulationCache cache_;
    std::unique_ptr<HipSEPAIHRDObjectiveFunction> objective_;
    int particles_, steps_per_interval_, n_age_;
    std::uint64_t seed0_;
    mutable std::uint64_t calls_ = 0;
    double dispersion_[3] = {std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(),
                             std::numeric_limits<double>::infinity()};
};

}  // namespace epidemic
