// host/include/epidemic_hip/HipPosteriorPredictive.hpp
//
// Posterior predictive draws with Poisson noise above sepaihrd_ensemble_predictive.  The reference has no such output: the
// bands of ResultAggregator::aggregatePosteriorPredictives (HipPosteriorEnsemble) are quantiles of the model's EXPECTED daily
// counts, parameter uncertainty only, while the likelihood it calibrates with treats an observed count as Poisson around that
// expectation.  Here every selected sample is simulated once and replicated R times, y ~ Poisson(max(0, increment) + 1e-10)
// from a stateless stream (csrc/sepaihrd_poisson.inc); bands of y and the mid-PIT of every usable observation follow.
// The CPU twin of the device's draw, sort and count passes (the same sampler text, OpenMP) is hostPosteriorPredictive.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "epidemic_hip/HipPosteriorEnsemble.hpp"

namespace epidemic {

// From means [S][3][T_pos][n_age] and status [S] as sepaihrd_ensemble_predictive returns them: the same draws
// [S][R][3][T_pos][n_age] (nullable; NaN for failed samples), pred_quantiles [6][n_probs][T_pos][n_age] and pit
// [3][T_pos][n_age] (nullable), bit for bit.  observed [3][T_pos][n_age] (hospitalisations, ICU admissions, deaths; NaN where
// there is none; NULL: no pit).  Returns SEPAIHRD_OK or SEPAIHRD_E_INVALID_ARG with sepaihrd_predictive_validate's message.
int hostPosteriorPredictive(const double* means, const int32_t* status, const double* observed, int S, int R, int T_pos, int n_age,
                            std::uint64_t seed, const double* probs, int n_probs, double* pred_quantiles, double* pit, double* draws,
                            std::string* error = nullptr);

// The dispersed form, the twin of sepaihrd_ensemble_predictive_nb: k_used [S][3] as that call returns it next to means and status;
// y ~ NegativeBinomial(m + 1e-10, k_used[s][series]) from csrc/sepaihrd_nb_draw.inc, a series at +inf the draws of the call above.
// SEPAIHRD_E_INVALID_ARG also for a NULL k_used and for a valid sample's k that sepaihrd_particle_nb_validate refuses (its message).
int hostPosteriorPredictiveNB(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                              int n_age, std::uint64_t seed, const double* probs, int n_probs, double* pred_quantiles, double* pit, double* draws,
                              std::string* error = nullptr);

// The scored form, the twin of sepaihrd_ensemble_predictive_scores (k_used NULL: Poisson draws): draws, pred_quantiles and pit as
// above -- the pit from the sorted segment's counts -- and cell_scores [3][T_pos][n_age][5 + 4 L], summary [3][n_age + 1][4 + 2 L]
// and *exact (nullable) by the text the kernels compile, csrc/sepaihrd_predictive_score.inc, after a std::sort of every segment:
// bit for bit where exact is 1.  observed [3][T_pos][n_age] is required.  SEPAIHRD_E_INVALID_ARG with
// sepaihrd_predictive_scores_validate's message.
int hostPosteriorPredictiveScores(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                                  int n_age, std::uint64_t seed, const double* probs, int n_probs, const double* levels, int n_levels,
                                  double* pred_quantiles, double* pit, double* cell_scores, double* summary, double* draws, int32_t* exact,
                                  std::string* error = nullptr);

// The scores on window and age-group totals, the twin of sepaihrd_ensemble_predictive_targets (k_used NULL: Poisson draws): the
// same daily draws summed into the targets of csrc/sepaihrd_predictive_targets.inc, a std::sort of every target segment and the
// score text; shapes as that call's.  observed [3][T_pos][n_age], target_quantiles, target_scores and summary are required; pit,
// target_obs, target_draws, draws and exact are nullable.  Bit for bit where *exact is 1.  SEPAIHRD_E_INVALID_ARG with
// sepaihrd_predictive_targets_validate's message.
int hostPosteriorPredictiveTargets(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                                   int n_age, std::uint64_t seed, const int32_t* age_group, int window, int origin, const double* probs, int n_probs,
                                   const double* levels, int n_levels, double* target_quantiles, double* pit, double* target_scores,
                                   double* summary, double* target_obs, double* target_draws, double* draws, int32_t* exact,
                                   std::string* error = nullptr);

// one unsorted sample x [m] against one observation y: scores [5 + 4 L] as a cell of cell_scores, its mid-PIT and whether its sums
// are exact (both nullable)
int hostScoreCell(const double* x, int m, double y, const double* levels, int n_levels, double* scores, double* pit, int32_t* exact,
                  std::string* error = nullptr);

// the gamma and negative-binomial samplers on the host: the variates at (seed, c0, c1, c2), and the twins of sepaihrd_gamma_device
// and sepaihrd_nb_draw_device (c0 = i, c1 = c2 = 0)
double hostGamma(std::uint64_t seed, std::uint32_t c0, std::uint32_t c1, std::uint32_t c2, double shape);
double hostNBDraw(std::uint64_t seed, std::uint32_t c0, std::uint32_t c1, std::uint32_t c2, double mu, double k);
void hostGammaProbe(std::uint64_t seed, const double* shape, int count, double* out);
void hostNBDrawProbe(std::uint64_t seed, const double* mu, const double* k, int count, double* out);

// the sampler on the host: the variate at (seed, c0, c1, c2), and the twin of sepaihrd_poisson_device (c0 = i, c1 = c2 = 0)
double hostPoisson(std::uint64_t seed, std::uint32_t c0, std::uint32_t c1, std::uint32_t c2, double lambda);
void hostPoissonProbe(std::uint64_t seed, const double* lambda, int count, double* out);

struct PosteriorPredictiveDraws {
    std::vector<double> time_points;  // the output times >= 0
    int n_age = 0, replicates = 0;
    int samples_used = 0;             // valid simulations; every segment holds samples_used x replicates draws
    std::vector<int> selected;        // indices of the simulated samples (HipPosteriorEnsemble::selectSamples)
    std::vector<double> probs;
    std::vector<double> pred_quantiles;  // [6][n_probs][T_pos][n_age]
    std::vector<double> pit;             // [3][T_pos][n_age]
    std::vector<double> means, draws;    // [S][3][T_pos][n_age], [S][R][3][T_pos][n_age]; empty unless asked for
    std::vector<int32_t> status;         // [S]
    std::vector<double> k_used;          // [S][3]: the dispersions drawn with; empty where the objective is not dispersed (Poisson draws)
};

// draw()'s result with the scores of sepaihrd_ensemble_predictive_scores
struct PosteriorPredictiveScores : PosteriorPredictiveDraws {
    std::vector<double> levels;       // the central coverage levels, L of them
    std::vector<double> cell_scores;  // [3][T_pos][n_age][5 + 4 L]
    std::vector<double> summary;      // [3][n_age + 1][4 + 2 L]
    bool exact = false;               // the sums were exact: the host twin gives the same bits
};

// the result of sepaihrd_ensemble_predictive_targets: pred_quantiles [6][n_probs][W][G] and pit [6][W][G] are the targets'
struct PosteriorPredictiveTargets : PosteriorPredictiveDraws {
    std::vector<int32_t> age_group;     // [n_age]
    int window = 0, origin = 0, W = 0, G = 0;
    std::vector<double> levels;
    std::vector<double> target_scores;  // [6][W][G][5 + 4 L]
    std::vector<double> summary;        // [6][G + 1][4 + 2 L]
    std::vector<double> target_obs;     // [6][W][G]
    std::vector<double> target_draws;   // [S][R][3][W][G]; empty unless asked for
    bool exact = false;
};

class HipPosteriorPredictive {
public:
    HipPosteriorPredictive(HipSEPAIHRDParameterManager& parameterManager, const CalibrationData& observed_data,
                           const std::vector<double>& time_points, const Eigen::VectorXd& initial_state,
                           std::shared_ptr<IOdeSolverStrategy> solver_strategy, double abs_error = 1.0e-6, double rel_error = 1.0e-6,
                           int device = -1, bool fma_arithmetic = false);

    // The device call over stored samples, selected by the PPC rule of HipPosteriorEnsemble::selectSamples
    // (num_samples_for_ppc draws with replacement from mt19937(random_seed) when 0 < num < size, else every sample in order).
    // Where the objective is dispersed (setDispersion on objective(), or calibrated dispersion_* names) the call is
    // sepaihrd_ensemble_predictive_nb with the context's dispersion: negative-binomial replicates, k_used filled.
    PosteriorPredictiveDraws draw(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc, unsigned int random_seed,
                                  int replicates, std::uint64_t seed, const std::vector<double>& probs, bool want_means = false,
                                  bool want_draws = false);

    // The scored call (sepaihrd_ensemble_predictive_scores) over the samples draw() would select, with the context's dispersion as
    // draw() picks it: Poisson draws where the objective is not dispersed.  k_used is always filled.  observed_table
    // [3][T_pos][n_age] (null: the data the object was built over) is what the scores and the PIT are taken against.
    PosteriorPredictiveScores score(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc, unsigned int random_seed,
                                    int replicates, std::uint64_t seed, const std::vector<double>& probs, const std::vector<double>& levels,
                                    const std::vector<double>* observed_table = nullptr, bool want_means = false, bool want_draws = false);

    // The scores on window and age-group totals (sepaihrd_ensemble_predictive_targets) over the samples score() would select, the
    // dispersion picked as score() picks it.  InvalidParameterException with sepaihrd_predictive_targets_validate's message for a
    // grouping or windows the call refuses.
    PosteriorPredictiveTargets scoreTargets(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc, unsigned int random_seed,
                                            int replicates, std::uint64_t seed, const std::vector<double>& probs,
                                            const std::vector<double>& levels, const std::vector<int32_t>& age_group, int window, int origin = 0,
                                            const std::vector<double>* observed_table = nullptr, bool want_means = false,
                                            bool want_draws = false, bool want_target_draws = false);

    // the observations as the device places them: [3][T_pos][n_age], row j of the data at output time j >= 0, NaN beyond the data
    std::vector<double> observed() const;

    // the objective whose context the draws run on (setDispersion)
    HipSEPAIHRDObjectiveFunction& objective() { return *objective_; }

private:
    // the header fields of `out`, its selection, and the selected samples as one S x P table (empty: nothing to simulate)
    std::vector<double> selectedThetas(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc, unsigned int random_seed,
                                       int replicates, const std::vector<double>& probs, PosteriorPredictiveDraws& out) const;

    HipSEPAIHRDParameterManager& pm_;
    const CalibrationData& data_;
    std::vector<double> time_points_;
    SimulationCache cache_;
    std::unique_ptr<HipSEPAIHRDObjectiveFunction> objective_;
    int n_ = 0, t_pos_ = 0;
};

}  // namespace epidemic
