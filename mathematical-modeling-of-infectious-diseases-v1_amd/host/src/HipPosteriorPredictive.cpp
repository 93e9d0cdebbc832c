// host/src/HipPosteriorPredictive.cpp -- HipPosteriorPredictive, the CPU twin of sepaihrd_ensemble_predictive's draw, sort and
// count passes, and of sepaihrd_ensemble_predictive_nb's.  The samplers are csrc/sepaihrd_poisson.inc and csrc/sepaihrd_nb_draw.inc, the
// texts the kernels compile; this library is built with -ffp-contract=off like the kernels.
#include "epidemic_hip/HipPosteriorPredictive.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>

#include "sepaihrd_hip.h"
#include "sepaihrd_nb_draw.inc"
#include "sepaihrd_poisson.inc"
#include "sepaihrd_predictive_score.inc"
#include "sepaihrd_predictive_targets.inc"
#include "sepaihrd_quantile.inc"

namespace epidemic {

namespace {
// what the scored form adds: every daily segment is scored after its sort, and the PIT comes from the sorted segment's counts
struct ScoreOut {
    const double* levels;
    int n_levels;
    double *cell_scores, *summary;
    int32_t* exact;
};

// both forms; k_used null: the Poisson call's draws
int predictive_from_means(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                          int n_age, std::uint64_t seed, const double* probs, int n_probs, double* pred_quantiles, double* pit, double* draws,
                          std::string* error, const ScoreOut* so = nullptr) {
    char msg[256] = "";
    int vrc = so ? sepaihrd_predictive_scores_validate(S, R, T_pos, n_age, probs, n_probs, so->levels, so->n_levels, msg, (int)sizeof(msg))
                 : sepaihrd_predictive_validate(S, R, T_pos, n_age, probs, n_probs, msg, (int)sizeof(msg));
    if (vrc == SEPAIHRD_OK && so && (!observed || !so->cell_scores || !so->summary)) {
        std::snprintf(msg, sizeof(msg), "ensemble_predictive_scores: observed, cell_scores and summary must not be NULL");
        vrc = SEPAIHRD_E_INVALID_ARG;
    }
    if (vrc == SEPAIHRD_OK && (!means || !status || !pred_quantiles)) {
        std::snprintf(msg, sizeof(msg), "ensemble_predictive: means, status and pred_quantiles must not be NULL");
        vrc = SEPAIHRD_E_INVALID_ARG;
    }
    if (vrc != SEPAIHRD_OK) {
        if (error) *error = msg;
        return vrc;
    }
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const size_t Tp = (size_t)T_pos, n = (size_t)n_age;
    std::vector<int> valid;  // positions in theta of the valid samples
    for (int s = 0; s < S; ++s)
        if (status[s] == 0) valid.push_back(s);
    const size_t nd = valid.size() * (size_t)R;  // draws per segment
    if (draws)
        for (int s = 0; s < S; ++s)
            if (status[s] != 0) std::fill(draws + (size_t)s * R * 3 * Tp * n, draws + (size_t)(s + 1) * R * 3 * Tp * n, qnan);
    int all_exact = 1;
    // one age class at a time: its 6 T_pos segments of nd draws
    std::vector<double> seg((size_t)6 * Tp * nd);
    for (size_t a = 0; a < n; ++a) {
#pragma omp parallel for schedule(static)
        for (long long d = 0; d < (long long)nd; ++d) {
            const size_t s = (size_t)valid[(size_t)d / (size_t)R], r = (size_t)d % (size_t)R;
            double run[3] = {0.0, 0.0, 0.0};
            for (size_t t = 0; t < Tp; ++t)
                for (size_t k = 0; k < 3; ++k) {
                    const size_t cell = (k * Tp + t) * n + a;
                    const double m = means[((s * 3 + k) * Tp + t) * n + a];
                    const double y = k_used ? sepaihrd_nb_draw::nb_variate(seed, (uint32_t)s, (uint32_t)r, (uint32_t)cell, m + 1e-10, k_used[s * 3 + k])
                                            : sepaihrd_poisson::poisson(seed, (uint32_t)s, (uint32_t)r, (uint32_t)cell, m + 1e-10);
                    run[k] += y;
                    seg[(k * Tp + t) * nd + (size_t)d] = y;
                    seg[((k + 3) * Tp + t) * nd + (size_t)d] = run[k];
                    if (draws) draws[(((s * (size_t)R + r) * 3 + k) * Tp + t) * n + a] = y;
                }
        }
#pragma omp parallel for schedule(dynamic, 4)
        for (long long sg = 0; sg < (long long)(6 * Tp); ++sg) {
            const size_t ser = (size_t)sg / Tp, t = (size_t)sg % Tp;
            double* x = seg.data() + (size_t)sg * nd;
            if (pit && ser < 3 && !so) {
                const size_t cell = (ser * Tp + t) * n + a;
                const double obs = observed ? observed[cell] : qnan;
                double v = qnan;
                if (obs >= 0.0 && obs <= std::numeric_limits<double>::max()) {
                    int64_t less = 0, equal = 0;
                    for (size_t i = 0; i < nd; ++i) {
                        less += x[i] < obs;
                        equal += x[i] == obs;
                    }
                    v = sepaihrd_poisson::mid_pit(less, equal, (int64_t)nd);
                }
                pit[cell] = v;
            }
            std::sort(x, x + nd);
            if (so && ser < 3) {
                const size_t cell = (ser * Tp + t) * n + a;
                const double obs = observed[cell];
                const sepaihrd_score::SegmentSums sums = sepaihrd_score::segment_sums(x, nd, obs);
                sepaihrd_score::cell_rule(x, nd, obs, sums, so->levels, so->n_levels,
                                          so->cell_scores + cell * (size_t)sepaihrd_score::cell_width(so->n_levels));
                if (pit) pit[cell] = sepaihrd_score::pit_of(sums, nd, obs);
                if (nd > 0 && !sepaihrd_score::sums_exact(nd, x[nd - 1])) {
#pragma omp atomic write
                    all_exact = 0;
                }
            }
            for (int p = 0; p < n_probs; ++p)
                pred_quantiles[((ser * (size_t)n_probs + (size_t)p) * Tp + t) * n + a] = nd > 0 ? sepaihrd_quantile::sorted_quantile(x, nd, probs[p]) : qnan;
        }
    }
    if (so) {
        const size_t SW = (size_t)sepaihrd_score::summary_width(so->n_levels);
        for (int ser = 0; ser < 3; ++ser)
            for (int a = 0; a <= n_age; ++a)
                sepaihrd_score::summary_walk(so->cell_scores, observed, nd, T_pos, n_age, so->n_levels, ser, a,
                                             so->summary + ((size_t)ser * (n + 1) + (size_t)a) * SW);
        if (so->exact) *so->exact = all_exact;
    }
    return SEPAIHRD_OK;
}
}  // namespace

int hostPosteriorPredictiveScores(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                                  int n_age, std::uint64_t seed, const double* probs, int n_probs, const double* levels, int n_levels,
                                  double* pred_quantiles, double* pit, double* cell_scores, double* summary, double* draws, int32_t* exact,
                                  std::string* error) {
    for (int s = 0; s < S && status && k_used; ++s) {
        if (status[s] != 0) continue;
        char msg[256] = "";
        if (sepaihrd_particle_nb_validate(k_used + (size_t)s * 3, msg, (int)sizeof(msg)) != SEPAIHRD_OK) {
            if (error) *error = msg;
            return SEPAIHRD_E_INVALID_ARG;
        }
    }
    const ScoreOut so{levels, n_levels, cell_scores, summary, exact};
    return predictive_from_means(means, status, k_used, observed, S, R, T_pos, n_age, seed, probs, n_probs, pred_quantiles, pit, draws, error, &so);
}

int hostScoreCell(const double* x, int m, double y, const double* levels, int n_levels, double* scores, double* pit, int32_t* exact,
                  std::string* error) {
    if (!x || m < 1 || !scores || n_levels < 0 || n_levels > sepaihrd_score::MAX_LEVELS || (n_levels > 0 && !levels)) {
        if (error) *error = "score_cell: need x, m >= 1, scores and 0 <= n_levels <= 8 levels";
        return SEPAIHRD_E_INVALID_ARG;
    }
    for (int l = 0; l < n_levels; ++l)
        if (!(levels[l] > 0.0 && levels[l] < 1.0)) {
            if (error) *error = "score_cell: levels must lie strictly inside (0, 1)";
            return SEPAIHRD_E_INVALID_ARG;
        }
    std::vector<double> sorted(x, x + m);
    std::sort(sorted.begin(), sorted.end());
    const sepaihrd_score::SegmentSums sums = sepaihrd_score::segment_sums(sorted.data(), (size_t)m, y);
    sepaihrd_score::cell_rule(sorted.data(), (size_t)m, y, sums, levels, n_levels, scores);
    if (pit) *pit = sepaihrd_score::pit_of(sums, (size_t)m, y);
    if (exact) *exact = sepaihrd_score::sums_exact((size_t)m, sorted[(size_t)m - 1]) ? 1 : 0;
    return SEPAIHRD_OK;
}

int hostPosteriorPredictiveTargets(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                                   int n_age, std::uint64_t seed, const int32_t* age_group, int window, int origin, const double* probs, int n_probs,
                                   const double* levels, int n_levels, double* target_quantiles, double* pit, double* target_scores,
                                   double* summary, double* target_obs, double* target_draws, double* draws, int32_t* exact, std::string* error) {
    char msg[256] = "";
    int W = 0, G = 0;
    int vrc = sepaihrd_predictive_targets_validate(S, R, T_pos, n_age, age_group, window, origin, probs, n_probs, levels, n_levels, &W, &G, msg,
                                                   (int)sizeof(msg));
    if (vrc == SEPAIHRD_OK && (!means || !status || !observed || !target_quantiles || !target_scores || !summary)) {
        std::snprintf(msg, sizeof(msg), "ensemble_predictive_targets: means, status, observed, target_quantiles, target_scores and summary must not be NULL");
        vrc = SEPAIHRD_E_INVALID_ARG;
    }
    for (int s = 0; vrc == SEPAIHRD_OK && s < S && k_used; ++s)
        if (status[s] == 0) vrc = sepaihrd_particle_nb_validate(k_used + (size_t)s * 3, msg, (int)sizeof(msg));
    if (vrc != SEPAIHRD_OK) {
        if (error) *error = msg;
        return vrc;
    }
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const size_t Tp = (size_t)T_pos, n = (size_t)n_age, WG = (size_t)W * G, segments = 6 * WG;
    std::vector<int> valid;
    for (int s = 0; s < S; ++s)
        if (status[s] == 0) valid.push_back(s);
    const size_t nd = valid.size() * (size_t)R;  // draws per segment
    const size_t per_draw = 3 * Tp * n;
    for (int s = 0; s < S; ++s) {
        if (status[s] == 0) continue;
        if (draws) std::fill(draws + (size_t)s * R * per_draw, draws + (size_t)(s + 1) * R * per_draw, qnan);
        if (target_draws) std::fill(target_draws + (size_t)s * R * 3 * WG, target_draws + (size_t)(s + 1) * R * 3 * WG, qnan);
    }
    // every draw's daily variates summed into its targets: the order does not show while the sums are exact
    std::vector<double> seg(segments * nd);
#pragma omp parallel
    {
        std::vector<double> tot(3 * WG);
#pragma omp for schedule(static)
        for (long long d = 0; d < (long long)nd; ++d) {
            const size_t s = (size_t)valid[(size_t)d / (size_t)R], r = (size_t)d % (size_t)R;
            std::fill(tot.begin(), tot.end(), 0.0);
            for (size_t k = 0; k < 3; ++k)
                for (size_t t = 0; t < Tp; ++t) {
                    const int v = sepaihrd_targets::window_of_row((int)t, window, origin, W);
                    for (size_t a = 0; a < n; ++a) {
                        const int g = age_group[a];
                        if (!draws && (v < 0 || g < 0)) continue;
                        const size_t cell = (k * Tp + t) * n + a;
                        const double m = means[((s * 3 + k) * Tp + t) * n + a];
                        const double y = k_used ? sepaihrd_nb_draw::nb_variate(seed, (uint32_t)s, (uint32_t)r, (uint32_t)cell, m + 1e-10, k_used[s * 3 + k])
                                                : sepaihrd_poisson::poisson(seed, (uint32_t)s, (uint32_t)r, (uint32_t)cell, m + 1e-10);
                        if (draws) draws[(s * (size_t)R + r) * per_draw + cell] = y;
                        if (v >= 0 && g >= 0) tot[(k * W + (size_t)v) * G + (size_t)g] += y;
                    }
                }
            for (size_t k = 0; k < 3; ++k)
                for (size_t g = 0; g < (size_t)G; ++g) {
                    double run = 0.0;
                    for (size_t v = 0; v < (size_t)W; ++v) {
                        const double x = tot[(k * W + v) * G + g];
                        run += x;
                        seg[sepaihrd_targets::target_index((int)k, (int)v, (int)g, W, G) * nd + (size_t)d] = x;
                        seg[sepaihrd_targets::target_index((int)k + 3, (int)v, (int)g, W, G) * nd + (size_t)d] = run;
                    }
                }
            if (target_draws) std::copy(tot.begin(), tot.end(), target_draws + (s * (size_t)R + r) * 3 * WG);
        }
    }
    std::vector<double> tobs_own;
    if (!target_obs) {
        tobs_own.resize(segments);
        target_obs = tobs_own.data();
    }
    const auto obs_at = [&](int k, int t, int a) { return observed[((size_t)k * Tp + (size_t)t) * n + (size_t)a]; };
    for (int k = 0; k < 3; ++k)
        for (int g = 0; g < G; ++g) sepaihrd_targets::observed_targets(obs_at, age_group, n_age, window, origin, W, G, k, g, target_obs);
    int all_exact = 1;
    const size_t CW = (size_t)sepaihrd_score::cell_width(n_levels);
#pragma omp parallel for schedule(dynamic, 4)
    for (long long sg = 0; sg < (long long)segments; ++sg) {
        const size_t sid = (size_t)sg, k = sid / WG, vg = sid % WG;
        double* x = seg.data() + sid * nd;
        std::sort(x, x + nd);
        const double obs = target_obs[sid];
        const sepaihrd_score::SegmentSums sums = sepaihrd_score::segment_sums(x, nd, obs);
        sepaihrd_score::cell_rule(x, nd, obs, sums, levels, n_levels, target_scores + sid * CW);
        if (pit) pit[sid] = sepaihrd_score::pit_of(sums, nd, obs);
        if (nd > 0 && !sepaihrd_score::sums_exact(nd, x[nd - 1])) {
#pragma omp atomic write
            all_exact = 0;
        }
        for (int p = 0; p < n_probs; ++p)
            target_quantiles[(k * (size_t)n_probs + (size_t)p) * WG + vg] = nd > 0 ? sepaihrd_quantile::sorted_quantile(x, nd, probs[p]) : qnan;
    }
    const size_t SW = (size_t)sepaihrd_score::summary_width(n_levels);
    for (int k = 0; k < sepaihrd_targets::N_SERIES; ++k)
        for (int g = 0; g <= G; ++g)
            for (int f = 0; f < (int)SW; ++f)
                summary[((size_t)k * (G + 1) + (size_t)g) * SW + (size_t)f] =
                    sepaihrd_targets::target_summary_field(target_scores, target_obs, nd, W, G, n_levels, k, g, f);
    if (exact) *exact = all_exact;
    return SEPAIHRD_OK;
}

int hostPosteriorPredictive(const double* means, const int32_t* status, const double* observed, int S, int R, int T_pos, int n_age,
                            std::uint64_t seed, const double* probs, int n_probs, double* pred_quantiles, double* pit, double* draws,
                            std::string* error) {
    return predictive_from_means(means, status, nullptr, observed, S, R, T_pos, n_age, seed, probs, n_probs, pred_quantiles, pit, draws, error);
}

int hostPosteriorPredictiveNB(const double* means, const int32_t* status, const double* k_used, const double* observed, int S, int R, int T_pos,
                              int n_age, std::uint64_t seed, const double* probs, int n_probs, double* pred_quantiles, double* pit, double* draws,
                              std::string* error) {
    if (!k_used) {
        if (error) *error = "ensemble_predictive: k_used must not be NULL";
        return SEPAIHRD_E_INVALID_ARG;
    }
    // a valid sample's dispersions are what the device call can have produced: each +inf or finite in [1e-3, 1e6]
    for (int s = 0; s < S && status; ++s) {
        if (status[s] != 0) continue;
        char msg[256] = "";
        if (sepaihrd_particle_nb_validate(k_used + (size_t)s * 3, msg, (int)sizeof(msg)) != SEPAIHRD_OK) {
            if (error) *error = msg;
            return SEPAIHRD_E_INVALID_ARG;
        }
    }
    return predictive_from_means(means, status, k_used, observed, S, R, T_pos, n_age, seed, probs, n_probs, pred_quantiles, pit, draws, error);
}

double hostGamma(std::uint64_t seed, std::uint32_t c0, std::uint32_t c1, std::uint32_t c2, double shape) {
    return sepaihrd_nb_draw::gamma(seed, c0, c1, c2, shape);
}

double hostNBDraw(std::uint64_t seed, std::uint32_t c0, std::uint32_t c1, std::uint32_t c2, double mu, double k) {
    return sepaihrd_nb_draw::nb_variate(seed, c0, c1, c2, mu, k);
}

void hostGammaProbe(std::uint64_t seed, const double* shape, int count, double* out) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < count; ++i) out[i] = sepaihrd_nb_draw::gamma(seed, (uint32_t)i, 0u, 0u, shape[i]);
}

void hostNBDrawProbe(std::uint64_t seed, const double* mu, const double* k, int count, double* out) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < count; ++i) out[i] = sepaihrd_nb_draw::nb_variate(seed, (uint32_t)i, 0u, 0u, mu[i], k[i]);
}

double hostPoisson(std::uint64_t seed, std::uint32_t c0, std::uint32_t c1, std::uint32_t c2, double lambda) {
    return sepaihrd_poisson::poisson(seed, c0, c1, c2, lambda);
}

void hostPoissonProbe(std::uint64_t seed, const double* lambda, int count, double* out) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < count; ++i) out[i] = sepaihrd_poisson::poisson(seed, (uint32_t)i, 0u, 0u, lambda[i]);
}

HipPosteriorPredictive::HipPosteriorPredictive(HipSEPAIHRDParameterManager& parameterManager, const CalibrationData& observed_data,
                                               const std::vector<double>& time_points, const Eigen::VectorXd& initial_state,
                                               std::shared_ptr<IOdeSolverStrategy> solver_strategy, double abs_error, double rel_error,
                                               int device, bool fma_arithmetic)
    : pm_(parameterManager), data_(observed_data), time_points_(time_points), cache_(1) {
    objective_ = std::make_unique<HipSEPAIHRDObjectiveFunction>(pm_, cache_, data_, time_points_, initial_state, std::move(solver_strategy),
                                                                abs_error, rel_error, device, fma_arithmetic);
    if (sepaihrd_set_initial_state_mode(objective_->deviceContext(), SEPAIHRD_INIT_FIXED) != SEPAIHRD_OK)
        throw ModelException("HipPosteriorPredictive", "sepaihrd_set_initial_state_mode failed");
    n_ = static_cast<int>(pm_.modelParameters().N.size());
    for (double t : time_points_) t_pos_ += (t >= 0.0);
}

std::vector<double> HipPosteriorPredictive::observed() const {
    const size_t Tp = static_cast<size_t>(t_pos_), n = static_cast<size_t>(n_);
    std::vector<double> out(3 * Tp * n, std::numeric_limits<double>::quiet_NaN());
    const Eigen::MatrixXd* src[3] = {&data_.getNewHospitalizations(), &data_.getNewICU(), &data_.getNewDeaths()};
    for (size_t k = 0; k < 3; ++k)
        for (size_t t = 0; t < Tp && t < static_cast<size_t>(src[k]->rows()); ++t)
            for (size_t a = 0; a < n && a < static_cast<size_t>(src[k]->cols()); ++a)
                out[(k * Tp + t) * n + a] = (*src[k])(static_cast<Eigen::Index>(t), static_cast<Eigen::Index>(a));
    return out;
}

std::vector<double> HipPosteriorPredictive::selectedThetas(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc,
                                                           unsigned int random_seed, int replicates, const std::vector<double>& probs,
                                                           PosteriorPredictiveDraws& out) const {
    for (double t : time_points_)
        if (t >= 0.0) out.time_points.push_back(t);
    out.n_age = n_;
    out.replicates = replicates;
    out.probs = probs;
    if (out.time_points.empty() || param_samples.empty()) return {};
    out.selected = HipPosteriorEnsemble::selectSamples(param_samples.size(), num_samples_for_ppc, random_seed);
    const size_t P = pm_.getParameterCount(), S = out.selected.size();
    std::vector<double> thetas(S * P);
    for (size_t s = 0; s < S; ++s) {
        const Eigen::VectorXd& v = param_samples[static_cast<size_t>(out.selected[s])];
        if (static_cast<size_t>(v.size()) != P) throw InvalidParameterException("HipPosteriorPredictive", "sample size mismatch");
        for (size_t i = 0; i < P; ++i) thetas[s * P + i] = v[static_cast<Eigen::Index>(i)];
    }
    return thetas;
}

PosteriorPredictiveScores HipPosteriorPredictive::score(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc,
                                                        unsigned int random_seed, int replicates, std::uint64_t seed,
                                                        const std::vector<double>& probs, const std::vector<double>& levels,
                                                        const std::vector<double>* observed_table, bool want_means, bool want_draws) {
    PosteriorPredictiveScores out;
    out.levels = levels;
    const std::vector<double> thetas = selectedThetas(param_samples, num_samples_for_ppc, random_seed, replicates, probs, out);
    if (thetas.empty()) return out;
    const size_t S = out.selected.size(), L = levels.size();
    const size_t cells = static_cast<size_t>(3) * t_pos_ * n_;
    if (observed_table && observed_table->size() != cells)
        throw InvalidParameterException("HipPosteriorPredictive", "observed must hold 3 x T_pos x n_age values");
    sepaihrd_ctx* ctx = objective_->deviceContext();
    objective_->syncDeviceConstraintMode();
    out.pred_quantiles.assign(2 * cells * probs.size(), 0.0);
    out.pit.assign(cells, 0.0);
    out.cell_scores.assign(cells * (5 + 4 * L), 0.0);
    out.summary.assign(static_cast<size_t>(3) * (n_ + 1) * (4 + 2 * L), 0.0);
    if (want_means) out.means.assign(S * cells, 0.0);
    if (want_draws && replicates > 0) out.draws.assign(S * static_cast<size_t>(replicates) * cells, 0.0);
    out.status.assign(S, 0);
    out.k_used.assign(S * 3, 0.0);
    int32_t nv = 0, exact = 0;
    // dispersion NULL: the context's own, per sample -- Poisson draws where the objective is not dispersed, as draw() picks
    const int rc = sepaihrd_ensemble_predictive_scores(
        ctx, thetas.data(), static_cast<int>(S), replicates, seed, nullptr, observed_table ? observed_table->data() : nullptr, probs.data(),
        static_cast<int>(probs.size()), levels.data(), static_cast<int>(L), out.pred_quantiles.data(), out.pit.data(), out.cell_scores.data(),
        out.summary.data(), want_means ? out.means.data() : nullptr, out.draws.empty() ? nullptr : out.draws.data(), out.k_used.data(),
        out.status.data(), &nv, &exact);
    if (rc != SEPAIHRD_OK)
        throw ModelException("HipPosteriorPredictive", std::string("sepaihrd_ensemble_predictive_scores: ") + sepaihrd_last_error(ctx));
    out.samples_used = nv;
    out.exact = exact != 0;
    return out;
}

PosteriorPredictiveTargets HipPosteriorPredictive::scoreTargets(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc,
                                                                unsigned int random_seed, int replicates, std::uint64_t seed,
                                                                const std::vector<double>& probs, const std::vector<double>& levels,
                                                                const std::vector<int32_t>& age_group, int window, int origin,
                                                                const std::vector<double>* observed_table, bool want_means, bool want_draws,
                                                                bool want_target_draws) {
    PosteriorPredictiveTargets out;
    out.levels = levels;
    out.age_group = age_group;
    out.window = window;
    out.origin = origin;
    const std::vector<double> thetas = selectedThetas(param_samples, num_samples_for_ppc, random_seed, replicates, probs, out);
    if (thetas.empty()) return out;
    const size_t S = out.selected.size(), L = levels.size();
    const size_t cells = static_cast<size_t>(3) * t_pos_ * n_;
    if (observed_table && observed_table->size() != cells)
        throw InvalidParameterException("HipPosteriorPredictive", "observed must hold 3 x T_pos x n_age values");
    if (static_cast<int>(age_group.size()) != n_) throw InvalidParameterException("HipPosteriorPredictive", "age_group must hold n_age entries");
    char msg[256] = "";
    if (replicates > 0 && !probs.empty() &&
        sepaihrd_predictive_scores_validate(static_cast<int>(S), replicates, t_pos_, n_, probs.data(), static_cast<int>(probs.size()), levels.data(),
                                            static_cast<int>(L), nullptr, 0) == SEPAIHRD_OK &&
        sepaihrd_predictive_targets_validate(static_cast<int>(S), replicates, t_pos_, n_, age_group.data(), window, origin, probs.data(),
                                             static_cast<int>(probs.size()), levels.data(), static_cast<int>(L), &out.W, &out.G, msg,
                                             static_cast<int>(sizeof(msg))) != SEPAIHRD_OK)
        throw InvalidParameterException("HipPosteriorPredictive", msg);
    if (out.W < 1 || out.G < 1) out.W = out.G = 1;  // the call below refuses with the scored call's own message
    sepaihrd_ctx* ctx = objective_->deviceContext();
    objective_->syncDeviceConstraintMode();
    const size_t targets = static_cast<size_t>(6) * out.W * out.G;
    out.pred_quantiles.assign(targets * probs.size(), 0.0);
    out.pit.assign(targets, 0.0);
    out.target_obs.assign(targets, 0.0);
    out.target_scores.assign(targets * (5 + 4 * L), 0.0);
    out.summary.assign(static_cast<size_t>(6) * (out.G + 1) * (4 + 2 * L), 0.0);
    if (want_means) out.means.assign(S * cells, 0.0);
    if (want_draws && replicates > 0) out.draws.assign(S * static_cast<size_t>(replicates) * cells, 0.0);
    if (want_target_draws && replicates > 0) out.target_draws.assign(S * static_cast<size_t>(replicates) * (targets / 2), 0.0);
    out.status.assign(S, 0);
    out.k_used.assign(S * 3, 0.0);
    int32_t nv = 0, exact = 0;
    const int rc = sepaihrd_ensemble_predictive_targets(
        ctx, thetas.data(), static_cast<int>(S), replicates, seed, nullptr, observed_table ? observed_table->data() : nullptr, age_group.data(),
        window, origin, probs.data(), static_cast<int>(probs.size()), levels.data(), static_cast<int>(L), out.pred_quantiles.data(), out.pit.data(),
        out.target_scores.data(), out.summary.data(), out.target_obs.data(), out.target_draws.empty() ? nullptr : out.target_draws.data(),
        want_means ? out.means.data() : nullptr, out.draws.empty() ? nullptr : out.draws.data(), out.k_used.data(), out.status.data(), &nv, &exact);
    if (rc != SEPAIHRD_OK)
        throw ModelException("HipPosteriorPredictive", std::string("sepaihrd_ensemble_predictive_targets: ") + sepaihrd_last_error(ctx));
    out.samples_used = nv;
    out.exact = exact != 0;
    return out;
}

PosteriorPredictiveDraws HipPosteriorPredictive::draw(const std::vector<Eigen::VectorXd>& param_samples, int num_samples_for_ppc,
                                                      unsigned int random_seed, int replicates, std::uint64_t seed,
                                                      const std::vector<double>& probs, bool want_means, bool want_draws) {
    PosteriorPredictiveDraws out;
    const std::vector<double> thetas = selectedThetas(param_samples, num_samples_for_ppc, random_seed, replicates, probs, out);
    if (thetas.empty()) return out;
    const size_t S = out.selected.size();
    sepaihrd_ctx* ctx = objective_->deviceContext();
    objective_->syncDeviceConstraintMode();
    const size_t cells = static_cast<size_t>(3) * t_pos_ * n_;
    out.pred_quantiles.assign(2 * cells * probs.size(), 0.0);
    out.pit.assign(cells, 0.0);
    if (want_means) out.means.assign(S * cells, 0.0);
    if (want_draws && replicates > 0) out.draws.assign(S * static_cast<size_t>(replicates) * cells, 0.0);
    out.status.assign(S, 0);
    int32_t nv = 0;
    // a dispersed objective (fixed values or calibrated dispersion_* names): the replicates carry its negative-binomial noise
    double fixed_k[3];
    bool dispersed = sepaihrd_get_dispersion(ctx, fixed_k) == SEPAIHRD_OK;
    if (dispersed) dispersed = !(std::isinf(fixed_k[0]) && std::isinf(fixed_k[1]) && std::isinf(fixed_k[2]));  // NaN: calibrated
    int rc;
    if (dispersed) {
        out.k_used.assign(S * 3, 0.0);
        rc = sepaihrd_ensemble_predictive_nb(ctx, thetas.data(), static_cast<int>(S), replicates, seed, nullptr, probs.data(),
                                             static_cast<int>(probs.size()), out.pred_quantiles.data(), out.pit.data(),
                                             want_means ? out.means.data() : nullptr, out.draws.empty() ? nullptr : out.draws.data(),
                                             out.k_used.data(), out.status.data(), &nv);
    } else {
        rc = sepaihrd_ensemble_predictive(ctx, thetas.data(), static_cast<int>(S), replicates, seed, probs.data(),
                                          static_cast<int>(probs.size()), out.pred_quantiles.data(), out.pit.data(),
                                          want_means ? out.means.data() : nullptr, out.draws.empty() ? nullptr : out.draws.data(),
                                          out.status.data(), &nv);
    }
    if (rc != SEPAIHRD_OK)
        throw ModelException("HipPosteriorPredictive", std::string("sepaihrd_ensemble_predictive: ") + sepaihrd_last_error(ctx));
    out.samples_used = nv;
    return out;
}

}  // namespace epidemic
