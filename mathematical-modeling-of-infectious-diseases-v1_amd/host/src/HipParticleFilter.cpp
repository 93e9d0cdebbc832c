// host/src/HipParticleFilter.cpp -- HipParticleLikelihood and the CPU twin of sepaihrd_particle_loglik's filter kernel.  The
// filter's rules are csrc/sepaihrd_particle.inc, the model, its interval walk (all_ages_interval), the stream and the sampler
// csrc/sepaihrd_stoch_sepaihrd.inc and csrc/sepaihrd_stoch.inc: the text the kernel compiles; what this twin shares with
// hostStochasticSEPAIHRD is host/src/StochasticSEPAIHRDTwin.hpp; this library is built with -ffp-contract=off like the kernel.
#include "epidemic_hip/HipParticleFilter.hpp"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <limits>

#include "StochasticSEPAIHRDTwin.hpp"
#include "sepaihrd_hip.h"
#include "sepaihrd_particle.inc"
#include "sepaihrd_particle_nb_host.h"
#include "sepaihrd_particle_states.inc"

namespace epidemic {

namespace epi = sepaihrd_stoch_epi;
namespace pf = sepaihrd_particle;
namespace ps = sepaihrd_particle_states;

namespace {

// The filter's walk over B parameter vectors, after the arguments have been accepted: what hostParticleLoglik and
// hostParticleLoglikWide both are, and their negative-binomial forms.  Nothing in it depends on how large J is.  disp is the
// dispersion of the observed series (NO_DISPERSION: every series Poisson); row_const the row constants G [T_pos] of a call with
// a dispersed series, null where there is none.  row_sink (optional): called once per output row k of every valid theta b with
// the cloud of csrc/sepaihrd_particle_states.inc -- the J particles the next interval starts from, after the resampling's copy
// where the row is weighted; count c of (particle j, age i) at cloud[j per + i stride + c].
using RowSink = std::function<void(int b, int k, const int32_t* cloud, size_t per, size_t stride)>;
constexpr pf::Dispersion NO_DISPERSION{std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(),
                                       std::numeric_limits<double>::infinity()};
void particle_walk(const StochasticSEPAIHRDFixedData& pb, const stoch_twin::Plan& plan, const ParticleObservations& obs, const double* model_values,
                   const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, const pf::Dispersion& disp, const double* row_const,
                   double* loglik, double* increments, double* ess, double* final_state, const RowSink& row_sink = nullptr) {
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const int n = pb.n_age, T = pb.n_times, m = steps_per_interval, runup_offset = plan.runup_offset;
    const size_t Tp = (size_t)plan.T_pos, nn = (size_t)n, W = plan.W, row_doubles = plan.row_doubles;
    const epi::RowLayout L = plan.L;
    // the observation of (series, output row t, age), NaN where there is none
    auto observed = [&](const double* series, int t, int i) { return t < obs.n_obs ? series[(size_t)t * nn + (size_t)i] : qnan; };
#pragma omp parallel for schedule(dynamic, 1)
    for (int b = 0; b < B; ++b) {
        double* my_inc = increments ? increments + (size_t)b * Tp : nullptr;
        double* my_ess = ess ? ess + (size_t)b * Tp : nullptr;
        double* my_final = final_state ? final_state + (size_t)b * J * row_doubles : nullptr;
        if (status[b] != 0) {
            loglik[b] = std::numeric_limits<double>::lowest();
            stoch_twin::nan_fill(my_inc, 0, Tp);
            stoch_twin::nan_fill(my_ess, 0, Tp);
            stoch_twin::nan_fill(my_final, 0, (size_t)J * row_doubles);
            continue;
        }
        const double* row = model_values + (size_t)b * W;
        // particle j: x[j][age][11], prev[j][age][3]; `next` receives the resampled copy
        const size_t per = nn * (epi::NUM_COMP + pf::NUM_PREV);
        std::vector<int32_t> state((size_t)J * per), next((size_t)J * per), anc((size_t)J);
        std::vector<double> lw((size_t)J), C((size_t)J), Q((size_t)J);
        auto x_of = [&](std::vector<int32_t>& s, int j, int i) { return s.data() + (size_t)j * per + (size_t)i * (epi::NUM_COMP + pf::NUM_PREV); };
        for (int j = 0; j < J; ++j)
            for (int i = 0; i < n; ++i) {
                int32_t* x = x_of(state, j, i);
                for (int c = 0; c < epi::NUM_COMP; ++c) x[c] = (int32_t)row[L.initial(c, i)];
                int32_t none[epi::NUM_PREV];
                epi::take_increments(x, x + epi::NUM_COMP, none);  // previous row := the initial counts (`state` starts as zeros)
            }
        epi::AgeProbs q[epi::MAX_AGES];
        double total = 0.0;
        for (int k = 0; k < T; ++k) {
            const int t = k - runup_offset;
            bool weighted = false;
            for (int i = 0; i < n && t >= 0; ++i)
                weighted = weighted || pf::usable(observed(obs.obs_H, t, i)) || pf::usable(observed(obs.obs_ICU, t, i)) || pf::usable(observed(obs.obs_D, t, i));
            double h = 0.0, t0 = 0.0;
            if (k > 0) {
                t0 = pb.times[k - 1];
                h = (pb.times[k] - t0) / (double)m;
                for (int i = 0; i < n; ++i) q[i] = epi::age_probs(row, L, i, h);
            }
            for (int j = 0; j < J; ++j) {
                if (k > 0)
                    epi::all_ages_interval(x_of(state, j, 0), epi::NUM_COMP + pf::NUM_PREV, row, L, pb.N, pb.M, pb.beta_end_times, pb.kappa_end_times, t0,
                                           h, q, m, seed, (uint32_t)b, (uint32_t)j, (uint32_t)((k - 1) * m));
                double sum = 0.0;
                for (int i = 0; i < n; ++i) {
                    int32_t* x = x_of(state, j, i);
                    int32_t inc[epi::NUM_PREV];
                    epi::take_increments(x, x + epi::NUM_COMP, inc);
                    if (weighted) sum += pf::age_term(observed(obs.obs_H, t, i), observed(obs.obs_ICU, t, i), observed(obs.obs_D, t, i), inc[0], inc[1], inc[2], disp);
                }
                lw[(size_t)j] = sum;
            }
            if (weighted) {
                double inc = 0.0, e = qnan;
                pf::normalise_and_resample(lw.data(), J, pf::resample_uniform(seed, (uint32_t)b, (uint32_t)k), C.data(), Q.data(), anc.data(), inc, e);
                for (int j = 0; j < J; ++j) std::copy_n(state.data() + (size_t)anc[(size_t)j] * per, per, next.data() + (size_t)j * per);
                state.swap(next);
                if (row_const) inc = pf::increment_with_constant(inc, row_const[t]);
                total += inc;
                if (my_inc) my_inc[t] = inc;
                if (my_ess) my_ess[t] = e;
            } else if (t >= 0) {
                if (my_inc) my_inc[t] = 0.0;
                if (my_ess) my_ess[t] = qnan;
            }
            if (row_sink) row_sink(b, k, state.data(), per, epi::NUM_COMP + pf::NUM_PREV);
        }
        loglik[b] = total;
        if (my_final)
            for (int j = 0; j < J; ++j)
                for (int i = 0; i < n; ++i)
                    for (int c = 0; c < epi::NUM_COMP; ++c) my_final[(size_t)j * row_doubles + (size_t)c * nn + (size_t)i] = (double)x_of(state, j, i)[c];
    }
}

// the observation of (series, output row t >= 0, age), NaN where there is none: the cells of the row constants
double observed_cell(const ParticleObservations& obs, int n_age, int series, int t, int age) {
    const double* table = series == 0 ? obs.obs_H : series == 1 ? obs.obs_ICU : obs.obs_D;
    return t < obs.n_obs ? table[(size_t)t * (size_t)n_age + (size_t)age] : std::numeric_limits<double>::quiet_NaN();
}

// Every twin after its form's validator (vrc, msg): what the walk itself needs, then the dispersion of a negative-binomial form
// (nb) with its row constants, then the walk.  A Poisson form passes no dispersion and never meets sepaihrd_particle_nb_validate.
int particle_twin(const char* who, int vrc, char (&msg)[256], const StochasticSEPAIHRDFixedData& pb, const stoch_twin::Plan& plan,
                  const ParticleObservations& obs, const double* model_values, const int32_t* status, int B, int J, int steps_per_interval,
                  std::uint64_t seed, bool nb, const double* dispersion, double* loglik, double* increments, double* ess, double* final_state,
                  std::string* error, const RowSink& row_sink = nullptr) {
    vrc = stoch_twin::verdict(
        who, vrc, msg,
        {{!model_values || !status || !loglik, "model_values, status and loglik must not be NULL"},
         {stoch_twin::fixed_data_missing(pb), stoch_twin::FIXED_DATA_TEXT},
         {obs.n_obs < 0 || (obs.n_obs > 0 && (!obs.obs_H || !obs.obs_ICU || !obs.obs_D)), "the observations need obs_H, obs_ICU and obs_D"}},
        error);
    if (vrc != SEPAIHRD_OK) return vrc;
    pf::Dispersion d = NO_DISPERSION;
    std::vector<double> G;
    if (nb) {
        if (sepaihrd_particle_nb_validate(dispersion, msg, (int)sizeof(msg)) != SEPAIHRD_OK) {
            if (error) *error = msg;
            return SEPAIHRD_E_INVALID_ARG;
        }
        d = pf::Dispersion{dispersion[0], dispersion[1], dispersion[2]};
        if (pf::any_dispersed(d)) {
            G.resize((size_t)plan.T_pos);
            pf::nb_row_constants(d, pb.n_age, plan.T_pos, [&](int series, int t, int age) { return observed_cell(obs, pb.n_age, series, t, age); }, G.data());
        }
    }
    particle_walk(pb, plan, obs, model_values, status, B, J, steps_per_interval, seed, d, G.empty() ? nullptr : G.data(), loglik, increments, ess,
                  final_state, row_sink);
    return SEPAIHRD_OK;
}

}  // namespace

int hostParticleLoglik(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                       const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, double* loglik, double* increments,
                       double* ess, double* final_state, std::string* error) {
    char msg[256] = "";
    const stoch_twin::Plan plan = stoch_twin::plan(pb);
    return particle_twin("particle_loglik", sepaihrd_particle_validate(B, J, steps_per_interval, pb.n_times, plan.T_pos, pb.n_age, msg, (int)sizeof(msg)),
                         msg, pb, plan, obs, model_values, status, B, J, steps_per_interval, seed, false, nullptr, loglik, increments, ess, final_state,
                         error);
}

int hostParticleLoglikWide(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                           const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, double* loglik, double* increments,
                           double* ess, double* final_state, std::string* error) {
    char msg[256] = "";
    const stoch_twin::Plan plan = stoch_twin::plan(pb);
    return particle_twin("particle_loglik_wide",
                         sepaihrd_particle_wide_validate(B, J, steps_per_interval, 0, pb.n_times, plan.T_pos, pb.n_age, msg, (int)sizeof(msg)), msg, pb,
                         plan, obs, model_values, status, B, J, steps_per_interval, seed, false, nullptr, loglik, increments, ess, final_state, error);
}

int hostParticleLoglikNB(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                         const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, const double* dispersion, double* loglik,
                         double* increments, double* ess, double* final_state, std::string* error) {
    char msg[256] = "";
    const stoch_twin::Plan plan = stoch_twin::plan(pb);
    return particle_twin("particle_loglik_nb", sepaihrd_particle_validate(B, J, steps_per_interval, pb.n_times, plan.T_pos, pb.n_age, msg, (int)sizeof(msg)),
                         msg, pb, plan, obs, model_values, status, B, J, steps_per_interval, seed, true, dispersion, loglik, increments, ess, final_state,
                         error);
}

int hostParticleLoglikWideNB(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                             const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, const double* dispersion, double* loglik,
                             double* increments, double* ess, double* final_state, std::string* error) {
    char msg[256] = "";
    const stoch_twin::Plan plan = stoch_twin::plan(pb);
    return particle_twin("particle_loglik_wide_nb",
                         sepaihrd_particle_wide_validate(B, J, steps_per_interval, 0, pb.n_times, plan.T_pos, pb.n_age, msg, (int)sizeof(msg)), msg, pb,
                         plan, obs, model_values, status, B, J, steps_per_interval, seed, true, dispersion, loglik, increments, ess, final_state, error);
}

int hostParticleStates(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values, const int32_t* status,
                       int B, int J, int steps_per_interval, std::uint64_t seed, const double* dispersion, const double* probs, int n_probs,
                       double* loglik, double* increments, double* ess, double* state_mean, double* state_quantiles, std::string* error) {
    char msg[256] = "";
    const stoch_twin::Plan plan = stoch_twin::plan(pb);
    int vrc = sepaihrd_particle_states_validate(B, J, steps_per_interval, 0, pb.n_times, plan.T_pos, pb.n_age, probs, n_probs, msg, (int)sizeof(msg));
    if (vrc == SEPAIHRD_OK && (!state_mean || (state_quantiles && n_probs == 0))) {
        std::snprintf(msg, sizeof(msg), "particle_filter_states: %s", !state_mean ? "need theta, loglik and state_mean" : "state_quantiles needs n_probs > 0");
        vrc = SEPAIHRD_E_INVALID_ARG;
    }
    const size_t series = (size_t)pb.n_age + 1, cells = (size_t)epi::NUM_COMP * series, row_cells = (size_t)std::max(pb.n_times, 0) * cells;
    // the summary of one row: per (count, series) the J values, their sum in 64-bit integers, std::sort, the quantile expression
    const RowSink sink = [&](int b, int k, const int32_t* cloud, size_t per, size_t stride) {
        std::vector<double> v((size_t)J);
        for (int c = 0; c < epi::NUM_COMP; ++c)
            for (size_t a = 0; a < series; ++a) {
                int64_t sum = 0;
                for (int j = 0; j < J; ++j) {
                    const int32_t* x = cloud + (size_t)j * per;
                    int64_t value = 0;
                    if (a < (size_t)pb.n_age)
                        value = x[a * stride + (size_t)c];
                    else
                        for (int i = 0; i < pb.n_age; ++i) value += x[(size_t)i * stride + (size_t)c];
                    v[(size_t)j] = (double)value;
                    sum += value;
                }
                const size_t cell = ((size_t)b * (size_t)pb.n_times + (size_t)k) * cells + (size_t)c * series + a;
                state_mean[cell] = ps::mean_of(sum, J);
                if (state_quantiles) {
                    std::sort(v.begin(), v.end());
                    for (int p = 0; p < n_probs; ++p) state_quantiles[cell * (size_t)n_probs + (size_t)p] = sepaihrd_quantile::sorted_quantile(v.data(), (size_t)J, probs[p]);
                }
            }
    };
    const int rc = particle_twin("particle_filter_states", vrc, msg, pb, plan, obs, model_values, status, B, J, steps_per_interval, seed,
                                 dispersion != nullptr, dispersion, loglik, increments, ess, nullptr, error, sink);
    if (rc != SEPAIHRD_OK) return rc;
    for (int b = 0; b < B; ++b)
        if (status[b] != 0) {
            stoch_twin::nan_fill(state_mean + (size_t)b * row_cells, 0, row_cells);
            if (state_quantiles) stoch_twin::nan_fill(state_quantiles + (size_t)b * row_cells * (size_t)n_probs, 0, row_cells * (size_t)n_probs);
        }
    return SEPAIHRD_OK;
}

int hostParticleNBRowConstants(const ParticleObservations& obs, int n_age, int T_pos, const double* dispersion, double* G, std::string* error) {
    char msg[256] = "";
    if (sepaihrd_particle_nb_validate(dispersion, msg, (int)sizeof(msg)) != SEPAIHRD_OK) {
        if (error) *error = msg;
        return SEPAIHRD_E_INVALID_ARG;
    }
    pf::nb_row_constants(pf::Dispersion{dispersion[0], dispersion[1], dispersion[2]}, n_age, T_pos,
                         [&](int series, int t, int age) { return observed_cell(obs, n_age, series, t, age); }, G);
    return SEPAIHRD_OK;
}

void hostParticleNBTerm(const double* obs, const int32_t* inc, int count, double k, double* out) {
    for (int i = 0; i < count; ++i) out[i] = pf::nb_term(obs[i], inc[i], k);
}

void hostParticleResample(std::uint64_t seed, std::uint32_t b, std::uint32_t row, const double* logw, int J, int32_t* ancestors,
                          double* increment, double* ess) {
    std::vector<double> C((size_t)J), Q((size_t)J);
    pf::normalise_and_resample(logw, J, pf::resample_uniform(seed, b, row), C.data(), Q.data(), ancestors, *increment, *ess);
}

HipParticleLikelihood::HipParticleLikelihood(HipSEPAIHRDParameterManager& parameterManager, const CalibrationData& observed_data,
                                             const std::vector<double>& time_points, const Eigen::VectorXd& initial_state,
                                             std::shared_ptr<IOdeSolverStrategy> solver_strategy, int particles, int steps_per_interval,
                                             std::uint64_t seed0, int device, int initial_state_mode)
    : pm_(parameterManager), data_(observed_data), time_points_(time_points), cache_(1), particles_(particles),
      steps_per_interval_(steps_per_interval), n_age_((int)(initial_state.size() / epi::NUM_COMP)), seed0_(seed0) {
    objective_ = stoch_twin::make_objective("HipParticleLikelihood", pm_, cache_, data_, time_points_, initial_state, std::move(solver_strategy), device,
                                            initial_state_mode);
}

void HipParticleLikelihood::setDispersion(double k_H, double k_ICU, double k_D) {
    const double d[3] = {k_H, k_ICU, k_D};
    char msg[256] = "";
    if (sepaihrd_particle_nb_validate(d, msg, (int)sizeof(msg)) != SEPAIHRD_OK) throw InvalidParameterException("HipParticleLikelihood", msg);
    std::copy_n(d, 3, dispersion_);
}

void HipParticleLikelihood::calculateBatch(const double* thetas, int B, double* out, int* status) const {
    sepaihrd_ctx* ctx = objective_->deviceContext();
    objective_->syncDeviceConstraintMode();
    std::vector<int32_t> st((size_t)std::max(B, 1), 0);
    const std::uint64_t seed = seed0_ + calls_;
    // up to the LDS kernel's limit that kernel, beyond it the wide form with the chunking left to the call: the same bits where
    // both take J, so the choice is one of speed alone
    const bool wide = particles_ > sepaihrd_particle_max_particles(n_age_);
    // the _nb call of that form once setDispersion has made some series dispersed
    const bool nb = pf::any_dispersed(pf::Dispersion{dispersion_[0], dispersion_[1], dispersion_[2]});
    int rc;
    if (nb)
        rc = wide ? sepaihrd_particle_loglik_wide_nb(ctx, thetas, B, particles_, steps_per_interval_, seed, dispersion_, 0, out, nullptr, nullptr, nullptr,
                                                     nullptr, st.data(), nullptr)
                  : sepaihrd_particle_loglik_nb(ctx, thetas, B, particles_, steps_per_interval_, seed, dispersion_, out, nullptr, nullptr, nullptr,
                                                nullptr, st.data(), nullptr);
    else
        rc = wide ? sepaihrd_particle_loglik_wide(ctx, thetas, B, particles_, steps_per_interval_, seed, 0, out, nullptr, nullptr, nullptr, nullptr,
                                                  st.data(), nullptr)
                  : sepaihrd_particle_loglik(ctx, thetas, B, particles_, steps_per_interval_, seed, out, nullptr, nullptr, nullptr, nullptr, st.data(),
                                             nullptr);
    if (rc != SEPAIHRD_OK)
        throw ModelException("HipParticleLikelihood", std::string(wide ? "sepaihrd_particle_loglik_wide" : "sepaihrd_particle_loglik") +
                                                          (nb ? "_nb: " : ": ") + sepaihrd_last_error(ctx));
    ++calls_;
    if (status) std::copy(st.begin(), st.begin() + B, status);
}

void HipParticleLikelihood::filterStates(const double* thetas, int B, const std::vector<double>& probs, std::vector<double>& state_mean,
                                         std::vector<double>& state_quantiles, std::vector<double>* loglik, int* status) const {
    sepaihrd_ctx* ctx = objective_->deviceContext();
    objective_->syncDeviceConstraintMode();
    const size_t cells = (size_t)std::max(B, 0) * time_points_.size() * epi::NUM_COMP * ((size_t)n_age_ + 1);
    state_mean.assign(cells, 0.0);
    state_quantiles.assign(cells * probs.size(), 0.0);
    std::vector<double> ll((size_t)std::max(B, 1));
    std::vector<int32_t> st((size_t)std::max(B, 1), 0);
    const bool nb = pf::any_dispersed(pf::Dispersion{dispersion_[0], dispersion_[1], dispersion_[2]});
    // the seed of the next calculateBatch; the call count stays
    const int rc = sepaihrd_particle_filter_states(ctx, thetas, B, particles_, steps_per_interval_, seed0_ + calls_, 0, nb ? dispersion_ : nullptr,
                                                   probs.empty() ? nullptr : probs.data(), (int)probs.size(), ll.data(), nullptr, nullptr,
                                                   state_mean.data(), probs.empty() ? nullptr : state_quantiles.data(), nullptr, st.data(), nullptr);
    if (rc != SEPAIHRD_OK) throw ModelException("HipParticleLikelihood", std::string("sepaihrd_particle_filter_states: ") + sepaihrd_last_error(ctx));
    if (loglik) loglik->assign(ll.begin(), ll.begin() + B);
    if (status) std::copy(st.begin(), st.begin() + B, status);
}

double HipParticleLikelihood::calculate(const Eigen::VectorXd& parameters) const {
    if (static_cast<size_t>(parameters.size()) != pm_.getParameterCount())
        throw InvalidParameterException("HipParticleLikelihood", "parameter vector size mismatch");
    std::vector<double> theta(static_cast<size_t>(parameters.size()));
    for (size_t i = 0; i < theta.size(); ++i) theta[i] = parameters[static_cast<Eigen::Index>(i)];
    double value = 0.0;
    calculateBatch(theta.data(), 1, &value, nullptr);
    return value;
}

}  // namespace epidemic
