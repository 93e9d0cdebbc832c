// host/src/HipParticleFilter.cpp -- HipParticleLikelihood and the CPU twin of sepaihrd_particle_loglik's filter kernel.  The
// filter's rules are csrc/sepaihrd_particle.inc, the model, the stream and the sampler csrc/sepaihrd_stoch_sepaihrd.inc and
// csrc/sepaihrd_stoch.inc: the text the kernel compiles; this library is built with -ffp-contract=off like the kernel.
#include "epidemic_hip/HipParticleFilter.hpp"

#include <algorithm>
#include <cstdio>
#include <limits>

#include "sepaihrd_hip.h"
#include "sepaihrd_particle.inc"

namespace epidemic {

namespace epi = sepaihrd_stoch_epi;
namespace pf = sepaihrd_particle;

int hostParticleLoglik(const StochasticSEPAIHRDFixedData& pb, const ParticleObservations& obs, const double* model_values,
                       const int32_t* status, int B, int J, int steps_per_interval, std::uint64_t seed, double* loglik, double* increments,
                       double* ess, double* final_state, std::string* error) {
    char msg[256] = "";
    int T_pos = 0;
    for (int k = 0; k < pb.n_times && pb.times; ++k) T_pos += pb.times[k] >= 0.0;
    int vrc = sepaihrd_particle_validate(B, J, steps_per_interval, pb.n_times, T_pos, pb.n_age, msg, (int)sizeof(msg));
    auto refuse = [&](const char* what) {
        std::snprintf(msg, sizeof(msg), "particle_loglik: %s", what);
        vrc = SEPAIHRD_E_INVALID_ARG;
    };
    if (vrc == SEPAIHRD_OK && (!model_values || !status || !loglik)) refuse("model_values, status and loglik must not be NULL");
    if (vrc == SEPAIHRD_OK && (!pb.N || !pb.M || !pb.kappa_end_times || pb.n_kappa < 1 || pb.n_beta < 0 || (pb.n_beta > 0 && !pb.beta_end_times)))
        refuse("the fixed data need N, M and the schedule end times (n_kappa >= 1)");
    if (vrc == SEPAIHRD_OK && (obs.n_obs < 0 || (obs.n_obs > 0 && (!obs.obs_H || !obs.obs_ICU || !obs.obs_D))))
        refuse("the observations need obs_H, obs_ICU and obs_D");
    if (vrc != SEPAIHRD_OK) {
        if (error) *error = msg;
        return vrc;
    }
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const int n = pb.n_age, T = pb.n_times, m = steps_per_interval;
    const size_t Tp = (size_t)T_pos, nn = (size_t)n;
    const int runup_offset = T - T_pos;  // the times increase: the output times >= 0 are the last T_pos
    const epi::RowLayout L{n, pb.n_beta, pb.n_kappa};
    const size_t W = (size_t)L.width();
    const size_t row_doubles = (size_t)epi::NUM_COMP * nn;
    // the observation of (series, output row t, age), NaN where there is none
    auto observed = [&](const double* series, int t, int i) { return t < obs.n_obs ? series[(size_t)t * nn + (size_t)i] : qnan; };
#pragma omp parallel for schedule(dynamic, 1)
    for (int b = 0; b < B; ++b) {
        double* my_inc = increments ? increments + (size_t)b * Tp : nullptr;
        double* my_ess = ess ? ess + (size_t)b * Tp : nullptr;
        double* my_final = final_state ? final_state + (size_t)b * J * row_doubles : nullptr;
        if (status[b] != 0) {
            loglik[b] = std::numeric_limits<double>::lowest();
            if (my_inc) std::fill(my_inc, my_inc + Tp, qnan);
            if (my_ess) std::fill(my_ess, my_ess + Tp, qnan);
            if (my_final) std::fill(my_final, my_final + (size_t)J * row_doubles, qnan);
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
                x[epi::NUM_COMP + 0] = x[epi::C_CUM_H]; x[epi::NUM_COMP + 1] = x[epi::C_CUM_ICU]; x[epi::NUM_COMP + 2] = x[epi::C_D];
            }
        double lambda[epi::MAX_AGES], pressure[epi::MAX_AGES];
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
                for (int s = 0; k > 0 && s < m; ++s) {
                    const double t_mid = t0 + ((double)s + 0.5) * h;
                    const double bk = epi::beta_kappa(row, L, pb.beta_end_times, pb.kappa_end_times, t_mid);
                    for (int i = 0; i < n; ++i)
                        pressure[i] = epi::infectious_pressure(x_of(state, j, i), row[epi::R_THETA], row[L.vec(epi::V_H_INFEC, i)], pb.N[i]);
                    for (int i = 0; i < n; ++i) {
                        double sum = 0.0;
                        for (int jj = 0; jj < n; ++jj) sum += pb.M[(size_t)i * nn + jj] * pressure[jj];
                        lambda[i] = epi::force_of_infection(sum, bk, row[L.vec(epi::V_A, i)]);
                    }
                    for (int i = 0; i < n; ++i)
                        epi::age_step(x_of(state, j, i), lambda[i], h, q[i], seed, (uint32_t)b, (uint32_t)j, (uint32_t)((k - 1) * m + s), (uint32_t)i);
                }
                double sum = 0.0;
                for (int i = 0; i < n; ++i) {
                    int32_t* x = x_of(state, j, i);
                    const int32_t incH = x[epi::C_CUM_H] - x[epi::NUM_COMP + 0], incICU = x[epi::C_CUM_ICU] - x[epi::NUM_COMP + 1],
                                  incD = x[epi::C_D] - x[epi::NUM_COMP + 2];
                    x[epi::NUM_COMP + 0] = x[epi::C_CUM_H]; x[epi::NUM_COMP + 1] = x[epi::C_CUM_ICU]; x[epi::NUM_COMP + 2] = x[epi::C_D];
                    if (weighted) sum += pf::age_term(observed(obs.obs_H, t, i), observed(obs.obs_ICU, t, i), observed(obs.obs_D, t, i), incH, incICU, incD);
                }
                lw[(size_t)j] = sum;
            }
            if (weighted) {
                double inc = 0.0, e = qnan;
                pf::normalise_and_resample(lw.data(), J, pf::resample_uniform(seed, (uint32_t)b, (uint32_t)k), C.data(), Q.data(), anc.data(), inc, e);
                for (int j = 0; j < J; ++j) std::copy_n(state.data() + (size_t)anc[(size_t)j] * per, per, next.data() + (size_t)j * per);
                state.swap(next);
                total += inc;
                if (my_inc) my_inc[t] = inc;
                if (my_ess) my_ess[t] = e;
            } else if (t >= 0) {
                if (my_inc) my_inc[t] = 0.0;
                if (my_ess) my_ess[t] = qnan;
            }
        }
        loglik[b] = total;
        if (my_final)
            for (int j = 0; j < J; ++j)
                for (int i = 0; i < n; ++i)
                    for (int c = 0; c < epi::NUM_COMP; ++c) my_final[(size_t)j * row_doubles + (size_t)c * nn + (size_t)i] = (double)x_of(state, j, i)[c];
    }
    return SEPAIHRD_OK;
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
      steps_per_interval_(steps_per_interval), seed0_(seed0) {
    objective_ = std::make_unique<HipSEPAIHRDObjectiveFunction>(pm_, cache_, data_, time_points_, initial_state, std::move(solver_strategy),
                                                                1.0e-6, 1.0e-6, device, false);
    if (sepaihrd_set_initial_state_mode(objective_->deviceContext(), initial_state_mode) != SEPAIHRD_OK)
        throw ModelException("HipParticleLikelihood", "sepaihrd_set_initial_state_mode failed");
}

void HipParticleLikelihood::calculateBatch(const double* thetas, int B, double* out, int* status) const {
    sepaihrd_ctx* ctx = objective_->deviceContext();
    objective_->syncDeviceConstraintMode();
    std::vector<int32_t> st((size_t)std::max(B, 1), 0);
    const std::uint64_t seed = seed0_ + calls_;
    const int rc = sepaihrd_particle_loglik(ctx, thetas, B, particles_, steps_per_interval_, seed, out, nullptr, nullptr, nullptr, nullptr, st.data(),
                                            nullptr);
    if (rc != SEPAIHRD_OK) throw ModelException("HipParticleLikelihood", std::string("sepaihrd_particle_loglik: ") + sepaihrd_last_error(ctx));
    ++calls_;
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
