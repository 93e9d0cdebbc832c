// host/src/HipStochasticSEPAIHRD.cpp -- HipStochasticSEPAIHRD and the CPU twin of sepaihrd_ensemble_stochastic's step, sort and
// quantile passes.  The model, its interval walk (all_ages_interval), the stream and the sampler are
// csrc/sepaihrd_stoch_sepaihrd.inc and csrc/sepaihrd_stoch.inc, the text the kernel compiles; what this twin shares with the
// particle filter's is host/src/StochasticSEPAIHRDTwin.hpp; this library is built with -ffp-contract=off like the kernel.
#include "epidemic_hip/HipStochasticSEPAIHRD.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

#include "StochasticSEPAIHRDTwin.hpp"
#include "sepaihrd_hip.h"
#include "sepaihrd_quantile.inc"  // the quantile rule of the predictive twin

namespace epidemic {

namespace epi = sepaihrd_stoch_epi;

int hostStochasticSEPAIHRD(const StochasticSEPAIHRDFixedData& pb, const double* model_values, const int32_t* status, int S, int R,
                           int steps_per_interval, std::uint64_t seed, const double* probs, int n_probs, int keep, double* quantiles,
                           double* extinct, double* traj, double* final_state, std::string* error) {
    char msg[256] = "";
    const stoch_twin::Plan plan = stoch_twin::plan(pb);
    const int vrc = stoch_twin::verdict(
        "ensemble_stochastic",
        sepaihrd_stochastic_validate(S, R, steps_per_interval, keep, pb.n_times, plan.T_pos, pb.n_age, probs, n_probs, msg, (int)sizeof(msg)), msg,
        {{!model_values || !status || !quantiles, "model_values, status and quantiles must not be NULL"},
         {stoch_twin::fixed_data_missing(pb), stoch_twin::FIXED_DATA_TEXT},
         {pb.n_age > epi::MAX_AGES, "built for at most 16 age classes"},
         {keep > 0 && !traj, "keep > 0 needs traj"}},
        error);
    if (vrc != SEPAIHRD_OK) return vrc;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const int n = pb.n_age, T = pb.n_times, m = steps_per_interval, runup_offset = plan.runup_offset;
    const size_t Tp = (size_t)plan.T_pos, nn = (size_t)n, W = plan.W, row_doubles = plan.row_doubles;
    const epi::RowLayout L = plan.L;
    std::vector<int> valid;  // positions of the valid samples
    for (int s = 0; s < S; ++s)
        if (status[s] == 0) valid.push_back(s);
    const size_t nd = valid.size() * (size_t)R;  // values per segment
    for (int s = 0; s < S; ++s)
        if (status[s] != 0) {
            stoch_twin::nan_fill(traj, (size_t)s * keep * T * row_doubles, (size_t)keep * T * row_doubles);
            stoch_twin::nan_fill(final_state, (size_t)s * R * row_doubles, (size_t)R * row_doubles);
        }
    // the daily increments of every replicate: inc[d][series][t][age], exact in int32
    std::vector<int32_t> inc(nd * 3 * Tp * nn);
    std::vector<uint8_t> died_out(nd, 0);
#pragma omp parallel for schedule(static)
    for (long long d = 0; d < (long long)nd; ++d) {
        const size_t s = (size_t)valid[(size_t)d / (size_t)R];
        const uint32_t r = (uint32_t)((size_t)d % (size_t)R);
        const double* row = model_values + s * W;
        int32_t x[epi::MAX_AGES][epi::NUM_COMP];
        int32_t prev[epi::MAX_AGES][epi::NUM_PREV];
        epi::AgeProbs q[epi::MAX_AGES];
        for (int i = 0; i < n; ++i) {
            for (int c = 0; c < epi::NUM_COMP; ++c) x[i][c] = (int32_t)row[L.initial(c, i)];
            prev[i][0] = x[i][epi::C_CUM_H]; prev[i][1] = x[i][epi::C_CUM_ICU]; prev[i][2] = x[i][epi::C_D];
        }
        double* tr = (traj && r < (uint32_t)keep) ? traj + ((s * (size_t)keep + r) * T) * row_doubles : nullptr;
        int32_t* my_inc = inc.data() + (size_t)d * 3 * Tp * nn;
        auto write_row = [&](int k) {
            for (int i = 0; i < n; ++i) {
                if (tr)
                    for (int c = 0; c < epi::NUM_COMP; ++c) tr[(size_t)k * row_doubles + (size_t)c * nn + i] = (double)x[i][c];
                int32_t since[epi::NUM_PREV];
                epi::take_increments(x[i], prev[i], since);
                for (int ser = 0; ser < 3 && k >= runup_offset; ++ser) my_inc[((size_t)ser * Tp + (size_t)(k - runup_offset)) * nn + i] = since[ser];
            }
        };
        write_row(0);
        for (int k = 0; k + 1 < T; ++k) {
            const double t0 = pb.times[k];
            const double h = (pb.times[k + 1] - t0) / (double)m;
            for (int i = 0; i < n; ++i) q[i] = epi::age_probs(row, L, i, h);
            epi::all_ages_interval(x[0], epi::NUM_COMP, row, L, pb.N, pb.M, pb.beta_end_times, pb.kappa_end_times, t0, h, q, m, seed, (uint32_t)s, r,
                                   (uint32_t)(k * m));
            write_row(k + 1);
        }
        bool infected = false;
        for (int i = 0; i < n; ++i) {
            infected = infected || (x[i][epi::C_E] | x[i][epi::C_P] | x[i][epi::C_A] | x[i][epi::C_I]) != 0;
            if (final_state)
                for (int c = 0; c < epi::NUM_COMP; ++c) final_state[(s * (size_t)R + r) * row_doubles + (size_t)c * nn + i] = (double)x[i][c];
        }
        died_out[(size_t)d] = infected ? 0 : 1;
    }
    if (extinct) {
        for (int s = 0; s < S; ++s) extinct[s] = qnan;
        for (size_t v = 0; v < valid.size(); ++v) {
            int32_t count = 0;
            for (int r = 0; r < R; ++r) count += died_out[v * (size_t)R + r];
            extinct[valid[v]] = (double)count / (double)R;
        }
    }
    // one age class at a time: its 6 T_pos segments of nd values
    std::vector<double> seg((size_t)6 * Tp * nd);
    for (size_t a = 0; a < nn; ++a) {
#pragma omp parallel for schedule(static)
        for (long long d = 0; d < (long long)nd; ++d) {
            const int32_t* my_inc = inc.data() + (size_t)d * 3 * Tp * nn;
            for (size_t ser = 0; ser < 3; ++ser) {
                double run = 0.0;
                for (size_t t = 0; t < Tp; ++t) {
                    const double y = (double)my_inc[(ser * Tp + t) * nn + a];
                    run += y;
                    seg[(ser * Tp + t) * nd + (size_t)d] = y;
                    seg[((ser + 3) * Tp + t) * nd + (size_t)d] = run;
                }
            }
        }
#pragma omp parallel for schedule(dynamic, 4)
        for (long long sg = 0; sg < (long long)(6 * Tp); ++sg) {
            const size_t ser = (size_t)sg / Tp, t = (size_t)sg % Tp;
            double* xs = seg.data() + (size_t)sg * nd;
            std::sort(xs, xs + nd);
            for (int p = 0; p < n_probs; ++p)
                quantiles[((ser * (size_t)n_probs + (size_t)p) * Tp + t) * nn + a] = nd > 0 ? sepaihrd_quantile::sorted_quantile(xs, nd, probs[p]) : qnan;
        }
    }
    return SEPAIHRD_OK;
}

HipStochasticSEPAIHRD::HipStochasticSEPAIHRD(HipSEPAIHRDParameterManager& parameterManager, const CalibrationData& observed_data,
                                             const std::vector<double>& time_points, const Eigen::VectorXd& initial_state,
                                             std::shared_ptr<IOdeSolverStrategy> solver_strategy, int device, int initial_state_mode)
    : pm_(parameterManager), data_(observed_data), time_points_(time_points), cache_(1) {
    objective_ = stoch_twin::make_objective("HipStochasticSEPAIHRD", pm_, cache_, data_, time_points_, initial_state, std::move(solver_strategy),
                                            device, initial_state_mode);
    n_ = static_cast<int>(pm_.modelParameters().N.size());
    for (double t : time_points_) t_pos_ += (t >= 0.0);
}

StochasticSEPAIHRDResult HipStochasticSEPAIHRD::run(const std::vector<Eigen::VectorXd>& param_samples, int num_samples,
                                                    unsigned int random_seed, int replicates, int steps_per_interval, std::uint64_t seed,
                                                    const std::vector<double>& probs) {
    StochasticSEPAIHRDResult out;
    for (double t : time_points_)
        if (t >= 0.0) out.time_points.push_back(t);
    out.n_age = n_;
    out.replicates = replicates;
    out.steps_per_interval = steps_per_interval;
    out.probs = probs;
    if (out.time_points.empty() || param_samples.empty()) return out;
    out.selected = HipPosteriorEnsemble::selectSamples(param_samples.size(), num_samples, random_seed);
    const size_t P = pm_.getParameterCount(), S = out.selected.size();
    std::vector<double> thetas(S * P);
    for (size_t s = 0; s < S; ++s) {
        const Eigen::VectorXd& v = param_samples[static_cast<size_t>(out.selected[s])];
        if (static_cast<size_t>(v.size()) != P) throw InvalidParameterException("HipStochasticSEPAIHRD", "sample size mismatch");
        for (size_t i = 0; i < P; ++i) thetas[s * P + i] = v[static_cast<Eigen::Index>(i)];
    }
    sepaihrd_ctx* ctx = objective_->deviceContext();
    objective_->syncDeviceConstraintMode();
    out.quantiles.assign(static_cast<size_t>(6) * probs.size() * t_pos_ * n_, 0.0);
    out.extinct.assign(S, 0.0);
    out.status.assign(S, 0);
    int32_t nv = 0;
    const int rc = sepaihrd_ensemble_stochastic(ctx, thetas.data(), static_cast<int>(S), replicates, steps_per_interval, seed, probs.data(),
                                                static_cast<int>(probs.size()), 0, out.quantiles.data(), out.extinct.data(), nullptr, nullptr,
                                                nullptr, out.status.data(), &nv);
    if (rc != SEPAIHRD_OK)
        throw ModelException("HipStochasticSEPAIHRD", std::string("sepaihrd_ensemble_stochastic: ") + sepaihrd_last_error(ctx));
    out.samples_used = nv;
    return out;
}

}  // namespace epidemic
