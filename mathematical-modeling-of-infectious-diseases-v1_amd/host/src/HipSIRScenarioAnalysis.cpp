// HipSIRScenarioAnalysis.cpp -- see HipSIRScenarioAnalysis.hpp.
#include "epidemic_hip/HipSIRScenarioAnalysis.hpp"

#include <algorithm>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <sstream>

#include "sepaihrd_hip.h"

namespace epidemic {

int SIRScenario::kindOf(const std::string& name) {
    if (name == "contact_reduction" || name == "social_distancing" || name == "lockdown") return SEPAIHRD_SIR_EV_CONTACT;
    if (name == "mask_mandate" || name == "transmission_reduction") return SEPAIHRD_SIR_EV_TRANSMISSION;
    return -1;
}

void SIRScenario::validateParameters(const std::string& name, const Eigen::VectorXd& params) {
    const int kind = kindOf(name);
    if (kind < 0) return;  // the model validates (addIntervention refuses what it would refuse)
    if (params.size() != 1)
        throw InvalidParameterException("SIRScenario::validateParameters",
                                        "Intervention '" + name + "' requires exactly 1 parameter. Got " + std::to_string(params.size()) + ".");
    if (kind == SEPAIHRD_SIR_EV_CONTACT && params[0] < 0.0)
        throw InvalidParameterException("SIRScenario::validateParameters",
                                        "Contact scale factor for '" + name + "' cannot be negative. Got " + std::to_string(params[0]) + ".");
    if (kind == SEPAIHRD_SIR_EV_TRANSMISSION && (params[0] < 0.0 || params[0] > 1.0))
        throw InvalidParameterException("SIRScenario::validateParameters", "Transmission reduction factor for '" + name +
                                                                               "' must be between 0 and 1. Got " + std::to_string(params[0]) + ".");
}

SIRScenario::SIRScenario(std::string name, const std::vector<double>& timePoints) : name_(std::move(name)), times_(timePoints) {}

void SIRScenario::addIntervention(double time, const std::string& name, const Eigen::VectorXd& params) {
    if (time < 0)
        throw InvalidParameterException("SIRScenario::addIntervention", "Intervention time cannot be negative. Got: " + std::to_string(time));
    validateParameters(name, params);
    const int kind = kindOf(name);
    if (kind < 0) throw ModelException("SIRScenario::addIntervention", "Unknown intervention type: '" + name + "'.");
    if (!(params[0] == params[0]) || params[0] - params[0] != 0.0)
        throw InvalidParameterException("SIRScenario::addIntervention", "Parameter of intervention '" + name + "' is not finite.");
    const auto it = std::find(times_.begin(), times_.end(), time);
    if (it == times_.end())
        throw InvalidParameterException("SIRScenario::addIntervention", "Intervention time " + std::to_string(time) +
                                                                            " is not one of the output time points: interventions act on grid times only.");
    if (events_.size() >= static_cast<size_t>(SEPAIHRD_SIR_MAX_EVENTS))
        throw InvalidParameterException("SIRScenario::addIntervention",
                                        "Scenario '" + name_ + "' already holds " + std::to_string(SEPAIHRD_SIR_MAX_EVENTS) + " interventions.");
    const SIRInterventionEvent ev{static_cast<int32_t>(it - times_.begin()), kind, params[0]};
    const auto pos = std::upper_bound(events_.begin(), events_.end(), ev,
                                      [](const SIRInterventionEvent& a, const SIRInterventionEvent& b) { return a.time_index < b.time_index; });
    events_.insert(pos, ev);
}

std::vector<std::string> HipSIRScenarioAnalysis::metricNames(int n_age) {
    std::vector<std::string> names = {"R0", "peak_prevalence", "time_to_peak_prevalence", "peak_incidence", "time_to_peak_incidence",
                                      "overall_attack_rate"};
    for (int i = 0; i < n_age; ++i) {
        names.push_back("attack_rate_age_" + std::to_string(i));
        names.push_back("peak_prevalence_age_" + std::to_string(i));
    }
    return names;
}

std::string HipSIRScenarioAnalysis::probLabel(double p) {
    std::ostringstream os;
    os << "q" << p * 100.0;
    return os.str();
}

HipSIRScenarioAnalysis::HipSIRScenarioAnalysis(const HipPoissonLikelihoodObjective& objective, const std::vector<double>& timePoints, int n_age)
    : ctx_(objective.deviceContext()), times_(timePoints), n_age_(n_age), n_params_(static_cast<int>(objective.getParameterNames().size())) {
    if (timePoints.empty() || n_age < 1) throw InvalidParameterException("HipSIRScenarioAnalysis", "Time points are empty or n_age < 1.");
}

SIRScenarioResult HipSIRScenarioAnalysis::run(const double* samples, int n_samples, int burn_in, int thinning,
                                              const std::vector<SIRScenario>& scenarios, const std::vector<double>& probs) const {
    if (scenarios.empty()) throw InvalidParameterException("HipSIRScenarioAnalysis::run", "No scenarios given.");
    if (probs.empty()) throw InvalidParameterException("HipSIRScenarioAnalysis::run", "No probabilities given.");
    const int step = std::max(thinning, 1), first = std::max(burn_in, 0);
    std::vector<double> theta;
    for (int s = first; s < n_samples; s += step)
        theta.insert(theta.end(), samples + static_cast<size_t>(s) * n_params_, samples + static_cast<size_t>(s + 1) * n_params_);
    const int S = static_cast<int>(theta.size() / static_cast<size_t>(n_params_));
    if (S == 0) throw InvalidParameterException("HipSIRScenarioAnalysis::run", "No posterior samples left after burn-in and thinning.");
    const int K = static_cast<int>(scenarios.size()), T = static_cast<int>(times_.size()), n_probs = static_cast<int>(probs.size());
    const int W = 6 + 2 * n_age_;
    std::vector<sepaihrd_sir_event> table(static_cast<size_t>(K) * SEPAIHRD_SIR_MAX_EVENTS, sepaihrd_sir_event{0, 0, 0.0});
    std::vector<int32_t> counts(static_cast<size_t>(K));
    SIRScenarioResult r;
    for (int k = 0; k < K; ++k) {
        const auto& ev = scenarios[static_cast<size_t>(k)].events();
        counts[static_cast<size_t>(k)] = static_cast<int32_t>(ev.size());
        for (size_t e = 0; e < ev.size() && e < static_cast<size_t>(SEPAIHRD_SIR_MAX_EVENTS); ++e)
            table[static_cast<size_t>(k) * SEPAIHRD_SIR_MAX_EVENTS + e] = sepaihrd_sir_event{ev[e].time_index, ev[e].kind, ev[e].value};
        r.scenario_names.push_back(scenarios[static_cast<size_t>(k)].name());
    }
    r.metric_names = metricNames(n_age_);
    r.probs = probs;
    r.times = times_;
    r.n_age = n_age_;
    r.n_samples = S;
    r.quantiles.resize(static_cast<size_t>(K) * 3 * n_probs * T * (n_age_ + 1));
    r.metrics.resize(static_cast<size_t>(K) * S * W);
    r.metric_summary.resize(static_cast<size_t>(K) * W * (2 + n_probs));
    r.diff_quantiles.resize(static_cast<size_t>(K) * W * n_probs);
    r.status.resize(static_cast<size_t>(K) * S);
    r.n_valid.resize(static_cast<size_t>(K));
    const int rc = sepaihrd_sir_scenario_ensemble(ctx_, theta.data(), S, table.data(), counts.data(), K, probs.data(), n_probs, r.quantiles.data(),
                                                  r.metrics.data(), r.metric_summary.data(), r.diff_quantiles.data(), r.status.data(), nullptr,
                                                  nullptr, r.n_valid.data());
    if (rc == SEPAIHRD_E_INVALID_ARG) throw InvalidParameterException("HipSIRScenarioAnalysis::run", sepaihrd_sir_last_error(ctx_));
    if (rc != SEPAIHRD_OK) throw SimulationException("HipSIRScenarioAnalysis::run", sepaihrd_sir_last_error(ctx_));
    return r;
}

namespace {
std::ofstream open_csv(const std::string& path) {
    const std::filesystem::path p(path);
    if (p.has_parent_path()) std::filesystem::create_directories(p.parent_path());
    std::ofstream file(path);
    if (!file) throw ModelException("HipSIRScenarioAnalysis", "Cannot open '" + path + "' for writing.");
    return file;
}
}  // namespace

// numbers go through the stream's default format (six significant digits), as in HipPosteriorEnsemble's writers
void HipSIRScenarioAnalysis::writeScenarioComparison(const std::string& path, const SIRScenarioResult& r) {
    std::ofstream file = open_csv(path);
    const size_t W = r.metric_names.size(), np = r.probs.size();
    file << "scenario,metric,mean,std_dev";
    for (double p : r.probs) file << "," << probLabel(p);
    for (double p : r.probs) file << ",diff_" << probLabel(p);
    file << "\n";
    for (size_t k = 0; k < r.scenario_names.size(); ++k)
        for (size_t w = 0; w < W; ++w) {
            const double* s = r.metric_summary.data() + (k * W + w) * (2 + np);
            const double* d = r.diff_quantiles.data() + (k * W + w) * np;
            file << r.scenario_names[k] << "," << r.metric_names[w];
            for (size_t i = 0; i < 2 + np; ++i) file << "," << s[i];
            for (size_t i = 0; i < np; ++i) file << "," << d[i];
            file << "\n";
        }
}

void HipSIRScenarioAnalysis::writePosteriorBands(const std::string& path, const SIRScenarioResult& r) {
    static const char* const series[3] = {"incidence", "prevalence", "cumulative_infections"};
    std::ofstream file = open_csv(path);
    const size_t T = r.times.size(), np = r.probs.size(), cols = static_cast<size_t>(r.n_age) + 1;
    file << "scenario,series,time,age";
    for (double p : r.probs) file << "," << probLabel(p);
    file << "\n";
    for (size_t k = 0; k < r.scenario_names.size(); ++k)
        for (size_t ser = 0; ser < 3; ++ser)
            for (size_t t = 0; t < T; ++t)
                for (size_t a = 0; a < cols; ++a) {
                    file << r.scenario_names[k] << "," << series[ser] << "," << r.times[t] << ",";
                    if (a + 1 == cols) file << "total";
                    else file << a;
                    for (size_t p = 0; p < np; ++p) file << "," << r.quantiles[((((k * 3 + ser) * np + p) * T + t) * cols) + a];
                    file << "\n";
                }
}

}  // namespace epidemic
