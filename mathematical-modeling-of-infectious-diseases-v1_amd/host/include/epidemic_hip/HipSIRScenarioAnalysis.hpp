// HipSIRScenarioAnalysis.hpp -- posterior ensemble and intervention scenarios of the age-structured SIR model on the device
// (sepaihrd_sir_scenario_ensemble of include/sepaihrd_hip.h): every posterior sample under every named scenario in one
// integrator launch, per-scenario quantile bands of incidence / prevalence / cumulative infections, a metric table with its
// summaries and the paired differences against the first scenario.
//
// A scenario is built from the reference's own intervention names, one addIntervention(time, name, params) per entry with
// the rules and error kinds of InterventionCallback::validateParameters / addIntervention
// (src/sir_age_structured/InterventionCallback.cpp:20-75) and the two rules of AgeSIRModel::applyIntervention
// (src/sir_age_structured/AgeSIRModel.cpp:141-173):
//   "contact_reduction" / "social_distancing" / "lockdown"   scale_C_total <- scale_C_total * params[0], params[0] >= 0
//   "mask_mandate" / "transmission_reduction"                q <- q * (1 - params[0]), 0 <= params[0] <= 1
// Interventions act on the output grid: `time` must be one of the objective's time points.  (The reference's demo main
// schedules off the grid and shifts its second segment by one row; neither is reproduced -- INTEGRATION.md.)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "HipSIR.hpp"

namespace epidemic {

struct SIRInterventionEvent {
    int32_t time_index, kind;  // kind: 0 contact (SEPAIHRD_SIR_EV_CONTACT), 1 transmission (SEPAIHRD_SIR_EV_TRANSMISSION)
    double value;
};

class SIRScenario {
public:
    // timePoints: the output grid the event times are looked up in
    SIRScenario(std::string name, const std::vector<double>& timePoints);
    // InvalidParameterException: negative time, a time that is no grid point, a parameter count other than 1, a value out of
    // its kind's range, more than 8 events; ModelException: an intervention name the model does not know.  Entries may be
    // added in any order: events() is sorted by time, entries of one time in the order they were added (the multimap of
    // the reference's schedule).
    void addIntervention(double time, const std::string& name, const Eigen::VectorXd& params);
    // the callback-level check alone (unknown names pass here, as in the reference, and are refused by addIntervention)
    static void validateParameters(const std::string& name, const Eigen::VectorXd& params);
    // 0 / 1 for the names above, -1 for any other
    static int kindOf(const std::string& name);
    const std::string& name() const { return name_; }
    const std::vector<SIRInterventionEvent>& events() const { return events_; }
private:
    std::string name_;
    std::vector<double> times_;
    std::vector<SIRInterventionEvent> events_;
};

struct SIRScenarioResult {
    std::vector<std::string> scenario_names, metric_names;
    std::vector<double> probs, times;
    int n_age = 0, n_samples = 0;
    std::vector<double> quantiles;       // [K][3][n_probs][T][n_age + 1]
    std::vector<double> metrics;         // [K][S][W]
    std::vector<double> metric_summary;  // [K][W][2 + n_probs]
    std::vector<double> diff_quantiles;  // [K][W][n_probs]
    std::vector<int32_t> status;         // [K][S]
    std::vector<int32_t> n_valid;        // [K]
};

class HipSIRScenarioAnalysis {
public:
    // the objective lends its device context; timePoints and n_age are the ones it was built with
    HipSIRScenarioAnalysis(const HipPoissonLikelihoodObjective& objective, const std::vector<double>& timePoints, int n_age);
    // samples [n_samples][P] row-major; rows burn_in, burn_in + thinning, ... are analysed (thinning < 1 counts as 1).
    // Throws InvalidParameterException when nothing is left, SimulationException when the call itself fails; a failed sample
    // is a NaN metric row and is skipped by the summaries.
    SIRScenarioResult run(const double* samples, int n_samples, int burn_in, int thinning, const std::vector<SIRScenario>& scenarios,
                          const std::vector<double>& probs) const;
    // sir_scenario_comparison.csv: scenario,metric,mean,std_dev,q<p>...,diff_q<p>...  -- one row per scenario x metric
    static void writeScenarioComparison(const std::string& path, const SIRScenarioResult& r);
    // sir_posterior_bands.csv: scenario,series,time,age,q<p>...  -- age "total" for the age sum
    static void writePosteriorBands(const std::string& path, const SIRScenarioResult& r);
    static std::vector<std::string> metricNames(int n_age);
    static std::string probLabel(double p);  // 0.025 -> "q2.5", 0.5 -> "q50"
private:
    sepaihrd_sir_ctx* ctx_;
    std::vector<double> times_;
    int n_age_, n_params_;
};

}  // namespace epidemic
