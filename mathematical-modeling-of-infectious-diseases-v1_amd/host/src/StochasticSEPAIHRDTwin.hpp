// host/src/StochasticSEPAIHRDTwin.hpp -- what the two CPU twins of the stochastic SEPAIHRD model (hostStochasticSEPAIHRD,
// hostParticleLoglik) and their two adapters do the same way.  Internal to the host library.
#pragma once
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <memory>
#include <string>
#include <utility>

#include "epidemic_hip/HipStochasticSEPAIHRD.hpp"
#include "sepaihrd_hip.h"
#include "sepaihrd_stoch_sepaihrd.inc"

namespace epidemic {
namespace stoch_twin {

namespace epi = sepaihrd_stoch_epi;

// what a twin derives from the fixed data before anything else
struct Plan {
    int T_pos = 0;          // output times >= 0
    int runup_offset = 0;   // the times increase: the output times >= 0 are the last T_pos
    epi::RowLayout L{0, 0, 0};
    size_t W = 0;           // doubles of a model-values row
    size_t row_doubles = 0; // doubles of one state: [11][n_age]
};
inline Plan plan(const StochasticSEPAIHRDFixedData& pb) {
    Plan p;
    for (int k = 0; k < pb.n_times && pb.times; ++k) p.T_pos += pb.times[k] >= 0.0;
    p.runup_offset = pb.n_times - p.T_pos;
    p.L = epi::RowLayout{pb.n_age, pb.n_beta, pb.n_kappa};
    p.W = (size_t)p.L.width();
    p.row_doubles = (size_t)epi::NUM_COMP * (size_t)pb.n_age;
    return p;
}

inline bool fixed_data_missing(const StochasticSEPAIHRDFixedData& pb) {
    return !pb.N || !pb.M || !pb.kappa_end_times || pb.n_kappa < 1 || pb.n_beta < 0 || (pb.n_beta > 0 && !pb.beta_end_times);
}
constexpr const char* FIXED_DATA_TEXT = "the fixed data need N, M and the schedule end times (n_kappa >= 1)";

// The verdict on a twin's arguments: the validator's (vrc with its text in msg) where it refused, else the first of `checks`
// (failed, text) that failed, as "<who>: <text>".  The message goes to *error.
inline int verdict(const char* who, int vrc, char (&msg)[256], std::initializer_list<std::pair<bool, const char*>> checks, std::string* error) {
    for (const auto& c : checks)
        if (vrc == SEPAIHRD_OK && c.first) {
            std::snprintf(msg, sizeof(msg), "%s: %s", who, c.second);
            vrc = SEPAIHRD_E_INVALID_ARG;
        }
    if (vrc != SEPAIHRD_OK && error) *error = msg;
    return vrc;
}

// what an invalid position leaves in an optional output: NaN in out[offset .. offset + count)
inline void nan_fill(double* out, size_t offset, size_t count) {
    if (out) std::fill(out + offset, out + offset + count, std::numeric_limits<double>::quiet_NaN());
}

// the objective whose device context an adapter runs its calls on, with the initial-state rule set; `who` names the adapter
inline std::unique_ptr<HipSEPAIHRDObjectiveFunction> make_objective(const char* who, HipSEPAIHRDParameterManager& pm, SimulationCache& cache,
                                                                    const CalibrationData& data, const std::vector<double>& time_points,
                                                                    const Eigen::VectorXd& initial_state,
                                                                    std::shared_ptr<IOdeSolverStrategy> solver_strategy, int device,
                                                                    int initial_state_mode) {
    auto objective = std::make_unique<HipSEPAIHRDObjectiveFunction>(pm, cache, data, time_points, initial_state, std::move(solver_strategy), 1.0e-6,
                                                                    1.0e-6, device, false);
    if (sepaihrd_set_initial_state_mode(objective->deviceContext(), initial_state_mode) != SEPAIHRD_OK)
        throw ModelException(who, "sepaihrd_set_initial_state_mode failed");
    return objective;
}

}  // namespace stoch_twin
}  // namespace epidemic
