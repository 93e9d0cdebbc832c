// host/include/epidemic_hip/HipStochasticSIR.hpp
//
// The reference's StochasticSIRModel (include/base/SIR_stochastic.hpp) above sepaihrd_stoch_sir_run: numSimulations
// replicates of a chain-binomial SIR, one lane each on the device, and the per-step mean, median, 5 % and 95 % point across
// them.  Same constructor arguments and conditions, plus what the reference cannot have: a seed (its generator is seeded
// from the clock; this build's stream is a function of the seed and of each variate's coordinates, csrc/sepaihrd_stoch.inc)
// and a device.  The CPU twin of the kernel (the same model text, OpenMP over replicates) is hostStochasticSIRRun below and
// the backend of a model constructed with device = HOST_TWIN.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "sepaihrd_hip.h"

namespace epidemic {

// sepaihrd_stoch_sir_run on the host: same arguments apart from the device, same outputs bit for bit.  Returns
// SEPAIHRD_OK or SEPAIHRD_E_INVALID_ARG with the validator's message.
int hostStochasticSIRRun(const sepaihrd_stoch_sir_config& config, const sepaihrd_stoch_sir_group* groups, double* stats, double* traj,
                         double* final_state, std::string* error = nullptr);

class HipStochasticSIRModel {
public:
    static constexpr int HOST_TWIN = -2;               // `device`: run the CPU twin instead of a device
    static constexpr unsigned MAX_WRITTEN_SIMS = 100;  // the reference writes (here: also keeps) the first 100 trajectories

    // throws std::invalid_argument under the reference's conditions (SIR_stochastic.cpp:29-34, 46-49) with its messages,
    // and for what this build adds (sepaihrd_stoch_sir_validate) with the validator's
    HipStochasticSIRModel(double N, double beta, double gamma, double S0, double I0, double R0, double t_start, double t_end, double h,
                          unsigned int numSimulations, std::uint64_t seed = 0, int device = -1);

    // trajectories kept for getResults() / writeCsv(): the first `count` replicates (default min(numSimulations, 100); the
    // reference keeps all of them, which at device scale is gigabytes).  Call before runSimulations().
    void setKeptTrajectories(unsigned int count);
    void setMaxWorkspaceBytes(std::uint64_t bytes) { config_.max_workspace_bytes = bytes; }

    void runSimulations();  // throws std::runtime_error when the run fails (no device, allocation)

    int numSteps() const { return steps_; }
    std::vector<std::vector<std::vector<double>>> getStatistics() const;  // [4: mean, median, p05, p95][3: S, I, R][steps]
    std::vector<std::vector<std::vector<double>>> getResults() const;     // [kept simulation][3][steps]

    // The reference's two kinds of file, into `dir`: stochastic_sir_stats.csv when numSimulations > 1, and
    // stochastic_sir_sim_<i>.csv for the first min(kept, 100) replicates; its headers, t = t_start + step h, numbers in the
    // stream's default formatting.
    void writeCsv(const std::string& dir) const;

private:
    sepaihrd_stoch_sir_config config_{};
    sepaihrd_stoch_sir_group group_{};
    int device_, steps_;
    bool ran_ = false;
    std::vector<double> stats_, traj_;
};

}  // namespace epidemic
