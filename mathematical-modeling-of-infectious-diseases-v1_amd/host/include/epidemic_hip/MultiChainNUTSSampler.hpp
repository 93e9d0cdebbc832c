// host/include/epidemic_hip/MultiChainNUTSSampler.hpp
//
// The No-U-Turn sampler for many independent chains in lock step.  HipNUTSSampler runs ONE chain and pays a device
// launch for every gradient; here every chain is a resumable state machine that runs until it needs an evaluation it
// does not hold, posts a request (value + gradient at theta, or value only) and yields.  One tick gathers the requests
// of all live chains, evaluates them in ONE call of a batch objective (IBatchGradientObjective -- over the device:
// HipSEPAIHRDGradientObjectiveFunction::evaluateRows, one sepaihrd_fd_gradient_batch) and resumes every chain.
// No thread or fiber per chain: a chain is a program counter, a few vectors and the stack of half-built subtrees of the
// tree it is doubling (at most max_tree_depth frames).  Chains never wait for each other at iteration boundaries.
//
// Per chain the algorithm is HipNUTSSampler's: the same constants, the same order of draws from the chain's own
// std::mt19937(seed0 + c), the same gradient clip, slice variable, stopping rule, dual averaging and per-iteration
// constraint of the stored sample, the same treatment of a non-finite value at an iteration's start, and the same
// four-entry memory of recent evaluations (a request whose theta is bit-equal to one of them is served from it:
// gradient_calls counts the calls, rows_evaluated the rows that ran).  Two differences, both about what a chain shares:
//   * no SimulationCache: the value after each iteration is served from the chain's own recent evaluations or is a
//     value-only row -- the cache keys on theta quantised to 1e-8 and chains must not see each other's entries;
//   * an evaluation that reports an integration failure (status >= 2) stops THAT chain: its samples so far are kept,
//     the status and the iteration are recorded, the other chains run on.  (In HipNUTSSampler the exception leaves
//     optimize().)  Only a failed call -- the objective throws -- ends the whole run.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "epidemic_hip/Interfaces.hpp"

namespace epidemic {

struct NUTSChainResult {
    std::vector<std::vector<double>> samples;  // the constrained state after every iteration
    std::vector<double> sample_values, epsilon_trace;
    std::vector<int> depth_trace;  // tree depth reached; -1: the iteration repeated the previous sample (non-finite start)
    std::vector<double> best_parameters;
    double best_value = -std::numeric_limits<double>::infinity();
    long gradient_calls = 0;   // HipNUTSSampler::gradientCalls() of the same chain
    long rows_evaluated = 0;   // requests that were not served from the chain's memory: one row of one tick each
    int failure_status = 0;    // 0, or the status (>= 2) of the evaluation that stopped the chain
    int failure_iteration = -1;  // iteration (1-based) in which it stopped; 0: during the step-size search
};

struct MultiChainNUTSResult {
    std::vector<NUTSChainResult> chains;
    long ticks = 0;       // batched evaluations made
    long rows_total = 0;  // sum of the ticks' live rows (= sum of the chains' rows_evaluated)
    double meanRowsPerTick() const { return ticks > 0 ? static_cast<double>(rows_total) / static_cast<double>(ticks) : 0.0; }
};

class MultiChainNUTSSampler {
public:
    // HipNUTSSampler's keys: nuts_iterations, nuts_adaptation_window, nuts_delta_target, nuts_max_tree_depth, seed
    // (chain c draws from std::mt19937(seed + c))
    void configure(const std::map<std::string, double>& settings);
    // initial: C starting vectors; the manager supplies applyConstraints and the sigmas of the first step size
    MultiChainNUTSResult run(const std::vector<std::vector<double>>& initial, IBatchGradientObjective& objective,
                             const IParameterManager& parameterManager) const;

private:
    int num_iterations_ = 2000, adaptation_window_ = 500, max_tree_depth_ = 10;
    double delta_target_ = 0.8;
    uint32_t seed_ = 1;
};

}  // namespace epidemic
