// host/include/epidemic_hip/HipChainDiagnostics.hpp
//
// Convergence diagnostics of many chains on the device (sepaihrd_chain_diagnostics): per parameter, and for the chains'
// values when given, the rank-normalised split R-hat and the bulk / tail effective sample sizes of Vehtari et al. (2021)
// as the R package `posterior` computes them.  The reference runs one chain and reports none of this; here it is what
// says whether the pooled samples of thousands of lock-step chains are one stationary distribution.
#pragma once
#include <string>
#include <vector>

#include "epidemic_hip/HipSEPAIHRD.hpp"

namespace epidemic {

// ChainDiagnosticsTable: include/epidemic_hip/HipSEPAIHRD.hpp (MultiChainMetropolisHastings::diagnostics() returns one)
class HipChainDiagnostics {
public:
    static const std::vector<std::string>& columns();  // the 7 column names, in order
    // chains[c][n] = draw n of chain c (every chain the same length N >= 4); values[c][n] the chain's value at that draw,
    // or an empty vector.  Runs on the objective's device context.
    static ChainDiagnosticsTable compute(HipSEPAIHRDObjectiveFunction& objective, const std::vector<std::vector<Eigen::VectorXd>>& chains,
                                         const std::vector<std::vector<double>>& values = {});
    static ChainDiagnosticsTable compute(sepaihrd_ctx* ctx, const std::vector<std::vector<Eigen::VectorXd>>& chains,
                                         const std::vector<std::vector<double>>& values = {});
    // parameter_posteriors/posterior_diagnostics.csv: "parameter,mean,...,r_hat", numbers as %.8e, one row per name and a
    // final log_likelihood row when the table has one more row than there are names
    static void writeCsv(const std::string& path, const std::vector<std::string>& names, const ChainDiagnosticsTable& table);
};

}  // namespace epidemic
