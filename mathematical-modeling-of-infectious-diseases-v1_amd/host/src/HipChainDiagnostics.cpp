// host/src/HipChainDiagnostics.cpp -- see include/epidemic_hip/HipChainDiagnostics.hpp
#include "epidemic_hip/HipChainDiagnostics.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>

#include "sepaihrd_hip.h"

namespace epidemic {

const std::vector<std::string>& HipChainDiagnostics::columns() {
    static const std::vector<std::string> c = {"mean", "sd", "mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "r_hat"};
    return c;
}

ChainDiagnosticsTable HipChainDiagnostics::compute(HipSEPAIHRDObjectiveFunction& objective, const std::vector<std::vector<Eigen::VectorXd>>& chains,
                                                   const std::vector<std::vector<double>>& values) {
    return compute(objective.deviceContext(), chains, values);
}

ChainDiagnosticsTable HipChainDiagnostics::compute(sepaihrd_ctx* ctx, const std::vector<std::vector<Eigen::VectorXd>>& chains,
                                                   const std::vector<std::vector<double>>& values) {
    const int C = static_cast<int>(chains.size());
    if (C < 1 || chains[0].empty()) throw InvalidParameterException("HipChainDiagnostics", "no draws");
    const int N = static_cast<int>(chains[0].size());
    const int P = static_cast<int>(chains[0][0].size());
    const bool with_values = !values.empty();
    if (with_values && static_cast<int>(values.size()) != C) throw InvalidParameterException("HipChainDiagnostics", "one value series per chain");
    std::vector<double> s(static_cast<size_t>(C) * N * P), v(with_values ? static_cast<size_t>(C) * N : 0);
    for (int c = 0; c < C; ++c) {
        if (static_cast<int>(chains[static_cast<size_t>(c)].size()) != N || (with_values && static_cast<int>(values[static_cast<size_t>(c)].size()) != N))
            throw InvalidParameterException("HipChainDiagnostics", "every chain needs the same number of draws (and values)");
        for (int n = 0; n < N; ++n) {
            const Eigen::VectorXd& x = chains[static_cast<size_t>(c)][static_cast<size_t>(n)];
            if (static_cast<int>(x.size()) != P) throw InvalidParameterException("HipChainDiagnostics", "draws of different lengths");
            for (int p = 0; p < P; ++p) s[(static_cast<size_t>(c) * N + n) * P + p] = x[p];
            if (with_values) v[static_cast<size_t>(c) * N + n] = values[static_cast<size_t>(c)][static_cast<size_t>(n)];
        }
    }
    ChainDiagnosticsTable t;
    t.rows = P + (with_values ? 1 : 0);
    t.values.resize(static_cast<size_t>(t.rows) * SEPAIHRD_DIAG_COLUMNS);
    t.max_lag.resize(static_cast<size_t>(t.rows) * 4);
    if (sepaihrd_chain_diagnostics(ctx, s.data(), with_values ? v.data() : nullptr, C, N, P, t.values.data(), t.max_lag.data()) != SEPAIHRD_OK)
        throw ModelException("HipChainDiagnostics", std::string("sepaihrd_chain_diagnostics: ") + sepaihrd_last_error(ctx));
    return t;
}

void HipChainDiagnostics::writeCsv(const std::string& path, const std::vector<std::string>& names, const ChainDiagnosticsTable& table) {
    const int P = static_cast<int>(names.size());
    if (table.rows != P && table.rows != P + 1)
        throw InvalidParameterException("HipChainDiagnostics", "writeCsv: the table has neither one row per name nor one more");
    std::ofstream file(path);
    if (!file.is_open()) throw ModelException("HipChainDiagnostics", "cannot open " + path);
    file << "parameter";
    for (const std::string& c : columns()) file << "," << c;
    file << "\n";
    char buf[32];
    for (int r = 0; r < table.rows; ++r) {
        file << (r < P ? names[static_cast<size_t>(r)] : std::string("log_likelihood"));
        for (int k = 0; k < SEPAIHRD_DIAG_COLUMNS; ++k) {
            const double v = table.at(r, k);
            if (std::isnan(v)) std::snprintf(buf, sizeof(buf), "nan");  // as Python's "%.8e" % nan, whatever the sign bit
            else std::snprintf(buf, sizeof(buf), "%.8e", v);
            file << "," << buf;
        }
        file << "\n";
    }
}

}  // namespace epidemic
