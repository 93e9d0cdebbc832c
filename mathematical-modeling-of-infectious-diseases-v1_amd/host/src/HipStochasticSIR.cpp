// host/src/HipStochasticSIR.cpp -- HipStochasticSIRModel, the CPU twin of sepaihrd_stoch_sir_run and the flat helpers the
// Python tests drive (host_stoch_*).  The model, the stream and the sampler are csrc/sepaihrd_stoch.inc, the text the
// kernel compiles; this library is built with -ffp-contract=off like the kernel.
#include "epidemic_hip/HipStochasticSIR.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <stdexcept>

#include "sepaihrd_stoch.inc"

namespace epidemic {

namespace {
using sepaihrd_stoch::Group;
static_assert(sizeof(Group) == sizeof(sepaihrd_stoch_sir_group), "one group layout");
}  // namespace

int hostStochasticSIRRun(const sepaihrd_stoch_sir_config& cfg, const sepaihrd_stoch_sir_group* groups, double* stats, double* traj,
                         double* final_state, std::string* error) {
    char msg[256] = "";
    const int vrc = sepaihrd_stoch_sir_validate(&cfg, groups, msg, (int)sizeof(msg));
    if (vrc == SEPAIHRD_OK && !stats) std::snprintf(msg, sizeof(msg), "stoch_sir: stats must not be NULL");
    if (vrc == SEPAIHRD_OK && stats && cfg.keep > 0 && !traj) std::snprintf(msg, sizeof(msg), "stoch_sir: keep > 0 needs traj");
    if (msg[0]) {
        if (error) *error = msg;
        return SEPAIHRD_E_INVALID_ARG;
    }
    const int G = cfg.n_groups, R = cfg.n_replicates, keep = traj ? cfg.keep : 0;
    const int steps = (int)sepaihrd_stoch_sir_num_steps(cfg.t_start, cfg.t_end, cfg.h);
    // the time axis in chunks of whole steps, as on the device: one group's rows [3][chunk][R] at a time
    const std::uint64_t budget = cfg.max_workspace_bytes ? cfg.max_workspace_bytes : SEPAIHRD_STOCH_SIR_DEFAULT_WORKSPACE;
    std::uint64_t cs64 = budget / ((std::uint64_t)3 * R * sizeof(double));
    cs64 = std::max<std::uint64_t>(1, std::min<std::uint64_t>(cs64, (std::uint64_t)steps));
    const int cs = (int)cs64;
    std::vector<double> buf((size_t)3 * cs * R), S(R), I(R), Rc(R);
    for (int g = 0; g < G; ++g) {
        Group grp;
        grp.N = groups[g].N; grp.beta = groups[g].beta; grp.gamma = groups[g].gamma;
        grp.S0 = groups[g].S0; grp.I0 = groups[g].I0; grp.R0 = groups[g].R0;
        const double pR = sepaihrd_stoch::recovery_probability(grp.gamma, cfg.h);
        std::fill(S.begin(), S.end(), grp.S0);
        std::fill(I.begin(), I.end(), grp.I0);
        std::fill(Rc.begin(), Rc.end(), grp.R0);
        for (int step0 = 0; step0 < steps; step0 += cs) {
            const int n = std::min(cs, steps - step0);
#pragma omp parallel for schedule(static)
            for (int r = 0; r < R; ++r) {
                double s = S[r], i = I[r], rc = Rc[r];
                for (int k = 0; k < n; ++k) {
                    buf[((size_t)0 * n + k) * R + r] = s;
                    buf[((size_t)1 * n + k) * R + r] = i;
                    buf[((size_t)2 * n + k) * R + r] = rc;
                    if (step0 + k < steps - 1)
                        sepaihrd_stoch::sir_step(s, i, rc, grp, cfg.h, pR, cfg.seed, (uint32_t)g, (uint32_t)r, (uint32_t)(step0 + k));
                }
                S[r] = s; I[r] = i; Rc[r] = rc;
            }
            for (int c = 0; c < 3 && keep > 0; ++c)
                for (int k = 0; k < n; ++k)
                    for (int r = 0; r < keep; ++r)
                        traj[(((size_t)g * keep + r) * 3 + c) * (size_t)steps + (size_t)(step0 + k)] = buf[((size_t)c * n + k) * R + r];
#pragma omp parallel for schedule(dynamic, 4)
            for (int seg = 0; seg < 3 * n; ++seg) {
                double* x = buf.data() + (size_t)seg * R;
                std::sort(x, x + R);
                const int c = seg / n, k = seg % n;
                for (int stat = 0; stat < 4; ++stat)
                    stats[(((size_t)g * 4 + stat) * 3 + c) * (size_t)steps + (size_t)(step0 + k)] = sepaihrd_stoch::sorted_stat(x, R, stat);
            }
        }
        for (int r = 0; r < R && final_state; ++r) {
            double* f = final_state + ((size_t)g * R + r) * 3;
            f[0] = S[r]; f[1] = I[r]; f[2] = Rc[r];
        }
    }
    return SEPAIHRD_OK;
}

HipStochasticSIRModel::HipStochasticSIRModel(double N, double beta, double gamma, double S0, double I0, double R0, double t_start, double t_end,
                                             double h, unsigned int numSimulations, std::uint64_t seed, int device)
    : device_(device), steps_(0) {
    if (N <= 0 || beta < 0 || gamma < 0 || S0 < 0 || I0 < 0 || R0 < 0 || h <= 0 || t_end <= t_start || numSimulations == 0)
        throw std::invalid_argument("Invalid parameters for StochasticSIRModel constructor.");
    if (std::abs((S0 + I0 + R0) - N) > 1e-6 * N) throw std::invalid_argument("Initial compartments S0+I0+R0 must sum to N.");
    group_.N = N; group_.beta = beta; group_.gamma = gamma; group_.S0 = S0; group_.I0 = I0; group_.R0 = R0;
    config_.abi_version = SEPAIHRD_ABI_VERSION;
    config_.n_groups = 1;
    config_.n_replicates = numSimulations > (unsigned)SEPAIHRD_STOCH_SIR_MAX_REPLICATES ? SEPAIHRD_STOCH_SIR_MAX_REPLICATES + 1 : (int)numSimulations;
    config_.keep = (int)std::min(numSimulations, MAX_WRITTEN_SIMS);
    config_.t_start = t_start; config_.t_end = t_end; config_.h = h;
    config_.seed = seed;
    config_.max_workspace_bytes = 0;
    char msg[256] = "";
    if (sepaihrd_stoch_sir_validate(&config_, &group_, msg, (int)sizeof(msg)) != SEPAIHRD_OK) throw std::invalid_argument(msg);
    steps_ = (int)sepaihrd_stoch_sir_num_steps(t_start, t_end, h);
}

void HipStochasticSIRModel::setKeptTrajectories(unsigned int count) {
    config_.keep = (int)std::min<unsigned>(count, (unsigned)config_.n_replicates);
}

void HipStochasticSIRModel::runSimulations() {
    stats_.assign((size_t)12 * steps_, 0.0);
    traj_.assign((size_t)config_.keep * 3 * steps_, 0.0);
    double* traj = config_.keep > 0 ? traj_.data() : nullptr;
    if (device_ == HOST_TWIN) {
        std::string error;
        if (hostStochasticSIRRun(config_, &group_, stats_.data(), traj, nullptr, &error) != SEPAIHRD_OK) throw std::runtime_error(error);
    } else {
        char msg[512] = "";
        const int rc = sepaihrd_stoch_sir_run(device_, &config_, &group_, stats_.data(), traj, nullptr, nullptr, msg, (int)sizeof(msg));
        if (rc != SEPAIHRD_OK) throw std::runtime_error("sepaihrd_stoch_sir_run failed (" + std::to_string(rc) + "): " + msg);
    }
    ran_ = true;
}

std::vector<std::vector<std::vector<double>>> HipStochasticSIRModel::getStatistics() const {
    if (!ran_) return {};
    std::vector<std::vector<std::vector<double>>> out(4, std::vector<std::vector<double>>(3));
    for (int stat = 0; stat < 4; ++stat)
        for (int c = 0; c < 3; ++c) {
            const double* p = stats_.data() + ((size_t)stat * 3 + c) * steps_;
            out[stat][c].assign(p, p + steps_);
        }
    return out;
}

std::vector<std::vector<std::vector<double>>> HipStochasticSIRModel::getResults() const {
    if (!ran_) return {};
    std::vector<std::vector<std::vector<double>>> out((size_t)config_.keep, std::vector<std::vector<double>>(3));
    for (int sim = 0; sim < config_.keep; ++sim)
        for (int c = 0; c < 3; ++c) {
            const double* p = traj_.data() + ((size_t)sim * 3 + c) * steps_;
            out[sim][c].assign(p, p + steps_);
        }
    return out;
}

void HipStochasticSIRModel::writeCsv(const std::string& dir) const {
    if (!ran_) throw std::runtime_error("HipStochasticSIRModel::writeCsv: runSimulations() has not run");
    const std::string base = dir.empty() ? std::string() : dir + "/";
    if (config_.n_replicates > 1) {
        std::ofstream f(base + "stochastic_sir_stats.csv");
        if (!f.is_open()) throw std::runtime_error("Could not open file for writing: " + base + "stochastic_sir_stats.csv");
        f << "t,S_mean,S_median,S_p05,S_p95,I_mean,I_median,I_p05,I_p95,R_mean,R_median,R_p05,R_p95\n";
        for (int step = 0; step < steps_; ++step) {
            const double t = config_.t_start + step * config_.h;
            f << t;
            for (int c = 0; c < 3; ++c)
                for (int stat = 0; stat < 4; ++stat) f << "," << stats_[((size_t)stat * 3 + c) * steps_ + step];
            f << "\n";
        }
    }
    const int written = std::min<int>(config_.keep, (int)MAX_WRITTEN_SIMS);
    for (int sim = 0; sim < written; ++sim) {
        const std::string path = base + "stochastic_sir_sim_" + std::to_string(sim) + ".csv";
        std::ofstream f(path);
        if (!f.is_open()) throw std::runtime_error("Could not open file for writing: " + path);
        f << "t,S,I,R\n";
        for (int step = 0; step < steps_; ++step) {
            const double t = config_.t_start + step * config_.h;
            f << t;
            for (int c = 0; c < 3; ++c) f << "," << traj_[((size_t)sim * 3 + c) * steps_ + step];
            f << "\n";
        }
    }
}

}  // namespace epidemic

// ---- flat helpers for the Python tests (no device unless said) ----
extern "C" {

void host_stoch_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
    const sepaihrd_stoch::Philox b = sepaihrd_stoch::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = b.w[i];
}

double host_stoch_uniform(uint32_t lo, uint32_t hi) { return sepaihrd_stoch::uniform_open(lo, hi); }

void host_stoch_probabilities(double beta, double I, double h, double N, double gamma, double* pI, double* pR) {
    *pI = sepaihrd_stoch::infection_probability(beta, I, h, N);
    *pR = sepaihrd_stoch::recovery_probability(gamma, h);
}

int32_t host_stoch_binomial_at(uint64_t seed, uint32_t group, uint32_t replicate, uint32_t step, uint32_t transition, int32_t n, double p) {
    sepaihrd_stoch::Coord c;
    c.seed = seed; c.group = group; c.replicate = replicate; c.step = step; c.transition = transition;
    return sepaihrd_stoch::binomial(c, n, p);
}

// the twin of sepaihrd_stoch_sir_binomial_device: out[i] at (seed, group 0, replicate i, step 0, infection)
void host_stoch_binomial_probe(uint64_t seed, const int32_t* n, const double* p, int count, int32_t* out) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < count; ++i) out[i] = host_stoch_binomial_at(seed, 0, (uint32_t)i, 0, sepaihrd_stoch::TRANSITION_INFECTION, n[i], p[i]);
}

int host_stoch_sir_run(const sepaihrd_stoch_sir_config* config, const sepaihrd_stoch_sir_group* groups, double* stats, double* traj,
                       double* final_state, char* err, int errlen) {
    if (!config) return SEPAIHRD_E_INVALID_ARG;
    std::string error;
    const int rc = epidemic::hostStochasticSIRRun(*config, groups, stats, traj, final_state, &error);
    if (rc != SEPAIHRD_OK && err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", error.c_str());
    return rc;
}

// HipStochasticSIRModel end to end: construct, run, write the CSVs into `dir`, hand back the statistics [4][3][steps] and
// the kept trajectories [keep][3][steps] (either may be NULL).  0 ok; 1 std::invalid_argument; 2 any other exception; the
// message in err.
int host_stoch_sir_model(double N, double beta, double gamma, double S0, double I0, double R0, double t_start, double t_end, double h,
                         unsigned int numSimulations, uint64_t seed, int device, const char* dir, double* stats, double* results,
                         int* n_steps, char* err, int errlen) {
    auto fail = [&](const char* what, int code) {
        if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", what);
        return code;
    };
    try {
        epidemic::HipStochasticSIRModel model(N, beta, gamma, S0, I0, R0, t_start, t_end, h, numSimulations, seed, device);
        if (n_steps) *n_steps = model.numSteps();
        if (!dir && !stats && !results) return 0;  // the constructor alone
        model.runSimulations();
        if (dir) model.writeCsv(dir);
        const auto st = model.getStatistics();
        for (size_t a = 0; stats && a < st.size(); ++a)
            for (size_t c = 0; c < 3; ++c) std::copy(st[a][c].begin(), st[a][c].end(), stats + (a * 3 + c) * (size_t)model.numSteps());
        const auto rs = model.getResults();
        for (size_t s = 0; results && s < rs.size(); ++s)
            for (size_t c = 0; c < 3; ++c) std::copy(rs[s][c].begin(), rs[s][c].end(), results + (s * 3 + c) * (size_t)model.numSteps());
        return 0;
    } catch (const std::invalid_argument& e) {
        return fail(e.what(), 1);
    } catch (const std::exception& e) {
        return fail(e.what(), 2);
    }
}

}  // extern "C"
