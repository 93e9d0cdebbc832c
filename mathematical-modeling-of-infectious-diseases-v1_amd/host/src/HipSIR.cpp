// HipSIR.cpp -- AgeSIRModel, HipSIRParameterManager, HipPoissonLikelihoodObjective (see HipSIR.hpp).
#include "epidemic_hip/HipSIR.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <limits>

#include "sepaihrd_hip.h"

namespace epidemic {

// ---------------------------------------------------------------------------------------------------------------
// AgeSIRModel
// ---------------------------------------------------------------------------------------------------------------
std::shared_ptr<AgeSIRModel> AgeSIRModel::create(const Eigen::VectorXd& N, const Eigen::MatrixXd& C, const Eigen::VectorXd& gamma,
                                                 double q, double scale_C) {
    const int n = static_cast<int>(N.size());
    if (n <= 0) throw ModelException("AgeSIRModel::create", "Number of age classes must be positive.");
    if (C.rows() != n || C.cols() != n)
        throw ModelException("AgeSIRModel::create", "Contact matrix dimensions (" + std::to_string(C.rows()) + "x" + std::to_string(C.cols()) +
                                                        ") must match number of age classes (" + std::to_string(n) + ").");
    if (gamma.size() != n)
        throw ModelException("AgeSIRModel::create", "Gamma vector size (" + std::to_string(gamma.size()) +
                                                        ") must match number of age classes (" + std::to_string(n) + ").");
    bool negative = q < 0 || scale_C < 0;
    for (int i = 0; i < n; ++i) negative = negative || N[i] < 0 || gamma[i] < 0;
    if (negative)
        throw ModelException("AgeSIRModel::create",
                             "Initial rates (gamma), transmissibility (q), scaling (scale_C), or populations (N) cannot be negative.");
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (C(i, j) < 0) throw ModelException("AgeSIRModel::create", "Baseline contact matrix cannot contain negative values.");
    return std::shared_ptr<AgeSIRModel>(new AgeSIRModel(N, C, gamma, q, scale_C));
}

AgeSIRModel::AgeSIRModel(const Eigen::VectorXd& N, const Eigen::MatrixXd& C, const Eigen::VectorXd& gamma, double q, double scale_C)
    : n_(static_cast<int>(N.size())), N_(N), gamma_(gamma), C_baseline_(C), q_(q), scale_(scale_C), baseline_q_(q), baseline_scale_(scale_C) {}

Eigen::MatrixXd AgeSIRModel::getCurrentContactMatrix() const {
    Eigen::MatrixXd c(n_, n_);
    for (int i = 0; i < n_; ++i)
        for (int j = 0; j < n_; ++j) c(i, j) = scale_ * C_baseline_(i, j);
    return c;
}

// AgeSIRModel.cpp:106-139.  The row sum runs left to right over j, as oracle::sir_rhs and the device kernel form it.
void AgeSIRModel::computeDerivatives(const std::vector<double>& state, std::vector<double>& derivatives, double) {
    const size_t m = static_cast<size_t>(getStateSize());
    if (state.size() != m || derivatives.size() != m)
        throw InvalidParameterException("AgeSIRModel::computeDerivatives",
                                        "State or derivative vector size mismatch. Expected " + std::to_string(m) + ", got state=" +
                                            std::to_string(state.size()) + ", derivatives=" + std::to_string(derivatives.size()) + ".");
    const int n = n_;
    std::vector<double> ion(static_cast<size_t>(n), 0.0);
    for (int j = 0; j < n; ++j)
        if (N_[j] > 1e-9) ion[j] = state[n + j] / N_[j];
    for (int i = 0; i < n; ++i) {
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc += (C_baseline_(i, j) * scale_) * ion[j];
        const double lambda = std::max(q_ * acc, 0.0);
        const double S = state[i], I = state[n + i], R = state[2 * n + i];
        double dS = -lambda * S, dI = lambda * S - gamma_[i] * I, dR = gamma_[i] * I;
        if (S < 1e-9 && dS < 0) dS = 0.0;
        if (I < 1e-9 && dI < 0) dI = 0.0;
        if (R < 1e-9 && dR < 0) dR = 0.0;
        derivatives[i] = dS; derivatives[n + i] = dI; derivatives[2 * n + i] = dR;
    }
}

void AgeSIRModel::applyIntervention(const std::string& name, double, const Eigen::VectorXd& params) {
    if (name == "contact_reduction" || name == "social_distancing" || name == "lockdown") {
        if (params.size() != 1 || params[0] < 0.0)
            throw ModelException("AgeSIRModel::applyIntervention", "Intervention '" + name + "' requires exactly 1 non-negative parameter.");
        setContactScaleFactor(scale_ * params[0]);
    } else if (name == "mask_mandate" || name == "transmission_reduction") {
        if (params.size() != 1 || params[0] < 0.0 || params[0] > 1.0)
            throw ModelException("AgeSIRModel::applyIntervention", "Intervention '" + name + "' requires exactly 1 parameter in [0, 1].");
        setTransmissibility(q_ * (1.0 - params[0]));
    } else {
        throw ModelException("AgeSIRModel::applyIntervention", "Unknown intervention type: '" + name + "'.");
    }
}

void AgeSIRModel::reset() { q_ = baseline_q_; scale_ = baseline_scale_; }

std::vector<std::string> AgeSIRModel::getStateNames() const {
    std::vector<std::string> names;
    for (const char* c : {"S", "I", "R"})
        for (int i = 0; i < n_; ++i) names.push_back(c + std::to_string(i));
    return names;
}

void AgeSIRModel::setRecoveryRate(const Eigen::VectorXd& g) {
    if (g.size() != n_)
        throw InvalidParameterException("AgeSIRModel::setRecoveryRate", "Recovery rate vector size (" + std::to_string(g.size()) +
                                                                            ") must match the number of age classes (" + std::to_string(n_) + ").");
    for (int i = 0; i < n_; ++i)
        if (g[i] < 0) throw InvalidParameterException("AgeSIRModel::setRecoveryRate", "Recovery rates cannot be negative.");
    gamma_ = g;
}
void AgeSIRModel::setTransmissibility(double q) {
    if (q < 0) throw InvalidParameterException("AgeSIRModel::setTransmissibility", "Transmissibility (q) cannot be negative. Got: " + std::to_string(q));
    q_ = q;
}
void AgeSIRModel::setContactScaleFactor(double s) {
    if (s < 0)
        throw InvalidParameterException("AgeSIRModel::setContactScaleFactor", "Contact matrix scaling factor cannot be negative. Got: " + std::to_string(s));
    scale_ = s;
}

// ---------------------------------------------------------------------------------------------------------------
// HipSIRParameterManager
// ---------------------------------------------------------------------------------------------------------------
HipSIRParameterManager::HipSIRParameterManager(std::shared_ptr<AgeSIRModel> model, const std::vector<std::string>& params_to_calibrate,
                                               const std::map<std::string, double>& proposal_sigmas)
    : model_(std::move(model)), names_(params_to_calibrate), sigmas_(proposal_sigmas) {
    if (!model_) throw InvalidParameterException("SIRParameterManager", "Model pointer is null.");
    if (names_.empty()) throw InvalidParameterException("SIRParameterManager", "Parameter names list cannot be empty.");
    const int n = model_->getNumAgeClasses();
    for (size_t i = 0; i < names_.size(); ++i) {
        const std::string& name = names_[i];
        name_to_index_[name] = i;
        int field = SEPAIHRD_SIR_F_Q, index = 0;
        double default_sigma = 0.05;
        if (name == "q") {
        } else if (name == "scale_C_total") {
            field = SEPAIHRD_SIR_F_SCALE_C_TOTAL;
        } else if (name.rfind("gamma_", 0) == 0) {
            field = SEPAIHRD_SIR_F_GAMMA;
            default_sigma = 0.01;
            try {
                index = std::stoi(name.substr(6));
            } catch (const std::invalid_argument&) {
                throw ModelException("SIRParameterManager", "Could not parse age index from parameter name '" + name + "': Invalid argument");
            } catch (const std::out_of_range&) {
                throw ModelException("SIRParameterManager", "Could not parse age index from parameter name '" + name + "': Index out of range");
            }
            if (index < 0 || index >= n)
                throw ModelException("SIRParameterManager",
                                     "Invalid age index in parameter name '" + name + "'. Max index: " + std::to_string(n - 1));
        } else {
            throw ModelException("SIRParameterManager", "Parameter name '" + name + "' not recognized for AgeSIRModel calibration.");
        }
        field_.push_back(field);
        index_.push_back(index);
        if (sigmas_.find(name) == sigmas_.end()) sigmas_[name] = default_sigma;
    }
}

Eigen::VectorXd HipSIRParameterManager::getCurrentParameters() const {
    Eigen::VectorXd v(static_cast<Eigen::Index>(names_.size()));
    for (size_t i = 0; i < names_.size(); ++i)
        v[i] = field_[i] == SEPAIHRD_SIR_F_Q ? model_->getTransmissibility()
               : field_[i] == SEPAIHRD_SIR_F_SCALE_C_TOTAL ? model_->getContactScaleFactor()
                                                           : model_->getRecoveryRate()[index_[i]];
    return v;
}

Eigen::VectorXd HipSIRParameterManager::applyConstraints(const Eigen::VectorXd& p) const {
    if (static_cast<size_t>(p.size()) != names_.size())
        throw InvalidParameterException("SIRParameterManager::applyConstraints",
                                        "Parameter vector size mismatch: expected " + std::to_string(names_.size()) + ", got " + std::to_string(p.size()));
    Eigen::VectorXd c = p;
    for (size_t i = 0; i < names_.size(); ++i) c[i] = field_[i] == SEPAIHRD_SIR_F_Q ? std::max(1e-12, p[i]) : std::max(0.0, p[i]);
    return c;
}

void HipSIRParameterManager::updateModelParameters(const Eigen::VectorXd& p) {
    if (static_cast<size_t>(p.size()) != names_.size())
        throw InvalidParameterException("SIRParameterManager::updateModelParameters",
                                        "Parameter vector size mismatch: expected " + std::to_string(names_.size()) + ", got " + std::to_string(p.size()));
    const Eigen::VectorXd c = applyConstraints(p);
    Eigen::VectorXd gamma = model_->getRecoveryRate();
    bool gamma_changed = false;
    for (size_t i = 0; i < names_.size(); ++i) {
        if (field_[i] == SEPAIHRD_SIR_F_Q) model_->setTransmissibility(c[i]);
        else if (field_[i] == SEPAIHRD_SIR_F_SCALE_C_TOTAL) model_->setContactScaleFactor(c[i]);
        else if (gamma[index_[i]] != c[i]) { gamma[index_[i]] = c[i]; gamma_changed = true; }
    }
    if (gamma_changed) model_->setRecoveryRate(gamma);
}

int HipSIRParameterManager::getIndexForParam(const std::string& name) const {
    const auto it = name_to_index_.find(name);
    return it == name_to_index_.end() ? -1 : static_cast<int>(it->second);
}

double HipSIRParameterManager::getSigmaForParamIndex(int index) const {
    if (index < 0 || static_cast<size_t>(index) >= names_.size())
        throw std::out_of_range("[ParamManager] Index out of bounds in getSigmaForParamIndex: " + std::to_string(index));
    return sigmas_.at(names_[static_cast<size_t>(index)]);
}

double HipSIRParameterManager::getDefaultSigmaForParam(const std::string& name) const {
    const auto it = sigmas_.find(name);
    if (it == sigmas_.end())
        throw InvalidParameterException("SIRParameterManager::getDefaultSigmaForParam", "Default sigma not found for parameter: " + name);
    return it->second;
}

double HipSIRParameterManager::getLowerBoundForParamIndex(int idx) const {
    if (idx < 0 || static_cast<size_t>(idx) >= names_.size()) throw std::out_of_range("[ParamManager] Index out of bounds: " + std::to_string(idx));
    return field_[static_cast<size_t>(idx)] == SEPAIHRD_SIR_F_Q ? 1e-12 : 0.0;
}
double HipSIRParameterManager::getUpperBoundForParamIndex(int idx) const {
    if (idx < 0 || static_cast<size_t>(idx) >= names_.size()) throw std::out_of_range("[ParamManager] Index out of bounds: " + std::to_string(idx));
    return std::numeric_limits<double>::infinity();
}

// ---------------------------------------------------------------------------------------------------------------
// HipPoissonLikelihoodObjective
// ---------------------------------------------------------------------------------------------------------------
HipPoissonLikelihoodObjective::HipPoissonLikelihoodObjective(std::shared_ptr<AgeSIRModel> model, IParameterManager& parameterManager,
                                                             ISimulationCache& cache, const Eigen::MatrixXd& observed,
                                                             const std::vector<double>& timePoints, const Eigen::VectorXd& initialState,
                                                             std::shared_ptr<IOdeSolverStrategy> solver_strategy, double dt_hint,
                                                             double abs_error, double rel_error, int device, bool fma_arithmetic, int max_attempts)
    : pm_(parameterManager), cache_(cache), names_(parameterManager.getParameterNames()) {
    if (!model) throw InvalidParameterException("PoissonLikelihoodObjective", "Model pointer is null.");
    if (timePoints.empty()) throw InvalidParameterException("PoissonLikelihoodObjective", "Time points vector is empty.");
    if (static_cast<Eigen::Index>(timePoints.size()) != observed.rows())
        throw InvalidParameterException("PoissonLikelihoodObjective", "Time points size (" + std::to_string(timePoints.size()) +
                                                                          ") does not match observed data rows (" + std::to_string(observed.rows()) + ").");
    const int n = model->getNumAgeClasses();
    if (observed.cols() != n || initialState.size() != 3 * n)
        throw InvalidParameterException("PoissonLikelihoodObjective", "Observed data columns or initial state size do not match the model.");
    const int P = static_cast<int>(names_.size());
    // field map from the names (a manager of another type than HipSIRParameterManager may be given)
    const HipSIRParameterManager names_only(model, names_);
    std::vector<int32_t> field(names_only.fieldCodes().begin(), names_only.fieldCodes().end());
    std::vector<int32_t> index(names_only.fieldIndices().begin(), names_only.fieldIndices().end());
    std::vector<double> C(static_cast<size_t>(n) * n), obs(timePoints.size() * static_cast<size_t>(n));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) C[static_cast<size_t>(i) * n + j] = model->getBaselineContactMatrix()(i, j);
    for (size_t k = 0; k < timePoints.size(); ++k)
        for (int i = 0; i < n; ++i) obs[k * n + i] = observed(static_cast<Eigen::Index>(k), i);
    sepaihrd_sir_problem pb{};
    pb.abi_version = SEPAIHRD_ABI_VERSION;
    pb.n_age = n; pb.n_times = static_cast<int32_t>(timePoints.size()); pb.n_params = P;
    if (dynamic_cast<Dopri5SolverStrategy*>(solver_strategy.get())) pb.solver = SEPAIHRD_SOLVER_DOPRI5;
    else if (dynamic_cast<CashKarpSolverStrategy*>(solver_strategy.get())) pb.solver = SEPAIHRD_SOLVER_CASH_KARP54;
    else if (dynamic_cast<FehlbergSolverStrategy*>(solver_strategy.get())) pb.solver = SEPAIHRD_SOLVER_FEHLBERG78;
    else throw InvalidParameterException("HipPoissonLikelihoodObjective", "the solver strategy has no HIP kernel (Dopri5, Cash-Karp, Fehlberg 7(8))");
    pb.arith = fma_arithmetic ? SEPAIHRD_ARITH_FMA : SEPAIHRD_ARITH_STRICT;
    pb.times = timePoints.data(); pb.N = model->getPopulationSizes().data(); pb.C = C.data();
    pb.gamma = model->getRecoveryRate().data(); pb.initial_state = initialState.data(); pb.obs = obs.data();
    pb.param_field = field.data(); pb.param_index = index.data();
    pb.q = model->getTransmissibility(); pb.scale_C_total = model->getContactScaleFactor();
    pb.abs_err = abs_error; pb.rel_err = rel_error; pb.dt_hint = dt_hint;
    pb.max_attempts = max_attempts;
    char err[512] = {0};
    ctx_ = sepaihrd_sir_create(&pb, device, err, sizeof(err));
    if (!ctx_) throw ModelException("HipPoissonLikelihoodObjective", std::string("sepaihrd_sir_create failed: ") + err);
}

HipPoissonLikelihoodObjective::~HipPoissonLikelihoodObjective() { sepaihrd_sir_destroy(ctx_); }

void HipPoissonLikelihoodObjective::calculateBatch(const double* thetas, int B, double* out, int* status) const {
    std::vector<int32_t> st(static_cast<size_t>(std::max(B, 0)));
    const int rc = sepaihrd_sir_eval_batch(ctx_, thetas, B, out, st.data(), nullptr, nullptr, nullptr);
    if (rc != SEPAIHRD_OK)  // a failure of the launch itself, not of a chain
        throw SimulationException("HipPoissonLikelihoodObjective::calculateBatch", sepaihrd_sir_last_error(ctx_));
    if (status) std::copy(st.begin(), st.end(), status);
}

double HipPoissonLikelihoodObjective::calculate(const Eigen::VectorXd& parameters) const {
    if (const std::optional<double> hit = cache_.get(parameters)) return *hit;
    double value = -std::numeric_limits<double>::infinity();
    if (static_cast<size_t>(parameters.size()) != names_.size()) {  // updateModelParameters would throw; calculate() catches it
        std::cerr << "[ObjectiveFunc] Parameter Error: parameter vector size mismatch" << std::endl;
        return value;
    }
    try {
        calculateBatch(parameters.data(), 1, &value, nullptr);
    } catch (const std::exception& e) {
        std::cerr << "[ObjectiveFunc] Generic Error during simulation or likelihood calculation: " << e.what() << std::endl;
        return -std::numeric_limits<double>::infinity();
    }
    if (!std::isnan(value) && !std::isinf(value)) cache_.set(parameters, value);
    else value = -std::numeric_limits<double>::infinity();
    return value;
}

}  // namespace epidemic
