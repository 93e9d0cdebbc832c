// HipSIR.hpp -- the age-structured SIR calibration path of the reference behind this repository's Interfaces.hpp, with the
// likelihood evaluated on the device through the sepaihrd_sir_* block of include/sepaihrd_hip.h.  Restatements of
// (paths under the reference tree):
//   AgeSIRModel                  include/sir_age_structured/AgeSIRModel.hpp, src/sir_age_structured/AgeSIRModel.cpp
//   SIRParameterManager          src/sir_age_structured/parameters/SIRParameterManager.cpp
//   PoissonLikelihoodObjective   src/sir_age_structured/objectives/PoissonLikelihoodObjective.cpp
// The calibration flow on top of them runs on the device too: MultiChainMetropolisHastings::optimizeChainsOnDevice has an
// overload for HipPoissonLikelihoodObjective (sepaihrd_sir_mh_create: chains, streams, accept test and adaptation resident
// in HBM) and HipModelCalibrator a constructor for this pair (HipModelCalibrator.hpp); deviceContext() is what they borrow.
// Mid-run interventions are outside the objective: AgeSIRModel::applyIntervention only changes the host object's values.
// Schedules of them run on the device for every posterior sample through HipSIRScenarioAnalysis.hpp.
#pragma once
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "Interfaces.hpp"

struct sepaihrd_sir_ctx;

namespace epidemic {

class AgeSIRModel : public IEpidemicModel {
public:
    // AgeSIRModel::create (:10-38): throws ModelException on a size mismatch or a negative N / gamma / q / scale / C entry
    static std::shared_ptr<AgeSIRModel> create(const Eigen::VectorXd& N, const Eigen::MatrixXd& C, const Eigen::VectorXd& gamma,
                                               double q, double scale_C = 1.0);
    void computeDerivatives(const std::vector<double>& state, std::vector<double>& derivatives, double time) override;
    void applyIntervention(const std::string& name, double time, const Eigen::VectorXd& params) override;
    void reset() override;
    int getStateSize() const override { return 3 * n_; }
    std::vector<std::string> getStateNames() const override;
    int getNumAgeClasses() const override { return n_; }
    // setters validate as the reference's do (InvalidParameterException on a negative value or a size mismatch)
    void setRecoveryRate(const Eigen::VectorXd& new_gamma);
    void setTransmissibility(double new_q);
    void setContactScaleFactor(double new_scale);
    const Eigen::VectorXd& getPopulationSizes() const { return N_; }
    const Eigen::MatrixXd& getBaselineContactMatrix() const { return C_baseline_; }
    Eigen::MatrixXd getCurrentContactMatrix() const;
    const Eigen::VectorXd& getRecoveryRate() const { return gamma_; }
    double getTransmissibility() const { return q_; }
    double getContactScaleFactor() const { return scale_; }
private:
    AgeSIRModel(const Eigen::VectorXd& N, const Eigen::MatrixXd& C, const Eigen::VectorXd& gamma, double q, double scale_C);
    int n_;
    Eigen::VectorXd N_, gamma_;
    Eigen::MatrixXd C_baseline_;
    double q_, scale_, baseline_q_, baseline_scale_;
};

class HipSIRParameterManager : public IParameterManager {
public:
    // names: "q", "scale_C_total", "gamma_<i>"; errors as SIRParameterManager.cpp:10-63; default sigmas 0.05 / 0.05 / 0.01
    HipSIRParameterManager(std::shared_ptr<AgeSIRModel> model, const std::vector<std::string>& params_to_calibrate,
                           const std::map<std::string, double>& proposal_sigmas = {});
    Eigen::VectorXd getCurrentParameters() const override;
    void updateModelParameters(const Eigen::VectorXd& parameters) override;
    const std::vector<std::string>& getParameterNames() const override { return names_; }
    size_t getParameterCount() const override { return names_.size(); }
    double getSigmaForParamIndex(int index) const override;
    Eigen::VectorXd applyConstraints(const Eigen::VectorXd& parameters) const override;
    int getIndexForParam(const std::string& name) const override;
    // The reference's SIR manager has no bounds; this repository's IParameterManager asks for them: the constraint floors
    // (1e-12 for q, 0 otherwise) and +infinity.
    double getLowerBoundForParamIndex(int idx) const override;
    double getUpperBoundForParamIndex(int idx) const override;
    double getDefaultSigmaForParam(const std::string& name) const;
    const AgeSIRModel& model() const { return *model_; }
    // field code (SEPAIHRD_SIR_F_*) and age index of every name
    const std::vector<int>& fieldCodes() const { return field_; }
    const std::vector<int>& fieldIndices() const { return index_; }
private:
    std::shared_ptr<AgeSIRModel> model_;
    std::vector<std::string> names_;
    std::map<std::string, double> sigmas_;
    std::unordered_map<std::string, size_t> name_to_index_;
    std::vector<int> field_, index_;
};

class HipPoissonLikelihoodObjective : public IObjectiveFunction, public IBatchObjectiveFunction {
public:
    // observed: [timePoints.size()][n] (CalibrationData::getNewConfirmedCases); the solver is selected by the dynamic type of
    // solver_strategy, as in the SEPAIHRD adapter.  Throws InvalidParameterException for a null model, empty time points or a
    // row mismatch (:31-42), ModelException when the device context cannot be created (no CPU fallback).  max_attempts is the
    // build-side step budget per evaluation (<= 0: 1000000); the reference has none.
    HipPoissonLikelihoodObjective(std::shared_ptr<AgeSIRModel> model, IParameterManager& parameterManager, ISimulationCache& cache,
                                  const Eigen::MatrixXd& observed, const std::vector<double>& timePoints,
                                  const Eigen::VectorXd& initialState, std::shared_ptr<IOdeSolverStrategy> solver_strategy,
                                  double dt_hint = 1.0, double abs_error = 1e-6, double rel_error = 1e-6, int device = -1,
                                  bool fma_arithmetic = false, int max_attempts = 0);
    ~HipPoissonLikelihoodObjective() override;
    HipPoissonLikelihoodObjective(const HipPoissonLikelihoodObjective&) = delete;
    HipPoissonLikelihoodObjective& operator=(const HipPoissonLikelihoodObjective&) = delete;
    // cache lookup, one-chain launch, finite values cached, -infinity never (:46-111); never throws for a failed evaluation
    double calculate(const Eigen::VectorXd& parameters) const override;
    const std::vector<std::string>& getParameterNames() const override { return names_; }
    // B evaluations in one launch, no cache; out[b] = -infinity and status[b] = 1 / 2 / 3 for a failed chain, nothing thrown
    void calculateBatch(const double* thetas, int B, double* out, int* status = nullptr) const override;
    // the context behind this objective, for the callers that keep work on the device
    // (MultiChainMetropolisHastings::optimizeChainsOnDevice)
    sepaihrd_sir_ctx* deviceContext() const { return ctx_; }
private:
    IParameterManager& pm_;
    ISimulationCache& cache_;
    std::vector<std::string> names_;
    sepaihrd_sir_ctx* ctx_ = nullptr;
};

}  // namespace epidemic
