// host/src/MultiChainNUTSSampler.cpp -- lock-step scheduler over resumable No-U-Turn chains (see the header).
#include "epidemic_hip/MultiChainNUTSSampler.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <random>

namespace epidemic {
namespace {

using Vec = std::vector<double>;
constexpr double kSliceSlack = 1000.0;    // a leaf further than this below the slice ends the tree
constexpr double kGradientCap = 1000.0;   // Euclidean norm the gradient is scaled down to
constexpr size_t kMemory = 4;             // recent evaluations a chain keeps

double inner(const Vec& a, const Vec& b) {
    double acc = 0.0;
    for (size_t i = 0; i < a.size(); ++i) acc += a[i] * b[i];
    return acc;
}

void capNorm(Vec& g) {
    double sq = 0.0;
    for (double x : g) sq += x * x;
    const double norm = std::sqrt(sq);
    if (norm > kGradientCap)
        for (double& x : g) x *= kGradientCap / norm;
}

bool sameBits(const Vec& a, const Vec& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0; }

// a (sub)tree of the doubling: its two ends, the candidate drawn from it, and the acceptance statistics
struct Span {
    Vec lo_q, lo_p, hi_q, hi_p, pick;
    int level = 0, inside = 0, visits = 0;
    bool open = false;
    double accept_sum = 0.0;
};

bool turnsBack(const Vec& lo_q, const Vec& hi_q, const Vec& lo_p, const Vec& hi_p) {
    double at_lo = 0.0, at_hi = 0.0;
    for (size_t i = 0; i < lo_q.size(); ++i) {
        const double d = hi_q[i] - lo_q[i];
        at_lo += d * lo_p[i];
        at_hi += d * hi_p[i];
    }
    return !(at_lo >= 0 && at_hi >= 0);
}

struct Settings {
    int iterations, window, max_depth;
    double target;
};

class Chain {
public:
    Chain(const Vec& start, uint32_t seed, const Settings& cfg, const IParameterManager& pm)
        : cfg_(cfg), pm_(pm), P_(start.size()), rng_(seed), q_(start) {}

    // the request the chain is parked on (valid while !finished())
    const Vec& requestPoint() const { return ask_q_; }
    bool requestWantsGradient() const { return ask_grad_; }
    bool finished() const { return pc_ == Pc::Done; }
    NUTSChainResult& result() { return out_; }

    void deliver(double value, const double* grad, int status) {
        ++out_.rows_evaluated;
        if (status >= 2) {
            out_.failure_status = status;
            out_.failure_iteration = searching_ ? 0 : iter_;
            pc_ = Pc::Done;
            return;
        }
        if (ask_grad_) {
            memory_[memory_next_ % kMemory] = {ask_q_, Vec(grad, grad + P_), value, serial_++};
            ++memory_next_;
        } else {
            value_only_ = value;
            value_only_ready_ = true;
        }
    }

    // runs until the next request is posted or the chain is done
    void advance() {
        for (;;) {
            switch (pc_) {
                case Pc::SearchBegin: {
                    searching_ = true;
                    double mean_sigma = 0.0;
                    for (size_t i = 0; i < P_; ++i) mean_sigma += pm_.getSigmaForParamIndex(static_cast<int>(i));
                    mean_sigma /= static_cast<double>(P_);
                    step_ = std::max(1e-6, std::min(mean_sigma * 0.1, 0.1));
                    std::normal_distribution<> gauss(0.0, 1.0);
                    p0_.resize(P_);
                    for (double& x : p0_) x = gauss(rng_);
                    pc_ = Pc::SearchStart;
                    break;
                }
                case Pc::SearchStart: {
                    if (!gradientAt(q_)) return;
                    if (!std::isfinite(got_value_)) { pc_ = Pc::SearchEnd; break; }
                    energy0_ = got_value_ - 0.5 * inner(p0_, p0_);
                    beginLeaf(q_, p0_, step_, Pc::SearchFirst);
                    break;
                }
                case Pc::SearchFirst: {
                    accept_ = std::exp(std::min(0.0, leaf_value_ - 0.5 * inner(leaf_p_, leaf_p_) - energy0_));
                    round_ = 0;
                    pc_ = Pc::SearchAdjust;
                    break;
                }
                case Pc::SearchAdjust: {
                    if (round_ >= 5) { pc_ = Pc::SearchEnd; break; }
                    if (accept_ < 0.1 && step_ > 1e-8) step_ *= 0.5;
                    else if (accept_ > 0.9 && step_ < 1.0) step_ *= 1.5;
                    else { pc_ = Pc::SearchEnd; break; }
                    beginLeaf(q_, p0_, step_, Pc::SearchJudge);
                    break;
                }
                case Pc::SearchJudge: {
                    ++round_;
                    if (!std::isfinite(leaf_value_)) step_ *= 0.5;
                    else accept_ = std::exp(std::min(0.0, leaf_value_ - 0.5 * inner(leaf_p_, leaf_p_) - energy0_));
                    pc_ = Pc::SearchAdjust;
                    break;
                }
                case Pc::SearchEnd: {
                    searching_ = false;
                    shrink_to_ = std::log(10.0 * step_);
                    step_avg_ = step_;
                    drift_ = 0.0;
                    iter_ = 1;
                    pc_ = Pc::IterationBegin;
                    break;
                }
                case Pc::IterationBegin: {
                    if (iter_ > cfg_.iterations) { pc_ = Pc::Done; return; }
                    std::normal_distribution<> gauss(0.0, 1.0);
                    p0_.resize(P_);
                    for (double& x : p0_) x = gauss(rng_);
                    pc_ = Pc::IterationStart;
                    break;
                }
                case Pc::IterationStart: {
                    if (!gradientAt(q_)) return;
                    if (!std::isfinite(got_value_)) {  // nothing to move from: the previous sample again, if there is one
                        if (!out_.samples.empty()) {
                            out_.samples.push_back(out_.samples.back());
                            out_.sample_values.push_back(out_.sample_values.back());
                            out_.epsilon_trace.push_back(step_);
                            out_.depth_trace.push_back(-1);
                        }
                        ++iter_;
                        pc_ = Pc::IterationBegin;
                        break;
                    }
                    energy0_ = got_value_ - 0.5 * inner(p0_, p0_);
                    slice_ = energy0_ - std::exponential_distribution<>(1.0)(rng_);
                    lo_q_ = hi_q_ = next_q_ = q_;
                    lo_p_ = hi_p_ = p0_;
                    depth_ = 0; inside_ = 1; visits_ = 0; accept_sum_ = 0.0; growing_ = true;
                    pc_ = Pc::Doubling;
                    break;
                }
                case Pc::Doubling: {
                    if (!(growing_ && depth_ < cfg_.max_depth)) { pc_ = Pc::IterationEnd; break; }
                    dir_ = (std::uniform_int_distribution<>(0, 1)(rng_) * 2) - 1;
                    frames_.clear();
                    if (dir_ < 0) beginLeaf(lo_q_, lo_p_, dir_ * step_, Pc::LeafDone);
                    else beginLeaf(hi_q_, hi_p_, dir_ * step_, Pc::LeafDone);
                    break;
                }
                case Pc::LeafDone: {
                    Span leaf;
                    const double energy = leaf_value_ - 0.5 * inner(leaf_p_, leaf_p_);
                    leaf.level = 0;
                    leaf.inside = slice_ <= energy ? 1 : 0;
                    leaf.open = slice_ < energy + kSliceSlack;
                    leaf.lo_q = leaf.hi_q = leaf.pick = leaf_q_;
                    leaf.lo_p = leaf.hi_p = leaf_p_;
                    leaf.accept_sum = std::min(1.0, std::exp(energy - energy0_));
                    leaf.visits = 1;
                    if (absorb(std::move(leaf))) pc_ = Pc::SubtreeDone;
                    else beginLeaf(leaf_q_, leaf_p_, dir_ * step_, Pc::LeafDone);  // onwards from the leaf just made
                    break;
                }
                case Pc::SubtreeDone: {
                    const Span& t = built_;
                    if (dir_ < 0) { lo_q_ = t.lo_q; lo_p_ = t.lo_p; }
                    else { hi_q_ = t.hi_q; hi_p_ = t.hi_p; }
                    if (t.open && !turnsBack(lo_q_, hi_q_, lo_p_, hi_p_)) {
                        const double take = static_cast<double>(t.inside) / static_cast<double>(inside_ + t.inside);
                        if (std::uniform_real_distribution<>(0.0, 1.0)(rng_) < take) next_q_ = t.pick;
                        inside_ += t.inside;
                        accept_sum_ += t.accept_sum;
                        visits_ += t.visits;
                        ++depth_;
                    } else {
                        growing_ = false;
                    }
                    pc_ = Pc::Doubling;
                    break;
                }
                case Pc::IterationEnd: {
                    q_ = next_q_;
                    if (iter_ <= cfg_.window) {  // dual averaging of the step size
                        const double mean_accept = visits_ > 0 ? accept_sum_ / visits_ : 0.0;
                        const double w = 1.0 / (iter_ + 10.0);
                        drift_ = (1.0 - w) * drift_ + w * (cfg_.target - mean_accept);
                        const double log_step = shrink_to_ - (std::sqrt(iter_) / 0.05) * drift_;
                        step_ = std::exp(log_step);
                        const double fade = std::pow(iter_, -0.75);
                        step_avg_ = std::exp(fade * log_step + (1.0 - fade) * std::log(step_avg_));
                    } else {
                        step_ = step_avg_;
                    }
                    kept_ = constrained(q_);
                    pc_ = Pc::IterationValue;
                    break;
                }
                case Pc::IterationValue: {
                    if (!valueAt(kept_)) return;
                    out_.samples.push_back(kept_);
                    out_.sample_values.push_back(got_value_);
                    if (got_value_ > out_.best_value) {
                        out_.best_value = got_value_;
                        out_.best_parameters = kept_;
                    }
                    out_.epsilon_trace.push_back(step_);
                    out_.depth_trace.push_back(depth_);
                    ++iter_;
                    pc_ = Pc::IterationBegin;
                    break;
                }
                // one leapfrog step and the value at its end: three gradient calls, the last two at the same point
                case Pc::LeafFirstHalf: {
                    if (!gradientAt(leaf_q_)) return;
                    capNorm(got_grad_);
                    for (size_t i = 0; i < P_; ++i) leaf_p_[i] += 0.5 * leaf_step_ * got_grad_[i];
                    for (size_t i = 0; i < P_; ++i) leaf_q_[i] += leaf_step_ * leaf_p_[i];
                    leaf_q_ = constrained(leaf_q_);
                    pc_ = Pc::LeafSecondHalf;
                    break;
                }
                case Pc::LeafSecondHalf: {
                    if (!gradientAt(leaf_q_)) return;
                    capNorm(got_grad_);
                    for (size_t i = 0; i < P_; ++i) leaf_p_[i] += 0.5 * leaf_step_ * got_grad_[i];
                    pc_ = Pc::LeafValue;
                    break;
                }
                case Pc::LeafValue: {
                    if (!gradientAt(leaf_q_)) return;
                    leaf_value_ = got_value_;
                    pc_ = leaf_then_;
                    break;
                }
                case Pc::Done:
                    return;
            }
        }
    }

private:
    enum class Pc {
        SearchBegin, SearchStart, SearchFirst, SearchAdjust, SearchJudge, SearchEnd,
        IterationBegin, IterationStart, Doubling, LeafDone, SubtreeDone, IterationEnd, IterationValue,
        LeafFirstHalf, LeafSecondHalf, LeafValue, Done
    };
    struct Remembered {
        Vec q, grad;
        double value = 0.0;
        long serial = -1;  // -1: empty slot
    };

    void beginLeaf(const Vec& q, const Vec& p, double step, Pc then) {
        leaf_q_ = q;
        leaf_p_ = p;
        leaf_step_ = step;
        leaf_then_ = then;
        pc_ = Pc::LeafFirstHalf;
    }

    Vec constrained(const Vec& q) const {
        Eigen::VectorXd v(static_cast<Eigen::Index>(P_));
        for (size_t i = 0; i < P_; ++i) v[static_cast<Eigen::Index>(i)] = q[i];
        const Eigen::VectorXd c = pm_.applyConstraints(v);
        Vec r(P_);
        for (size_t i = 0; i < P_; ++i) r[i] = c[static_cast<Eigen::Index>(i)];
        return r;
    }

    const Remembered* recall(const Vec& q) const {
        const Remembered* hit = nullptr;  // the newest match, as a front-to-back search of a newest-first list finds
        for (const Remembered& m : memory_)
            if (m.serial >= 0 && sameBits(m.q, q) && (!hit || m.serial > hit->serial)) hit = &m;
        return hit;
    }

    // value and gradient at q into got_value_ / got_grad_; false: a request was posted, call again after deliver().
    // The state that calls it has no side effect before the call, so re-entering it is harmless.
    bool gradientAt(const Vec& q) {
        if (!parked_) ++out_.gradient_calls;
        parked_ = false;
        if (const Remembered* m = recall(q)) {
            got_value_ = m->value;
            got_grad_ = m->grad;
            return true;
        }
        ask_q_ = q;
        ask_grad_ = true;
        parked_ = true;
        return false;
    }

    bool valueAt(const Vec& q) {
        parked_ = false;
        if (value_only_ready_) {
            value_only_ready_ = false;
            got_value_ = value_only_;
            return true;
        }
        if (const Remembered* m = recall(q)) {
            got_value_ = m->value;
            return true;
        }
        ask_q_ = q;
        ask_grad_ = false;
        parked_ = true;
        return false;
    }

    // A finished span of the subtree being built (target level depth_) meets the frames of its unfinished ancestors: the
    // frames hold the left halves that wait for their right halves, levels falling towards the top.  Returns true when the
    // subtree is complete (built_), false when another leaf is needed.
    bool absorb(Span t) {
        for (;;) {
            if (t.level == depth_) { built_ = std::move(t); return true; }
            if (!frames_.empty() && frames_.back().level == t.level) {  // t is the right half of the top frame
                Span left = std::move(frames_.back());
                frames_.pop_back();
                Span both;
                both.level = t.level + 1;
                if (dir_ < 0) { both.lo_q = t.lo_q; both.lo_p = t.lo_p; both.hi_q = left.hi_q; both.hi_p = left.hi_p; }
                else { both.lo_q = left.lo_q; both.lo_p = left.lo_p; both.hi_q = t.hi_q; both.hi_p = t.hi_p; }
                if (t.open) {
                    both.inside = left.inside + t.inside;
                    const double take = both.inside > 0 ? static_cast<double>(t.inside) / static_cast<double>(both.inside) : 0.0;
                    both.pick = std::uniform_real_distribution<>(0.0, 1.0)(rng_) < take ? t.pick : left.pick;
                    both.accept_sum = left.accept_sum + t.accept_sum;
                    both.visits = left.visits + t.visits;
                    both.open = left.open && !turnsBack(both.lo_q, both.hi_q, both.lo_p, both.hi_p);
                } else {  // a closed right half contributes its ends only
                    both.pick = left.pick;
                    both.inside = left.inside;
                    both.accept_sum = left.accept_sum;
                    both.visits = left.visits;
                    both.open = false;
                }
                t = std::move(both);
            } else if (!t.open) {  // a closed left half IS its parent: no right half is built
                ++t.level;
            } else {
                frames_.push_back(std::move(t));
                return false;
            }
        }
    }

    const Settings cfg_;
    const IParameterManager& pm_;
    const size_t P_;
    std::mt19937 rng_;
    Pc pc_ = Pc::SearchBegin, leaf_then_ = Pc::Done;
    NUTSChainResult out_;
    // request / evaluation memory
    Vec ask_q_, got_grad_;
    bool ask_grad_ = false, parked_ = false, value_only_ready_ = false, searching_ = true;
    double got_value_ = 0.0, value_only_ = 0.0;
    std::array<Remembered, kMemory> memory_;
    size_t memory_next_ = 0;
    long serial_ = 0;
    // step-size search and adaptation
    double step_ = 0.0, step_avg_ = 0.0, drift_ = 0.0, shrink_to_ = 0.0, accept_ = 0.0, energy0_ = 0.0, slice_ = 0.0;
    int round_ = 0, iter_ = 0;
    // the iteration's trajectory
    Vec q_, p0_, lo_q_, lo_p_, hi_q_, hi_p_, next_q_, kept_;
    int depth_ = 0, inside_ = 1, visits_ = 0, dir_ = 1;
    double accept_sum_ = 0.0;
    bool growing_ = true;
    std::vector<Span> frames_;
    Span built_;
    // the leaf in progress
    Vec leaf_q_, leaf_p_;
    double leaf_step_ = 0.0, leaf_value_ = 0.0;
};

}  // namespace

void MultiChainNUTSSampler::configure(const std::map<std::string, double>& settings) {
    auto value = [&](const char* key, double fallback) {
        const auto it = settings.find(key);
        return it == settings.end() ? fallback : it->second;
    };
    num_iterations_ = static_cast<int>(value("nuts_iterations", 2000.0));
    adaptation_window_ = static_cast<int>(value("nuts_adaptation_window", 500.0));
    delta_target_ = value("nuts_delta_target", 0.8);
    max_tree_depth_ = static_cast<int>(value("nuts_max_tree_depth", 10.0));
    seed_ = static_cast<uint32_t>(value("seed", 1.0));
}

MultiChainNUTSResult MultiChainNUTSSampler::run(const std::vector<std::vector<double>>& initial, IBatchGradientObjective& objective,
                                                const IParameterManager& parameterManager) const {
    MultiChainNUTSResult result;
    const size_t C = initial.size();
    if (C == 0) return result;
    const size_t P = initial.front().size();
    for (const Vec& v : initial)
        if (v.size() != P || P == 0) throw InvalidParameterException("MultiChainNUTSSampler", "starting vectors must share one non-zero length");
    const Settings cfg{num_iterations_, adaptation_window_, max_tree_depth_, delta_target_};
    std::vector<Chain> chains;
    chains.reserve(C);
    for (size_t c = 0; c < C; ++c) chains.emplace_back(initial[c], seed_ + static_cast<uint32_t>(c), cfg, parameterManager);

    std::vector<size_t> live(C), parked;
    for (size_t c = 0; c < C; ++c) live[c] = c;
    Vec rows, values, gradients;
    std::vector<uint8_t> want;
    std::vector<int32_t> status;
    while (!live.empty()) {
        parked.clear();
        for (size_t c : live) {
            chains[c].advance();
            if (!chains[c].finished()) parked.push_back(c);
        }
        live.swap(parked);
        if (live.empty()) break;
        const size_t B = live.size();
        rows.resize(B * P); values.resize(B); gradients.resize(B * P); want.resize(B); status.assign(B, 0);
        for (size_t b = 0; b < B; ++b) {
            const Chain& ch = chains[live[b]];
            std::memcpy(&rows[b * P], ch.requestPoint().data(), P * sizeof(double));
            want[b] = ch.requestWantsGradient() ? 1 : 0;
        }
        objective.evaluateRows(rows.data(), want.data(), static_cast<int>(B), static_cast<int>(P), values.data(), gradients.data(),
                               status.data());
        ++result.ticks;
        result.rows_total += static_cast<long>(B);
        for (size_t b = 0; b < B; ++b) chains[live[b]].deliver(values[b], &gradients[b * P], status[b]);
    }
    result.chains.reserve(C);
    for (Chain& ch : chains) result.chains.push_back(std::move(ch.result()));
    return result;
}

}  // namespace epidemic
