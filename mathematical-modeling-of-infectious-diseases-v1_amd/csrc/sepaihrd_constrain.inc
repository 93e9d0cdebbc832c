// csrc/sepaihrd_constrain.inc -- the parameter constraint rule (SEPAIHRDParameterManager::applyConstraints) as ONE text for host
// and device: the integrators' prologues (through csrc/sepaihrd_dev_common.inc), the propose kernels of the sampler, the
// ensemble's Rt and metric kernels, the decode kernel of the stochastic model, sepaihrd_apply_constraints and the host library's
// parameter manager all compile these two functions.  A sampler that proposes under one rule while the evaluator constrains
// under another is a silent wrong posterior; with one text they cannot part.
// Contraction: not every includer is built with -ffp-contract=off (csrc/sepaihrd_capi.cpp, the fma integrators).  The only
// multiply-add in the rule is `y += 2.0 * width`; a product with 2 is exact, so the fused and the unfused form agree bit for bit.
#pragma once

#if defined(__HIPCC__)
#define SEP_CONSTRAIN_FN __host__ __device__ __forceinline__
#else
#define SEP_CONSTRAIN_FN inline
#endif

// SEPAIHRDParameterManager.cpp:302-313 / :326-343
SEP_CONSTRAIN_FN double reflect_bound(double value, double minb, double maxb) {
    if (minb >= maxb) return minb;
    const double width = maxb - minb;
    double y = fmod(value - minb, 2.0 * width);
    if (y < 0) y += 2.0 * width;
    if (y <= width) return minb + y;
    return maxb - (y - width);
}
SEP_CONSTRAIN_FN double constrain(double v, double lo, double hi, int has_bounds, int mode) {
    if (has_bounds) {
        if (lo > hi) { const double t = lo; lo = hi; hi = t; }
        if (mode == 0) {
            const double m = (v < lo) ? lo : v;  // std::max(v, lo)
            return (hi < m) ? hi : m;            // std::min(m, hi)
        }
        return reflect_bound(v, lo, hi);
    }
    if (mode == 0) return (0.0 < v) ? v : 0.0;  // std::max(0.0, v)
    return fabs(v);
}

// Where DevProblem is visible (csrc/sepaihrd_device.h included first): slot `slot` of the model's scalars, entry (field, age) of
// its per-age vectors -- the constrained theta entry where the slot is calibrated (src >= 0), else the base value.
#if defined(SEPAIHRD_HAVE_DEV_PROBLEM)
__device__ __forceinline__ double constrained_theta(const DevProblem& pb, const double* th, int p) {
    return constrain(th[p], pb.lower[p], pb.upper[p], pb.has_bounds[p], pb.constraint_mode);
}
__device__ __forceinline__ double slot_scalar(const DevProblem& pb, const double* th, int slot) {
    const int src = pb.src_scalar[slot];
    return src >= 0 ? constrained_theta(pb, th, src) : pb.base_scalar[slot];
}
__device__ __forceinline__ double slot_vec(const DevProblem& pb, const double* th, int field, int age) {
    const int src = pb.src_vec[field * pb.lpc + age];
    return src >= 0 ? constrained_theta(pb, th, src) : pb.base_vec[field * pb.lpc + age];
}
#endif
