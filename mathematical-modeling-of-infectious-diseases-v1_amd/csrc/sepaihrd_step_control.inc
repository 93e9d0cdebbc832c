// csrc/sepaihrd_step_control.inc -- the arithmetic of the error norm and of the step-size controller, shared by every
// integrator of the library (sepaihrd_kernels.hip and sepaihrd_sir.hip; each compiled once per arithmetic mode).
// Included inside namespace sepaihrd { namespace { ... } } after sepaihrd_dev_common.inc (log_ctl) with
// SEPAIHRD_ARITH_FMA defined.

// |e| / s of the error norm.  strict: the IEEE division of the CPU build.  fma: Newton-refined
// reciprocal (4 instructions instead of 15); s > 0 is a tolerance scale, far from the overflow /
// underflow cases the IEEE sequence guards against.
__device__ __forceinline__ double quotient(double e, double s) {
#if SEPAIHRD_ARITH_FMA
    double r = __builtin_amdgcn_rcp(s);   // ~2^-26 relative
    r = fma(fma(-s, r, 1.0), r, r);       // one Newton step: ~2^-52
    return e * r;                         // a couple of ulp: the value only drives the step-size rule
#else
    return e / s;
#endif
}

// exp for the step-size controller: p = k ln2 + r, |r| <= ln2/2, degree-13 Taylor (remainder < 5e-18).
__device__ __forceinline__ double exp_ctl(double p) {
    constexpr double log2e = 1.44269504088896338700e+00;
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double kd = rint(p * log2e);
    double r = fma(-kd, ln2_hi, p);
    r = fma(-kd, ln2_lo, r);
    double q = 1.0 / 6227020800.0;
    q = fma(q, r, 1.0 / 479001600.0);
    q = fma(q, r, 1.0 / 39916800.0);
    q = fma(q, r, 1.0 / 3628800.0);
    q = fma(q, r, 1.0 / 362880.0);
    q = fma(q, r, 1.0 / 40320.0);
    q = fma(q, r, 1.0 / 5040.0);
    q = fma(q, r, 1.0 / 720.0);
    q = fma(q, r, 1.0 / 120.0);
    q = fma(q, r, 1.0 / 24.0);
    q = fma(q, r, 1.0 / 6.0);
    q = fma(q, r, 0.5);
    q = fma(q, r, 1.0);
    q = fma(q, r, 1.0);
    return ldexp(q, (int)kd);
}
// x^c for the controller's err^(-1/3), err^(-1/5): exp(c log x), a few ulp -- the reference calls
// std::pow (libm, not bit-pinned); the result only scales the next trial step.
__device__ __forceinline__ double pow_ctl(double x, double c) {
#if SEPAIHRD_ARITH_FMA
    // tolerance mode: the factor only scales the next TRIAL step, whose local error the controller checks
    // again; the hardware's single-precision log2 / exp2 (~1e-7 relative) are exact enough and cost five
    // instructions instead of fifty-seven.  err = +inf gives 0 (floored at 1/5 by the caller), like pow.
    const float l2 = __builtin_amdgcn_logf((float)x);
    return (double)__builtin_amdgcn_exp2f((float)c * l2);
#else
    return exp_ctl(c * log_ctl(x));
#endif
}
