// csrc/sepaihrd_rk_stages.inc -- the stages of one attempt of the three controlled steppers for a state of N values per
// lane and any right-hand side: rhs_call(x_in, k_out).  Included inside namespace sepaihrd { namespace { ... } } after
// sepaihrd_dev_common.inc (the tableaus dp::, ck::, f78::).
//   SOLVER 0  runge_kutta_dopri5::do_step_impl (FSAL: k1 is the derivative at x on entry, k7 the one at xnew on exit)
//   SOLVER 1  runge_kutta_cash_karp54 through generic_rk (k1 evaluated here, at every attempt)
//   SOLVER 2  runge_kutta_fehlberg78 through generic_rk (k1 evaluated here, at every attempt)
// Every stage input is 1.0 x + (a_i1 dt) k1 + ... summed left to right with the zero entries left out, the factors
// dt * coefficient formed first: the operation sequence of sepaihrd_eval_kernel's written-out bodies (sepaihrd_kernels.hip),
// which keep their own copy because their register allocation and code placement are tuned per lane count.  Under
// -ffp-contract=off that is the CPU build's arithmetic; under -ffp-contract=fast the compiler contracts as it sees fit.
template <int SOLVER, int N, class RHS>
__device__ __forceinline__ void rk_attempt(const double cur, const double (&x)[N], double (&k1)[N], double (&k7)[N],
                                           double (&xnew)[N], double (&xerr)[N], RHS&& rhs_call) {
    double xt[N];
    if constexpr (SOLVER == 0) {
        double k2[N], k3[N], k4[N], k5[N], k6[N];
        { const double f1 = cur * dp::b21;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c];
          rhs_call(xt, k2); }
        { const double f1 = cur * dp::b31, f2 = cur * dp::b32;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c];
          rhs_call(xt, k3); }
        { const double f1 = cur * dp::b41, f2 = cur * dp::b42, f3 = cur * dp::b43;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c];
          rhs_call(xt, k4); }
        { const double f1 = cur * dp::b51, f2 = cur * dp::b52, f3 = cur * dp::b53, f4 = cur * dp::b54;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c];
          rhs_call(xt, k5); }
        { const double f1 = cur * dp::b61, f2 = cur * dp::b62, f3 = cur * dp::b63, f4 = cur * dp::b64, f5 = cur * dp::b65;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c] + f5 * k5[c];
          rhs_call(xt, k6); }
        { const double f1 = cur * dp::c1, f3 = cur * dp::c3, f4 = cur * dp::c4, f5 = cur * dp::c5, f6 = cur * dp::c6;
          SEP_UNROLL for (int c = 0; c < N; ++c) xnew[c] = x[c] + f1 * k1[c] + f3 * k3[c] + f4 * k4[c] + f5 * k5[c] + f6 * k6[c];
          rhs_call(xnew, k7); }
        { const double e1 = cur * dp::dc1, e3 = cur * dp::dc3, e4 = cur * dp::dc4, e5 = cur * dp::dc5, e6 = cur * dp::dc6,
                       e7 = cur * dp::dc7;
          SEP_UNROLL for (int c = 0; c < N; ++c)
              xerr[c] = e1 * k1[c] + e3 * k3[c] + e4 * k4[c] + e5 * k5[c] + e6 * k6[c] + e7 * k7[c]; }
    } else if constexpr (SOLVER == 1) {
        double k2[N], k3[N], k4[N], k5[N], k6[N];
        rhs_call(x, k1);
        { const double f1 = ck::a21 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c];
          rhs_call(xt, k2); }
        { const double f1 = ck::a31 * cur, f2 = ck::a32 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c];
          rhs_call(xt, k3); }
        { const double f1 = ck::a41 * cur, f2 = ck::a42 * cur, f3 = ck::a43 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c];
          rhs_call(xt, k4); }
        { const double f1 = ck::a51 * cur, f2 = ck::a52 * cur, f3 = ck::a53 * cur, f4 = ck::a54 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c];
          rhs_call(xt, k5); }
        { const double f1 = ck::a61 * cur, f2 = ck::a62 * cur, f3 = ck::a63 * cur, f4 = ck::a64 * cur, f5 = ck::a65 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c] + f5 * k5[c];
          rhs_call(xt, k6); }
        // zero tableau entries (b2 = b5 = 0, db2 = 0) contribute an exact +0.0 in the reference
        { const double f1 = ck::b1 * cur, f3 = ck::b3 * cur, f4 = ck::b4 * cur, f6 = ck::b6 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xnew[c] = x[c] + f1 * k1[c] + f3 * k3[c] + f4 * k4[c] + f6 * k6[c]; }
        { const double e1 = ck::db1 * cur, e3 = ck::db3 * cur, e4 = ck::db4 * cur, e5 = ck::db5 * cur, e6 = ck::db6 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xerr[c] = e1 * k1[c] + e3 * k3[c] + e4 * k4[c] + e5 * k5[c] + e6 * k6[c]; }
    } else {
        // k2 and k3 die at stages 3 and 5, k11 goes straight into the error sum, the solution is summed after the last stage
        double k2[N], k3[N], k4[N], k5[N], k6[N], k8[N], k9[N], k10[N], k11[N], k12[N], k13[N];
        rhs_call(x, k1);
        { const double f1 = f78::a2_1 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c];
          rhs_call(xt, k2); }
        { const double f1 = f78::a3_1 * cur, f2 = f78::a3_2 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c];
          rhs_call(xt, k3); }
        { const double f1 = f78::a4_1 * cur, f3 = f78::a4_3 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f3 * k3[c];
          rhs_call(xt, k4); }
        { const double f1 = f78::a5_1 * cur, f3 = f78::a5_3 * cur, f4 = f78::a5_4 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f3 * k3[c] + f4 * k4[c];
          rhs_call(xt, k5); }
        { const double f1 = f78::a6_1 * cur, f4 = f78::a6_4 * cur, f5 = f78::a6_5 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f4 * k4[c] + f5 * k5[c];
          rhs_call(xt, k6); }
        { const double f1 = f78::a7_1 * cur, f4 = f78::a7_4 * cur, f5 = f78::a7_5 * cur, f6 = f78::a7_6 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f4 * k4[c] + f5 * k5[c] + f6 * k6[c];
          rhs_call(xt, k7); }
        { const double f1 = f78::a8_1 * cur, f5 = f78::a8_5 * cur, f6 = f78::a8_6 * cur, f7 = f78::a8_7 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xt[c] = x[c] + f1 * k1[c] + f5 * k5[c] + f6 * k6[c] + f7 * k7[c];
          rhs_call(xt, k8); }
        { const double f1 = f78::a9_1 * cur, f4 = f78::a9_4 * cur, f5 = f78::a9_5 * cur, f6 = f78::a9_6 * cur,
                       f7 = f78::a9_7 * cur, f8 = f78::a9_8 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c)
              xt[c] = x[c] + f1 * k1[c] + f4 * k4[c] + f5 * k5[c] + f6 * k6[c] + f7 * k7[c] + f8 * k8[c];
          rhs_call(xt, k9); }
        { const double f1 = f78::a10_1 * cur, f4 = f78::a10_4 * cur, f5 = f78::a10_5 * cur, f6 = f78::a10_6 * cur,
                       f7 = f78::a10_7 * cur, f8 = f78::a10_8 * cur, f9 = f78::a10_9 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c)
              xt[c] = x[c] + f1 * k1[c] + f4 * k4[c] + f5 * k5[c] + f6 * k6[c] + f7 * k7[c] + f8 * k8[c] + f9 * k9[c];
          rhs_call(xt, k10); }
        { const double f1 = f78::a11_1 * cur, f4 = f78::a11_4 * cur, f5 = f78::a11_5 * cur, f6 = f78::a11_6 * cur,
                       f7 = f78::a11_7 * cur, f8 = f78::a11_8 * cur, f9 = f78::a11_9 * cur, f10 = f78::a11_10 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c)
              xt[c] = x[c] + f1 * k1[c] + f4 * k4[c] + f5 * k5[c] + f6 * k6[c] + f7 * k7[c] + f8 * k8[c] + f9 * k9[c] + f10 * k10[c];
          rhs_call(xt, k11); }
        { const double e1 = f78::db1 * cur, e11 = f78::db11 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xerr[c] = e1 * k1[c] + e11 * k11[c]; }
        { const double f1 = f78::a12_1 * cur, f6 = f78::a12_6 * cur, f7 = f78::a12_7 * cur, f8 = f78::a12_8 * cur,
                       f9 = f78::a12_9 * cur, f10 = f78::a12_10 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c)
              xt[c] = x[c] + f1 * k1[c] + f6 * k6[c] + f7 * k7[c] + f8 * k8[c] + f9 * k9[c] + f10 * k10[c];
          rhs_call(xt, k12); }
        { const double f1 = f78::a13_1 * cur, f4 = f78::a13_4 * cur, f5 = f78::a13_5 * cur, f6 = f78::a13_6 * cur,
                       f7 = f78::a13_7 * cur, f8 = f78::a13_8 * cur, f9 = f78::a13_9 * cur, f10 = f78::a13_10 * cur,
                       f12 = f78::a13_12 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c)
              xt[c] = x[c] + f1 * k1[c] + f4 * k4[c] + f5 * k5[c] + f6 * k6[c] + f7 * k7[c] + f8 * k8[c] + f9 * k9[c]
                      + f10 * k10[c] + f12 * k12[c];
          rhs_call(xt, k13); }
        { const double e12 = f78::db12 * cur, e13 = f78::db13 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c) xerr[c] = xerr[c] + e12 * k12[c] + e13 * k13[c]; }
        // the 8th-order solution: b1..b5 = b11 = 0
        { const double f6 = f78::b6 * cur, f7 = f78::b7 * cur, f8 = f78::b8 * cur, f9 = f78::b9 * cur, f10 = f78::b10 * cur,
                       f12 = f78::b12 * cur, f13 = f78::b13 * cur;
          SEP_UNROLL for (int c = 0; c < N; ++c)
              xnew[c] = x[c] + f6 * k6[c] + f7 * k7[c] + f8 * k8[c] + f9 * k9[c] + f10 * k10[c] + f12 * k12[c] + f13 * k13[c]; }
    }
}
