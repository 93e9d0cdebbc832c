// csrc/sepaihrd_wave_chain.inc -- included by sepaihrd_kernels.hip (tolerance build only, inside its namespace).
//
// The evaluation kernel for the 4-age model with ONE WAVEFRONT PER CHAIN -- the mapping BASELINE.json's north star
// names -- kept as a MEASUREMENT (SEPAIHRD_WAVE_CHAIN=1|2; never launched otherwise).  It needs about 260 instructions
// per RK attempt of ONE chain (the 16-lane form: 92 per chain, the 4-lane form: 40): a lane carries a single state value,
// so the stage sums are 26 fused multiply-adds per attempt for the whole chain and the step control is wave-uniform.
// Measured (DESIGN.md section 3): no latency gain at any batch size -- with one value per lane every sum is a single
// dependent chain and a lone wave waits 8 cycles between dependent FP64 instructions -- and 1.3x (1024 chains) to 2.2x
// (4096) slower than the 16-lane form once a SIMD holds more than one of its waves.
//
//   lane = 16 * age + slot        (a 16-lane DPP row = one age class)
//   slot 0..10 = S, E, P, A, I, H, ICU, R, D, CumH, CumICU;  slot 11 = the age class's infectious pressure;  12..15 idle
//
// Right-hand side: every derivative is a sum of (rate) x (another compartment of the SAME age class) plus, for S and E,
// lambda_i S_i.  ONE instruction stream serves all lanes: ten v_fmac_f64_dpp, each adding (per-lane coefficient) x
// (row_newbcast of one compartment), in the order E, P, A, I, H, ICU, A, ICU, I, ICU -- a shortest sequence that contains
// every compartment's own association as the 4-lane kernel evaluates it (dR = ((g_I I + g_H H) + g_A A) + g_ICU ICU,
// dD = (d_H H + d_comm I) + d_ICU ICU, ...); a zero coefficient adds an exact zero.  The pressure P + A + theta I forms in
// slot 11 the same way, crosses the rows through v_readlane (four scalar pairs), and lambda_i = sum_j m_ij pi_j is four
// multiply-adds with scalar operands.  Same roundings in the same order as the other two forms: a chain's
// log-likelihood, step counts and trajectory are bit-identical whichever form evaluated it (tests/test_gpu_parity.py).
//
// The likelihood uses the separate pass (increments parked in the context's workspace: ten megabytes at 1024 chains).
#if SEPAIHRD_ARITH_FMA

constexpr int WC_PI_SLOT = 11;
constexpr int WAVE_CHAIN_MAX = 1024;  // SEPAIHRD_WAVE_CHAIN=1 uses the form up to here (one wave per SIMD)

struct WaveModel {
    double cW, cE, cP, cA, cI, cH, cICU, cA2, cICU2, cI3, cICU3;  // derivative of this lane's compartment
    double pP, pA, pI;                                          // slot 11: P + A + theta I
    double m[4];                                                 // (a_i M(i, j)) (h_infec_j / N_j) of this lane's age class
};

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// AgeSEPAIHRDModel::computeDerivatives, one compartment per lane; x = this lane's state value
__device__ __forceinline__ void rhs_wave(const WaveModel& q, const double x, double& dx, const double beta_eff) {
    double pr = 0.0;  // P + A + theta I in the slot-11 lanes: fma(1, P, 0) = P, fma(1, A, P) = P + A, fma(theta, I, P + A)
    fmac_row_bcast<2, 0xf, true>(pr, x, q.pP);
    fmac_row_bcast<3, 0xf, false>(pr, x, q.pA);
    fmac_row_bcast<4, 0xf, false>(pr, x, q.pI);
    // lambda_i = m_i0 pi_0 + ..., j ascending; pi_j sits in lane 16 j + 11
    double lambda = q.m[0] * readlane_f64(pr, 0 * 16 + WC_PI_SLOT);
    lambda = fma(q.m[1], readlane_f64(pr, 1 * 16 + WC_PI_SLOT), lambda);
    lambda = fma(q.m[2], readlane_f64(pr, 2 * 16 + WC_PI_SLOT), lambda);
    lambda = fma(q.m[3], readlane_f64(pr, 3 * 16 + WC_PI_SLOT), lambda);
    lambda *= beta_eff;
    const double lambda_val = (0.0 < lambda) ? lambda : 0.0;
    const double W = lambda_val * dpp_bcast_row<0, 0xf, 0, 0x0>(x);  // flow_SE = lambda_i S_i
    double acc = q.cW * W;                                             // -W in S, +W in E, 0 elsewhere
    fmac_row_bcast<1, 0xf, false>(acc, x, q.cE);  // x was written long before: no wait states needed
    fmac_row_bcast<2, 0xf, false>(acc, x, q.cP);
    fmac_row_bcast<3, 0xf, false>(acc, x, q.cA);
    fmac_row_bcast<4, 0xf, false>(acc, x, q.cI);
    fmac_row_bcast<5, 0xf, false>(acc, x, q.cH);
    fmac_row_bcast<6, 0xf, false>(acc, x, q.cICU);
    fmac_row_bcast<3, 0xf, false>(acc, x, q.cA2);
    fmac_row_bcast<6, 0xf, false>(acc, x, q.cICU2);
    fmac_row_bcast<4, 0xf, false>(acc, x, q.cI3);
    fmac_row_bcast<6, 0xf, false>(acc, x, q.cICU3);
    dx = acc;
}

template <int SOLVER>
__global__ __launch_bounds__(WAVE, 2) void sepaihrd_eval_wave_kernel(const DevProblem pb, const double* __restrict__ theta, const int B,
                                                                     const EvalOutputs out, const int cum_chains) {
    constexpr int LPC = 4;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* const lds_times = lds;
    double* const lds_mends = lds + times_pad(pb);
    double* const lds_bk = lds_mends + pb.nm_pad;      // [nm + 1]
    double* const lds_theta = lds_bk + (pb.nm + 1);    // [P]
    const int lane = threadIdx.x;
    const int age = lane >> 4, slot = lane & 15;
    const int comp = slot < NUM_COMP ? slot : -1;
    const long long chain = blockIdx.x;                // grid = B waves: every wave has its chain
    const int P = pb.P;

    for (int idx = lane; idx < P; idx += WAVE)
        lds_theta[idx] = constrain(theta[chain * P + idx], pb.lower[idx], pb.upper[idx], pb.has_bounds[idx], pb.constraint_mode);
    for (int k = lane; k < pb.nm_pad; k += WAVE) lds_mends[k] = pb.mends[k];
    for (int k = lane; k < pb.T; k += WAVE) lds_times[k] = pb.times[k];
    __syncthreads();
    const double* th = lds_theta;
    auto scalar_slot = [&](int s_) -> double {
        const int s = pb.src_scalar[s_];
        return s >= 0 ? th[s] : pb.base_scalar[s_];
    };
    auto vec_slot = [&](int field) -> double {
        const int s = pb.src_vec[field * LPC + age];
        return s >= 0 ? th[s] : pb.base_vec[field * LPC + age];
    };

    // ---- theta -> per-lane coefficients (the tolerance build's folds, as in the other two forms)
    WaveModel q;
    const double Ni = pb.N[age];
    {
        const double sigma = scalar_slot(SS_SIGMA), gamma_p = scalar_slot(SS_GAMMA_P), gamma_A = scalar_slot(SS_GAMMA_A),
                     gamma_I = scalar_slot(SS_GAMMA_I), gamma_H = scalar_slot(SS_GAMMA_H), gamma_ICU = scalar_slot(SS_GAMMA_ICU);
        const double a = vec_slot(VF_A), h_infec = vec_slot(VF_H_INFEC), p = vec_slot(VF_P), h = vec_slot(VF_H), icu = vec_slot(VF_ICU),
                     d_H = vec_slot(VF_D_H), d_ICU = vec_slot(VF_D_ICU), d_comm = vec_slot(VF_D_COMM);
        const double inv_N = (Ni > 1e-9) ? (1.0 / Ni) : 0.0;
        const double pg = rounded_here(p * gamma_p), pi_ = gamma_p - pg;
        const double r_I = gamma_I + h + d_comm, r_H = gamma_H + d_H + icu, r_ICU = gamma_ICU + d_ICU;
        const double c_inf = h_infec * inv_N;
        SEP_UNROLL
        for (int j = 0; j < LPC; ++j) q.m[j] = a * pb.Mrow[age * LPC + j] * readlane_f64(c_inf, 16 * j);
        auto pick = [&](int c, double v) -> double { return comp == c ? v : 0.0; };
        q.cW = pick(0, -1.0) + pick(1, 1.0);
        q.cE = pick(1, -sigma) + pick(2, sigma);
        q.cP = pick(2, -gamma_p) + pick(3, pg) + pick(4, pi_);
        q.cA = pick(3, -gamma_A);
        q.cI = pick(4, -r_I) + pick(5, h) + pick(7, gamma_I) + pick(9, h);
        q.cH = pick(5, -r_H) + pick(6, icu) + pick(7, gamma_H) + pick(8, d_H) + pick(10, icu);
        q.cICU = pick(6, -r_ICU);
        q.cA2 = pick(7, gamma_A);
        q.cICU2 = pick(7, gamma_ICU);
        q.cI3 = pick(8, d_comm);
        q.cICU3 = pick(8, d_ICU);
        const bool pi_lane = slot == WC_PI_SLOT;
        q.pP = pi_lane ? 1.0 : 0.0;
        q.pA = pi_lane ? 1.0 : 0.0;
        q.pI = pi_lane ? scalar_slot(SS_THETA) : 0.0;
    }

    Schedule sch;
    sch.me = lds_mends;
    for (int j = lane; j <= pb.nm; j += WAVE) {
        const double beta = (pb.nb > 0) ? scalar_slot(SS_SCHEDULE0 + pb.seg_ib[j]) : scalar_slot(SS_BETA);
        const double kappa = scenario_kappa(pb, chain, pb.seg_ik[j], scalar_slot(SS_SCHEDULE0 + pb.nb + pb.seg_ik[j]));
        lds_bk[j] = beta * kappa;
    }
    sch.bkv = lds_bk;

    int status = 0;
    if (pb.kappa_calibrated) {
        bool neg = false;
        for (int k = 1; k < pb.nk; ++k) neg |= (scalar_slot(SS_SCHEDULE0 + pb.nb + k) < 0.0);
        if (neg) status = 1;
    }
    if (!pb.obs_rows_match && pb.init_mode == 0) status = 1;

    // ---- initial state (SEPAIHRDObjectiveFunction.cpp:124-163); the sum over E..D runs in compartment order
    double x = (comp >= 0) ? pb.init_state[comp * LPC + age] : 0.0;
    if (pb.init_mode != 1) {
        const double runup_days = scalar_slot(SS_RUNUP_DAYS);
        const double seed_exposed = scalar_slot(SS_SEED_EXPOSED);
        if (pb.init_mode == 0 && runup_days > 0 && seed_exposed > 0) {
            if (comp == 1) x = seed_exposed * pb.age_fraction[age];
            else if (comp >= 2) x = 0.0;
        } else if (comp >= 1 && comp <= 8) {
            x *= scalar_slot(SS_E0_MULT + (comp - 1));
        }
        double sum = 0;
        sum += dpp_bcast_row<1, 0xf, 1, 0x0>(x); sum += dpp_bcast_row<2, 0xf, 2, 0x0>(x); sum += dpp_bcast_row<3, 0xf, 3, 0x0>(x);
        sum += dpp_bcast_row<4, 0xf, 4, 0x0>(x); sum += dpp_bcast_row<5, 0xf, 5, 0x0>(x); sum += dpp_bcast_row<6, 0xf, 6, 0x0>(x);
        sum += dpp_bcast_row<7, 0xf, 7, 0x0>(x); sum += dpp_bcast_row<8, 0xf, 8, 0x0>(x);
        if (__ballot(sum > Ni || (pb.init_mode == 2 && sum < 0)) != 0ull) status = 1;
        if (comp == 0) x = Ni - sum;
    }
    __syncthreads();

    int n_acc = 0, n_rej = 0;
    const int T = pb.T;
    const int n_real = pb.n;
    // observer: the lanes of D, CumH, CumICU park their daily increments for the likelihood pass
    const int which = comp == 8 ? 0 : (comp == 9 ? 1 : 2);
    const bool stores = comp >= 8;
    double* cum_row = out.cum + cum_index(pb.T, (size_t)chain * LPC + age, 0, which);
    const size_t cum_step = CUM_ROW_DOUBLES;
    double prev = x;
    auto observe_store = [&](int k) {
        if (stores) *cum_row = x - prev;
        cum_row += cum_step;
        prev = x;
        if (out.traj != nullptr && comp >= 0 && age < n_real)
            out.traj[((size_t)chain * T + k) * (NUM_COMP * n_real) + (size_t)comp * n_real + age] = x;
    };

    bool active = (status == 0);
    int k_next = 1;
    double t = pb.times[0];
    double dt = pb.dt_hint;
    int fails = 0, attempts = 0;
    double t_next = (T > 1) ? pb.times[1] : t;
    double t_after = (T > 2) ? pb.times[2] : t_next;
    if (active) observe_store(0);
    if (T <= 1) active = false;

    sch.lo = INFINITY; sch.hi = -INFINITY; sch.bk = 0.0;
    double k1[1] = {0.0};
    if (SOLVER == 0) {
        int c0, c1;
        segment_index2(sch, pb.nm_pad, t, t, c0, c1);
        rhs_wave(q, x, k1[0], sch.bkv[c0]);
    }
    const double eps_abs = pb.abs_tol, eps_rel = pb.rel_tol;
    const double coefA = QUAD_COEF[SOLVER][0][lane & 15], coefB = QUAD_COEF[SOLVER][1][lane & 15];

    // every per-chain quantity is the same in all 64 lanes: the branches below are uniform
    while (active) {
        const double cur = fmin(dt, t_next - t);
        double vecA, vecB;
        asm("v_mul_f64 %0, %2, %3\n\tv_mul_f64 %1, %2, %4\n\ts_nop 1" : "=&v"(vecA), "=&v"(vecB) : "v"(cur), "v"(coefA), "v"(coefB));
        double tau[7], bks[7];
        if (SOLVER == 0) {
            tau[0] = t;
            tau[1] = t + cur * dp::a2; tau[2] = t + cur * dp::a3; tau[3] = t + cur * dp::a4;
            tau[4] = t + cur * dp::a5; tau[5] = t + cur; tau[6] = t + cur;
        } else {
            tau[0] = t;
            tau[1] = t + ck::c2 * cur; tau[2] = t + ck::c3 * cur; tau[3] = t + ck::c4 * cur;
            tau[4] = t + ck::c5 * cur; tau[5] = t + ck::c6 * cur; tau[6] = t + cur;
        }
        {
            const double tmin = (SOLVER == 0) ? tau[1] : tau[0];
            const double tmax = (SOLVER == 0) ? tau[6] : tau[4];
            const bool in_seg = (tmin > sch.lo) && (tmax <= sch.hi);
            if (__ballot(!in_seg) != 0ull) {
                int c_lo, c_hi;
                segment_index2(sch, pb.nm_pad, tmin, tmax, c_lo, c_hi);
                const double v_lo = sch.bkv[c_lo], v_hi = sch.bkv[c_hi];
                if (c_hi <= c_lo + 1) {
                    const double bpt = (c_lo < pb.nm) ? sch.me[c_lo] : INFINITY;
                    SEP_UNROLL
                    for (int s = 0; s < 7; ++s) bks[s] = (tau[s] > bpt) ? v_hi : v_lo;
                } else {
                    for (int s = 0; s < 7; ++s) {
                        int ca, cb;
                        segment_index2(sch, pb.nm_pad, tau[s], tau[s], ca, cb);
                        bks[s] = sch.bkv[ca];
                    }
                }
                sch.lo = (c_hi > 0) ? sch.me[c_hi - 1] : -INFINITY;
                sch.hi = (c_hi < pb.nm) ? sch.me[c_hi] : INFINITY;
                sch.bk = v_hi;
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): no waits left for the stage code
            } else {
                SEP_UNROLL
                for (int s = 0; s < 7; ++s) bks[s] = sch.bk;
            }
        }

        double k2[1], k3[1], k4[1], k5[1], k6[1], k7[1], xnew[1], xerr[1];
        const double xs[1] = {x};
        rk_stages_row_coef<SOLVER, 1>(cur, vecA, vecB, xs, k1, k2, k3, k4, k5, k6, k7, xnew, xerr, bks,
                                      [&](const double (&xin)[1], double (&kout)[1], double bk) { rhs_wave(q, xin[0], kout[0], bk); });

        // default_error_checker / default_step_adjuster: as in the other forms, with a whole-wave maximum
        const double sc = eps_abs + eps_rel * (fabs(x) + cur * fabs(k1[0]));
        const double ea = fabs(xerr[0]);
        const bool over = __ballot(ea > sc) != 0ull;
        const bool grow_relevant = (dt < pb.max_gap) && (4.5000001 * cur > dt);
        double err = 0.0;
        if (over || grow_relevant) {
            err = max_keep(0.0, quotient(ea, sc));
            err = group_max<16>(err);                                      // every row holds its maximum
            err = max_keep(max_keep(readlane_f64(err, 0), readlane_f64(err, 16)), max_keep(readlane_f64(err, 32), readlane_f64(err, 48)));
        }
        const bool reject = err > 1.0;
        ++attempts;
        const bool need_inc = !reject && (err < 0.5) && grow_relevant;
        double cur_after = cur;
        if (reject || need_inc) {
            const double arg = max_moved_uniform(err, 1.0 / 3125.0);  // 5^-5: the floor of the increase rule; a rejected step has err > 1
            const double expo = reject ? -1.0 / (4 - 1) : -1.0 / 5;
            const double pw = 9.0 / 10.0 * pow_ctl(arg, expo);
            cur_after = cur * fmax(pw, 1.0 / 5.0);  // the floor of the decrease rule; an increase has pw > 1 (err < 0.5)
        }
        if (reject) {
            ++n_rej;
            dt = cur_after;
            if (fails >= 500) { status = 2; active = false; }
            ++fails;
        } else {
            ++n_acc;
            dt = fmax(dt, cur_after);
            fails = 0;
            t += cur;
            x = xnew[0];
            if (SOLVER == 0) k1[0] = k7[0];
            if (!((t_next - t) > DBL_EPSILON)) {
                observe_store(k_next);
                t = t_next;
                ++k_next;
                if (k_next >= T) active = false;
                t_next = t_after;
                t_after = lds_times[(k_next + 1 < T) ? k_next + 1 : T - 1];
            }
        }
        if (active && attempts >= pb.max_attempts) { status = 3; active = false; }
    }

    if (lane == 0) {
        out.wstatus[chain] = status;  // the likelihood pass finishes the evaluation
        if (out.n_accept) out.n_accept[chain] = n_acc;
        if (out.n_reject) out.n_reject[chain] = n_rej;
    }
}

// SEPAIHRD_WAVE_CHAIN=1 uses this form for batches of up to WAVE_CHAIN_MAX chains of a 4-age problem, =2 at any batch
// size (measurement switches); unset or 0: never
inline bool wave_chain_wanted(int B) {
    static const int mode = [] {
        const char* e = getenv("SEPAIHRD_WAVE_CHAIN");
        return e == nullptr ? -1 : atoi(e);
    }();
    return mode < 0 ? false : (mode == 1 ? B <= WAVE_CHAIN_MAX : mode != 0);
}
inline size_t wave_chain_lds_bytes(const DevProblem& pb) {
    return ((size_t)times_pad(pb) + pb.nm_pad + (pb.nm + 1) + pb.P) * sizeof(double);
}

template <int SOLVER>
int launch_wave_chain(const DevProblem& pb, const double* d_theta, int B, const EvalOutputs& out, void* stream) {
    if (out.cum == nullptr || out.rows == nullptr || out.wstatus == nullptr) return -5;  // see needs_workspace_one()
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ll_blocks = (B + 15) / 16;  // the likelihood passes keep the 4-lane column layout
    const int cum_chains = ll_blocks * 16;
    hipLaunchKernelGGL((sepaihrd_eval_wave_kernel<SOLVER>), dim3(B), dim3(WAVE), wave_chain_lds_bytes(pb), st, pb, d_theta, B, out, cum_chains);
    if (out.ev_after_integrator) (void)hipEventRecord(static_cast<hipEvent_t>(out.ev_after_integrator), st);
    if (out.force_split == FORCE_SPLIT_PARK_ONLY) return hipGetLastError() == hipSuccess ? 0 : -3;  // the caller's own pass follows
    hipLaunchKernelGGL((sepaihrd_ll_terms_kernel<4>), dim3(ll_blocks, (pb.T + LL_DAYS_PER_BLOCK - 1) / LL_DAYS_PER_BLOCK),
                       dim3(WAVE * LL_DAYS_PER_BLOCK), 0, st, pb, B, out, cum_chains);
    hipLaunchKernelGGL(sepaihrd_ll_reduce_kernel, dim3((B + 15) / 16), dim3(WAVE), 0, st, pb, B, out, cum_chains, pb.T);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
#endif  // SEPAIHRD_ARITH_FMA
