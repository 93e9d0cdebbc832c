// =============================================================================
// csrc/sepaihrd_sir.hip -- gfx950 kernels for one PoissonLikelihoodObjective::calculate of the age-structured SIR
// model per chain:
//     theta -> constrained q / scale_C_total / gamma_i -> adaptive RK (Dopri5 FSAL / Cash-Karp 5(4) / Fehlberg 7(8))
//     from the problem's fixed initial state over the output grid -> incidence lambda_i(x(t)) S_i(t) at every output
//     time -> Poisson log-likelihood.
//
// Mapping: as sepaihrd_eval_kernel (sepaihrd_kernels.hip) -- one LANE per (chain, age class), a chain is a group of
// LPC = pow2(n) adjacent lanes, a wavefront integrates 64 / LPC chains; S, I, R of the age class, the stage derivatives,
// the chain's parameters and the lane's row of the scaled contact matrix live in VGPRs.  Cross-lane traffic: the
// contact-row contraction of the force of infection (DPP broadcasts up to 16 lanes, ds_bpermute above), the max-norm of
// the error estimate, the age sum of the Poisson terms of an output time.  The incidence needs only x(t), so the terms
// are formed at each output point inside the integrator and added in (t, i) row order: no second pass, no HBM traffic
// but theta in and the results out.
//
// Compiled twice: -DSEPAIHRD_ARITH_FMA=0 -ffp-contract=off (the CPU build's operation sequence) and
// -DSEPAIHRD_ARITH_FMA=1 -ffp-contract=fast (contraction left to the compiler, reciprocal instead of division in the
// error norm and in I / N, single-precision pow in the controller).
//
// Reference behaviour followed (paths under the reference tree):
//   RHS                 src/sir_age_structured/AgeSIRModel.cpp:106-139
//   constraints, theta  src/sir_age_structured/parameters/SIRParameterManager.cpp:98-156
//   incidence           src/sir_age_structured/SimulationResultProcessor.cpp:144-189
//   objective           src/sir_age_structured/objectives/PoissonLikelihoodObjective.cpp:46-144
//   integrator          Boost.Odeint integrate_times + controlled_runge_kutta, as sepaihrd_kernels.hip
// =============================================================================
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <utility>

#include "sepaihrd_device.h"
#include "sepaihrd_sir_device.h"

#ifndef SEPAIHRD_ARITH_FMA
#error "compile with -DSEPAIHRD_ARITH_FMA=0 or 1"
#endif
// The ensemble build (csrc/Makefile sir_ens_*.o, sepaihrd_sir_scenario_ensemble): the same integrator with a per-chain
// cursor over the intervention events of the chain's scenario, the restart an event asks for, and an observer that stores
// incidence, prevalence and cumulative infections of every output time instead of forming Poisson terms.  Every addition
// is under this macro: without it the translation unit is token for token the one the shipped objects were compiled from.
#ifndef SEPAIHRD_SIR_ENSEMBLE
#define SEPAIHRD_SIR_ENSEMBLE 0
#endif
#if SEPAIHRD_SIR_ENSEMBLE
#define sepaihrd_sir_eval_kernel sepaihrd_sir_ens_kernel
#endif

namespace sepaihrd {
namespace {

#include "sepaihrd_dev_common.inc"    // cross-lane helpers, tableaus, log_pos
#include "sepaihrd_step_control.inc"  // quotient, pow_ctl
#include "sepaihrd_rk_stages.inc"     // rk_attempt

enum SirField { SIR_F_Q = 0, SIR_F_SCALE = 1, SIR_F_GAMMA = 2 };  // include/sepaihrd_hip.h SEPAIHRD_SIR_F_*

// this lane's age class of one chain
template <int LPC, bool RL>
struct SirLane {
    double q, gamma;
    double n_or_inv;  // strict: N_i (I / N is a division, as in the CPU build); fma: 1 / N_i
    bool has_pop;     // N_i > 1e-9
    // (C(i, j) scale), j = 0 .. LPC-1: the row of C_current.  Up to sixteen lanes per chain it lives in registers and the
    // I / N of the other ages come by DPP; above that a register row (64 or 128 VGPRs) and 32 or 64 unrolled ds_bpermute per
    // call do not fit without spills, so the rows sit transposed in LDS ([j][lane]: conflict-free) next to one exchange
    // slot per lane.
    double cs[RL ? 1 : LPC];
    const double* cs_t;  // LDS [LPC][WAVE] (RL: rows in LDS)
    double* xch;         // LDS [WAVE]      (RL)
    int lane;
};
// (the strict Fehlberg 7(8) stepper of sixteen ages as well: thirteen stage vectors and a 32-register row pass 256 VGPRs)
constexpr bool sir_rows_in_lds(int lpc, int solver) { return lpc > 16 || (lpc == 16 && solver == 2 && SEPAIHRD_ARITH_FMA == 0); }

// value v of every lane of my chain group visible in m.xch (rows in LDS).  One wavefront per block: the barrier orders
// the compiler's LDS accesses, the wave's LDS instructions execute in order.
template <int LPC, bool RL>
__device__ __forceinline__ void publish(const SirLane<LPC, RL>& m, double v) {
    __syncthreads();  // the readers of the previous exchange are done
    m.xch[m.lane] = v;
    __syncthreads();
}

// lambda_i = max(q (C_current (I / N))_i, 0), the row sum left to right over j.  Every lane of the wave calls it.
template <int LPC, bool RL>
__device__ __forceinline__ double sir_lambda(const SirLane<LPC, RL>& m, double I) {
#if SEPAIHRD_ARITH_FMA
    const double ion = m.has_pop ? I * m.n_or_inv : 0.0;
#else
    const double ion = m.has_pop ? I / m.n_or_inv : 0.0;
#endif
    double acc;
    if constexpr (RL) {
        publish<LPC, RL>(m, ion);
        const double* mine = m.xch + (m.lane & ~(LPC - 1));
        acc = m.cs_t[m.lane] * mine[0];
#pragma unroll 4
        for (int j = 1; j < LPC; ++j) acc += m.cs_t[j * WAVE + m.lane] * mine[j];
    } else {
        acc = m.cs[0] * group_bcast<LPC, 0>(ion);
        [&]<int... J>(std::integer_sequence<int, J...>) {
            ((acc += m.cs[J + 1] * group_bcast<LPC, J + 1>(ion)), ...);
        }(std::make_integer_sequence<int, LPC - 1>{});
    }
    const double lambda = m.q * acc;
    return (lambda < 0.0) ? 0.0 : lambda;  // std::max(lambda, 0.0)
}

// a value pinned to vector registers: what is needed only after the step loop (result addresses) or once per output would
// otherwise be kept in -- and spilled from -- the scalar file, which the tableau's 64-bit literals fill
template <class T>
__device__ __forceinline__ T in_vgpr(T v) {
    asm volatile("" : "+v"(v));
    return v;
}

// AgeSIRModel::computeDerivatives for this lane's age class
template <int LPC, bool RL>
__device__ __forceinline__ void sir_rhs(const SirLane<LPC, RL>& m, const double (&x)[SIR_COMP], double (&dx)[SIR_COMP]) {
    const double S = x[0], I = x[1], R = x[2];
    const double lambda = sir_lambda<LPC, RL>(m, I);
    double dS = -lambda * S;
    double dI = lambda * S - m.gamma * I;
    double dR = m.gamma * I;
    if (S < 1e-9 && dS < 0) dS = 0.0;
    if (I < 1e-9 && dI < 0) dI = 0.0;
    if (R < 1e-9 && dR < 0) dR = 0.0;
    dx[0] = dS; dx[1] = dI; dx[2] = dR;
}

// ----------------------------------------------------------------------------------
// the evaluation kernel: block = one wavefront = 64 / LPC chains
// ----------------------------------------------------------------------------------
template <int LPC, int SOLVER, int ARITH_FMA>
__global__ __launch_bounds__(WAVE) void sepaihrd_sir_eval_kernel(const SirDevProblem pb, const double* __restrict__ theta,
                                                                 const int B, const SirOutputs out
#if SEPAIHRD_SIR_ENSEMBLE
                                                                 , const SirEnsArgs ens
#endif
                                                                 ) {
    constexpr int CPW = WAVE / LPC;
    constexpr bool RL = sir_rows_in_lds(LPC, SOLVER);
    const int lane = threadIdx.x;
    const int grp = lane / LPC;
    const int age = lane % LPC;
    const long long chain0 = (long long)blockIdx.x * CPW;
    const int chains_here = (B - chain0) < CPW ? (int)(B - chain0) : CPW;
    const bool chain_valid = grp < chains_here;
    // lanes of a group past the end of the batch shadow group 0 (always valid): same control flow, no stores
    const int g = chain_valid ? grp : 0;
    const long long chain = chain0 + g;
    const int T = pb.T, n = pb.n, P = pb.P;
    const int age_real = in_vgpr(age < n ? 1 : 0);

    extern __shared__ __attribute__((aligned(16))) double sir_lds[];  // LPC > 16: [LPC][WAVE] contact rows, [WAVE] exchange
#if !SEPAIHRD_SIR_ENSEMBLE
    stage_log_table(lane, WAVE);  // the Poisson term's log reads its table from LDS
    __syncthreads();
#endif

    // ---- 1. applyConstraints + updateModelParameters: later entries overwrite earlier ones, as the loop over names does
    SirLane<LPC, RL> m;
    double scale = pb.scale;
    m.q = pb.q;
    m.gamma = pb.gamma[age];
    {
        const double* th = theta + chain * P;
        for (int p = 0; p < P; ++p) {
            const int f = pb.param_field[p];
            const double v = th[p];
            if (f == SIR_F_Q) m.q = (1e-12 < v) ? v : 1e-12;           // std::max(1e-12, v)
            else if (f == SIR_F_SCALE) scale = (0.0 < v) ? v : 0.0;     // std::max(0.0, v)
            else if (f == SIR_F_GAMMA && pb.param_index[p] == age) m.gamma = (0.0 < v) ? v : 0.0;
        }
    }
#if SEPAIHRD_SIR_ENSEMBLE
    // the chain's scenario and its event cursor.  The table is read per lane: a wavefront can straddle two scenarios.
    // ev_k is the grid index of the next event (-1: none left), so the step loop compares registers only.
    const int scen = (int)(chain / ens.S);
    const int samp = (int)(chain - (long long)scen * ens.S);
    const SirEvent* ev_cur = ens.events + (size_t)scen * SIR_MAX_EVENTS;
    int ev_left = ens.n_events[scen];
    int ev_k = (ev_left > 0) ? ev_cur->time_index : -1;
    // the events of grid index k in listed order, compounding as repeated AgeSIRModel::applyIntervention calls do
    // (AgeSIRModel.cpp:141-173): contact kinds scale scale_C_total, transmission kinds scale q by 1 - r
    auto apply_events = [&](bool on, int k) {
        while (on && ev_k == k) {
            const double v = ev_cur->value;
            if (ev_cur->kind == SIR_EV_CONTACT) scale = scale * v;
            else m.q = m.q * (1.0 - v);
            ++ev_cur;
            --ev_left;
            ev_k = (ev_left > 0) ? ev_cur->time_index : -1;
        }
    };
    apply_events(true, 0);  // before the first observation: a plain run with the changed parameters
#endif
    const double Ni = pb.N[age];
    m.has_pop = Ni > 1e-9;
#if SEPAIHRD_ARITH_FMA
    m.n_or_inv = m.has_pop ? 1.0 / Ni : 0.0;
#else
    m.n_or_inv = Ni;
#endif
    m.lane = lane;
    m.cs_t = sir_lds;
    m.xch = sir_lds + (RL ? LPC * WAVE : 0);
    if constexpr (RL) {
        for (int j = 0; j < LPC; ++j) sir_lds[j * WAVE + lane] = pb.C[age * LPC + j] * scale;
        __syncthreads();
    } else {
        SEP_UNROLL
        for (int j = 0; j < LPC; ++j) m.cs[j] = pb.C[age * LPC + j] * scale;  // C_current = scale_C_total * C_baseline
    }

#if SEPAIHRD_SIR_ENSEMBLE
    // C_current of the chains with `on` set re-formed from the baseline row and the scale now in force (not the stored row
    // times the event's value: this is what a model constructed with the new scale_C_total holds)
    auto form_rows = [&](bool on) {
        if constexpr (RL) {
            for (int j = 0; j < LPC; ++j)
                if (on) sir_lds[j * WAVE + lane] = pb.C[age * LPC + j] * scale;
        } else {
            if (on) {
                SEP_UNROLL
                for (int j = 0; j < LPC; ++j) m.cs[j] = pb.C[age * LPC + j] * scale;
            }
        }
    };
    int status = 0;  // the observations play no part here
#else
    int status = pb.obs_not_finite ? 1 : 0;  // y_obs.allFinite() fails whatever the simulation gives
#endif

    // ---- 2. the problem's fixed initial state
    double x[SIR_COMP];
    SEP_UNROLL
    for (int c = 0; c < SIR_COMP; ++c) x[c] = pb.init_state[c * LPC + age];

    // Observer at output index k for the chains with do_it set: incidence_i = lambda_i(x(t)) S_i(t), sim = max(incidence, 1e-9),
    // term = obs log(sim) - sim; the terms of the row are added to the chain's sum in ascending age order (row order of the
    // (t, i) matrix).  All lanes execute; terms of chains without do_it and of padded ages are +0.0.
#if SEPAIHRD_SIR_ENSEMBLE
    const double* times_v = in_vgpr(pb.times);
    const int writer = in_vgpr((chain_valid && age == 0) ? 1 : 0);
    // this lane's column of output time 0, series 0 of the chain's scenario; rows are ens_row doubles apart, series T rows
    double* ens_dst = in_vgpr(chain_valid ? ens.vals + ((size_t)scen * SIR_ENS_SERIES * T * (n + 1) + age) * (size_t)ens.S_pad + samp : nullptr);
    const size_t ens_row = in_vgpr((size_t)(n + 1) * (size_t)ens.S_pad);
    const size_t ens_total = in_vgpr((size_t)(n - age) * (size_t)ens.S_pad);  // from this lane's column to the age total's
    const double* s0_lane = in_vgpr(pb.init_state + age);
    const int ens_T = in_vgpr(T);
#else
    const double* obs_lane = in_vgpr(pb.obs + age);
    const double* times_v = in_vgpr(pb.times);
    const int traj_n = in_vgpr(n);
    double* traj_lane = in_vgpr((out.traj != nullptr && chain_valid) ? out.traj + (size_t)chain * T * ((size_t)SIR_COMP * n) + age : nullptr);
    const int writer = in_vgpr((chain_valid && age == 0) ? 1 : 0);  // a lane mask kept to the end would sit in scalar registers
    double* ll_dst = in_vgpr(out.loglik + chain);
#endif
    int32_t* status_dst = in_vgpr(out.status ? out.status + chain : nullptr);
    int32_t* nacc_dst = in_vgpr(out.n_accept ? out.n_accept + chain : nullptr);
    int32_t* nrej_dst = in_vgpr(out.n_reject ? out.n_reject + chain : nullptr);
    const int max_attempts = in_vgpr(pb.max_attempts);
    const double max_gap = in_vgpr(pb.max_gap);
#if SEPAIHRD_SIR_ENSEMBLE
    // Observer of the ensemble build at output index k for the chains with do_it set: series 0 incidence_i = lambda_i(x(t))
    // S_i(t) with the parameters in force (no 1e-9 floor), 1 prevalence I_i(t), 2 cumulative infections S_i(t0) - S_i(t),
    // each with its age total (ages added in ascending order) in column n.  All lanes execute; padded ages add +0.0.
    bool not_finite = false;
    auto observe = [&](bool do_it, int k) {
        const double inc = sir_lambda<LPC, RL>(m, x[1]) * x[0];
        const bool use = do_it && age_real != 0;
        not_finite |= use && !isfinite(inc);
        const double v[SIR_ENS_SERIES] = {use ? inc : 0.0, use ? x[1] : 0.0, use ? s0_lane[0] - x[0] : 0.0};
        double tot[SIR_ENS_SERIES] = {0.0, 0.0, 0.0};
        SEP_UNROLL
        for (int ser = 0; ser < SIR_ENS_SERIES; ++ser) {
            if constexpr (RL) {
                publish<LPC, RL>(m, v[ser]);
                const double* mine = m.xch + (lane & ~(LPC - 1));
#pragma unroll 4
                for (int j = 0; j < LPC; ++j) tot[ser] += mine[j];
            } else {
                [&]<int... J>(std::integer_sequence<int, J...>) {
                    ((tot[ser] += group_bcast<LPC, J>(v[ser])), ...);
                }(std::make_integer_sequence<int, LPC>{});
            }
        }
        if (ens_dst != nullptr && use) {
            double* d = ens_dst + (size_t)k * ens_row;
            const size_t ser_stride = (size_t)ens_T * ens_row;
            SEP_UNROLL
            for (int ser = 0; ser < SIR_ENS_SERIES; ++ser) {
                d[ser * ser_stride] = v[ser];
                if (writer != 0) d[ser * ser_stride + ens_total] = tot[ser];
            }
        }
    };
#else
    double ll = 0.0;
    bool not_finite = false;
    auto observe = [&](bool do_it, int k) {
        const double obs = obs_lane[(size_t)k * LPC];
        const double inc = sir_lambda<LPC, RL>(m, x[1]) * x[0];
        const double sim = (inc < 1e-9) ? 1e-9 : inc;  // cwiseMax(1e-9)
        const bool use = do_it && age_real != 0;
        not_finite |= use && !isfinite(inc);              // y_sim.allFinite()
        const double v = obs * log_pos(sim) - sim;
        const double term = use ? v : 0.0;
        if constexpr (RL) {
            publish<LPC, RL>(m, term);
            const double* mine = m.xch + (lane & ~(LPC - 1));
#pragma unroll 4
            for (int j = 0; j < LPC; ++j) ll += mine[j];
        } else {
            [&]<int... J>(std::integer_sequence<int, J...>) {
                ((ll += group_bcast<LPC, J>(term)), ...);
            }(std::make_integer_sequence<int, LPC>{});
        }
        if (traj_lane != nullptr && use) {
            double* tdst = traj_lane + (size_t)k * ((size_t)SIR_COMP * traj_n);
            SEP_UNROLL
            for (int c = 0; c < SIR_COMP; ++c) tdst[c * traj_n] = x[c];
        }
    };
#endif

    // ---- 3. integrate_times(controlled stepper, ..., times, dt_hint, observer)
    int n_acc = 0, n_rej = 0;
    bool active = (status == 0);
    int k_next = 1;
    double t = times_v[0];
    double t_next = (T > 1) ? times_v[1] : t;
    double dt = pb.dt_hint;
    int fails = 0, attempts = 0;
    observe(active, 0);
    if (T <= 1) active = false;

    auto rhs_call = [&](const double (&xin)[SIR_COMP], double (&kout)[SIR_COMP]) { sir_rhs<LPC, RL>(m, xin, kout); };
    double k1[SIR_COMP];
    if constexpr (SOLVER == 0) rhs_call(x, k1);  // controlled FSAL stepper: initialize() at the first try_step
    const double eps_abs = in_vgpr(pb.abs_tol), eps_rel = in_vgpr(pb.rel_tol);
    // default_step_adjuster: stepper order 5 / error order 4 for Dopri5 and Cash-Karp; 8 / 7 for Fehlberg 7(8)
    constexpr double CTL_FLOOR = SOLVER == 2 ? 1.0 / 390625.0 : 1.0 / 3125.0;
    constexpr double CTL_EXPO_DEC = SOLVER == 2 ? -1.0 / (7 - 1) : -1.0 / (4 - 1);
    constexpr double CTL_EXPO_INC = SOLVER == 2 ? -1.0 / 8 : -1.0 / 5;

    while (__ballot(active) != 0ull) {
        // min_abs(dt, t_next - t); finished chains idle with a harmless unit step
        const double cur = active ? fmin(dt, t_next - t) : 1.0;
        double k7[SIR_COMP], xnew[SIR_COMP], xerr[SIR_COMP];
        rk_attempt<SOLVER, SIR_COMP>(cur, x, k1, k7, xnew, xerr, rhs_call);

        // default_error_checker: err = max_i |xerr_i| / (eps_abs + eps_rel (|x_i| + dt |dxdt_i|)) over all 3 n components of the
        // chain, start-of-step x and dxdt; reject iff err > 1.  |e| <= s  =>  fl(|e| / s) <= 1, so the quotients are only formed
        // when one may exceed 1 or when err feeds the controller (sepaihrd_eval_kernel has the argument in full).
        double sc[SIR_COMP], ea[SIR_COMP];
        bool over = false;
        SEP_UNROLL
        for (int c = 0; c < SIR_COMP; ++c) {
            sc[c] = eps_abs + eps_rel * (fabs(x[c]) + cur * fabs(k1[c]));
            ea[c] = fabs(xerr[c]);
            over |= (ea[c] > sc[c]);
        }
        // growth multiplies the trial step by at most 4.5 and only matters while dt is below the largest output gap
        const bool grow_relevant = (dt < max_gap) && (4.5000001 * cur > dt);
        const bool need_err = active && (over || grow_relevant);
        double err = 0.0;
        if (__ballot(need_err) != 0ull) {
            SEP_UNROLL
            for (int c = 0; c < SIR_COMP; ++c) err = max_keep(err, quotient(ea[c], sc[c]));
            err = group_max<LPC>(err);
        }
        const bool reject = err > 1.0;
        ++attempts;
        const bool need_dec = active && reject;
        const bool need_inc = active && !reject && (err < 0.5) && grow_relevant;
        double cur_after = cur;
        if (__ballot(need_dec || need_inc) != 0ull) {
            const double arg = fmax(err, CTL_FLOOR);  // 5^-order: the floor of the increase rule; a rejected step has err > 1
            const double expo = need_dec ? CTL_EXPO_DEC : CTL_EXPO_INC;
            const double pw = 9.0 / 10.0 * pow_ctl(arg, expo);
            const double f = fmax(pw, 1.0 / 5.0);  // the floor of the decrease rule; an increase has pw > 1 (err < 0.5)
            if (need_dec || need_inc) cur_after = cur * f;
        }
        const bool rej = active && reject;
        const bool acc = active && !reject;
        n_rej += rej ? 1 : 0;
        n_acc += acc ? 1 : 0;
        // failure: dt = reduced current_dt; success: dt = max_abs(dt, current_dt)
        dt = rej ? cur_after : (acc ? fmax(dt, cur_after) : dt);
        // failed_step_checker: throws when 500 consecutive failures precede this one
        if (rej && fails >= 500) { status = 2; active = false; }
        fails = acc ? 0 : fails + (rej ? 1 : 0);
        if (acc) {
            t += cur;
            SEP_UNROLL
            for (int c = 0; c < SIR_COMP; ++c) x[c] = xnew[c];
            if constexpr (SOLVER == 0) {
                SEP_UNROLL
                for (int c = 0; c < SIR_COMP; ++c) k1[c] = k7[c];
            }
        }
        // less_with_sign(t, t_next, dt): t_next - t > epsilon
        const bool reached = acc && !((t_next - t) > DBL_EPSILON);
        if (__ballot(reached) != 0ull) {
            observe(reached, reached ? k_next : 0);
#if SEPAIHRD_SIR_ENSEMBLE
            // An event at this grid index: the row just stored belongs to the interval that ends here (old parameters); now
            // the parameters change and the integrator restarts as a fresh integrate_times call would -- dt = dt_hint, no
            // consecutive failures, the FSAL derivative recomputed.  attempts and the step counters run on.
            const bool restart = reached && k_next == ev_k;
            if (__ballot(restart) != 0ull) {
                apply_events(restart, k_next);
                form_rows(restart);
                if (restart) { dt = pb.dt_hint; fails = 0; }
                if constexpr (SOLVER == 0) {
                    double kr[SIR_COMP];
                    rhs_call(x, kr);  // every lane calls: the contraction is cross-lane
                    SEP_UNROLL
                    for (int c = 0; c < SIR_COMP; ++c) k1[c] = restart ? kr[c] : k1[c];
                }
            }
#endif
            if (reached) {
                t = t_next;  // integrate_times re-reads the exact grid time
                ++k_next;
                if (k_next >= T) active = false;
                else t_next = times_v[k_next];
            }
        }
        if (active && attempts >= max_attempts) { status = 3; active = false; }
    }

    // ---- 4. the total (PoissonLikelihoodObjective.cpp:84-108, :128-141): every failure is -infinity, nothing throws
    const bool any_not_finite = group_any<LPC>(not_finite, lane);
    if (writer != 0) {
#if SEPAIHRD_SIR_ENSEMBLE
        if (status == 0 && any_not_finite) status = 1;
#else
        if (status == 0 && (any_not_finite || isnan(ll) || isinf(ll))) status = 1;
        *ll_dst = (status != 0) ? -INFINITY : ll;
#endif
        if (status_dst) *status_dst = status;
        if (nacc_dst) *nacc_dst = n_acc;
        if (nrej_dst) *nrej_dst = n_rej;
    }
}

template <int LPC, int SOLVER>
#if SEPAIHRD_SIR_ENSEMBLE
int launch_lpc(const SirDevProblem& pb, const double* d_theta, int B, const SirOutputs& out, hipStream_t st, const SirEnsArgs& ens) {
    constexpr int CPW = WAVE / LPC;
    const unsigned blocks = (unsigned)(((long long)B + CPW - 1) / CPW);
    hipLaunchKernelGGL((sepaihrd_sir_eval_kernel<LPC, SOLVER, SEPAIHRD_ARITH_FMA>), dim3(blocks), dim3(WAVE), sir_rows_in_lds(LPC, SOLVER) ? (LPC * WAVE + WAVE) * sizeof(double) : 0, st, pb, d_theta, B, out, ens);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
#else
int launch_lpc(const SirDevProblem& pb, const double* d_theta, int B, const SirOutputs& out, hipStream_t st) {
    constexpr int CPW = WAVE / LPC;
    const unsigned blocks = (unsigned)(((long long)B + CPW - 1) / CPW);
    hipLaunchKernelGGL((sepaihrd_sir_eval_kernel<LPC, SOLVER, SEPAIHRD_ARITH_FMA>), dim3(blocks), dim3(WAVE), sir_rows_in_lds(LPC, SOLVER) ? (LPC * WAVE + WAVE) * sizeof(double) : 0, st, pb, d_theta, B, out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
#endif

#if SEPAIHRD_SIR_ENSEMBLE
template <int SOLVER>
int launch_solver(const SirDevProblem& pb, const double* d_theta, int B, const SirOutputs& out, hipStream_t st, const SirEnsArgs& ens) {
    switch (pb.lpc) {
        case 1: return launch_lpc<1, SOLVER>(pb, d_theta, B, out, st, ens);
        case 2: return launch_lpc<2, SOLVER>(pb, d_theta, B, out, st, ens);
        case 4: return launch_lpc<4, SOLVER>(pb, d_theta, B, out, st, ens);
        case 8: return launch_lpc<8, SOLVER>(pb, d_theta, B, out, st, ens);
        case 16: return launch_lpc<16, SOLVER>(pb, d_theta, B, out, st, ens);
        case 32: return launch_lpc<32, SOLVER>(pb, d_theta, B, out, st, ens);
        case 64: return launch_lpc<64, SOLVER>(pb, d_theta, B, out, st, ens);
        default: return -4;
    }
}
#else
template <int SOLVER>
int launch_solver(const SirDevProblem& pb, const double* d_theta, int B, const SirOutputs& out, hipStream_t st) {
    switch (pb.lpc) {
        case 1: return launch_lpc<1, SOLVER>(pb, d_theta, B, out, st);
        case 2: return launch_lpc<2, SOLVER>(pb, d_theta, B, out, st);
        case 4: return launch_lpc<4, SOLVER>(pb, d_theta, B, out, st);
        case 8: return launch_lpc<8, SOLVER>(pb, d_theta, B, out, st);
        case 16: return launch_lpc<16, SOLVER>(pb, d_theta, B, out, st);
        case 32: return launch_lpc<32, SOLVER>(pb, d_theta, B, out, st);
        case 64: return launch_lpc<64, SOLVER>(pb, d_theta, B, out, st);
        default: return -4;
    }
}
#endif

}  // namespace

#if SEPAIHRD_SIR_ENSEMBLE
#if SEPAIHRD_ARITH_FMA
int launch_sir_ens_fma(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, const SirEnsArgs& ens, void* stream) {
#else
int launch_sir_ens_strict(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, const SirEnsArgs& ens, void* stream) {
#endif
    if (B <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (solver) {
        case 0: return launch_solver<0>(pb, d_theta, B, out, st, ens);
        case 1: return launch_solver<1>(pb, d_theta, B, out, st, ens);
        case 2: return launch_solver<2>(pb, d_theta, B, out, st, ens);
        default: return -4;
    }
}
#else
#if SEPAIHRD_ARITH_FMA
int launch_sir_eval_fma(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, void* stream) {
#else
int launch_sir_eval_strict(const SirDevProblem& pb, int solver, const double* d_theta, int B, const SirOutputs& out, void* stream) {
#endif
    if (B <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (solver) {
        case 0: return launch_solver<0>(pb, d_theta, B, out, st);
        case 1: return launch_solver<1>(pb, d_theta, B, out, st);
        case 2: return launch_solver<2>(pb, d_theta, B, out, st);
        default: return -4;
    }
}
#endif

}  // namespace sepaihrd
