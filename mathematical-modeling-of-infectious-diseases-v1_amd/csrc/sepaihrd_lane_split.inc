// csrc/sepaihrd_lane_split.inc -- included by sepaihrd_kernels.hip (both arithmetic builds, inside its namespace).
//
// Small-batch form of the evaluation kernel for the 4-age model: SIXTEEN lanes per chain instead of four.
// Why: a lone wave issues one VALU instruction per ~4.8 cycles whatever it is (tools/ubench/issue_rate.hip), and
// up to 4096 chains the 4-lane mapping occupies at most 256 of the 1024 SIMDs with one wave each -- the step time
// is (instructions per RK attempt per lane) x 4.8 cycles and three quarters of the chip idle.  Here the 11
// compartments of an age class are spread over the four lanes of a quad, so a lane carries 3 of them: the stage
// sums, the error norm and the state update shrink ~3.5x per lane and four times as many waves share the work.
//
//   lane = 16 * chain_in_wave + 4 * age + cg        (a 16-lane DPP row = one chain, a quad = one age class)
//
//              slot 0     slot 1     slot 2 (quadratures: nothing reads them back)
//   cg 0       S          E          CumICU
//   cg 1       -          P          CumH
//   cg 2       A          I          R
//   cg 3       ICU        H          D
//
// Round 4: this assignment is the winner of an exhaustive search over all 39.9 M placements of the 11 compartments on the
// 12 places (tools/layout_search.py), scored by the instructions one wave issues per RK attempt: 25 per right-hand-side call
// against 28 for the rounds 1-3 layout ({S,E,D},{P,A,-},{I,H,CumH},{ICU,CumICU,R}); 20 assignments reach 25, this is the one of
// them in which every lane observes at most one of D, CumH, CumICU and all three sit in the same slot.  The disease progression
// E -> P -> I -> H runs along slot 1 from lane to lane, so the whole slot needs ONE rotated source.
//
// Every derivative of the model is linear in the compartments of its own age class except lambda_i S_i, so one
// instruction stream serves the four lanes of a quad with per-lane COEFFICIENT registers (zero where a term does
// not apply) and three quad rotations (Lx1 = slot 1 of the lane one to the LEFT, cg - 1; Nx1, Nx0 = slots 1, 0 of the NEXT
// lane, cg + 1):
//   d1 = cO1 x1 + cL1 Lx1 + W                        (W = lambda_i S_i in the cg-0 lanes, an exact 0 elsewhere: the
//   d0 = cO0 x0 + cX0 x1 + cL0 Lx1 - W                 contact row of a lane without an S is zero)
//   d2 = a1 x1 + a2 Nx1 + a3 Lx1 + a4 x0 + a5 Nx0
// e.g. lane cg 2: d1 = (gamma_p - p gamma_p) P - (gamma_I + h + d_comm) I with P = Lx1; d2 = gamma_I I + gamma_H H +
// gamma_A A + gamma_ICU ICU with H = Nx1, A = x0, ICU = Nx0; lane cg 3: d2 = d_H H + d_comm I + d_ICU ICU with I = Lx1.
// The infectious pressure P + A + theta I of an age class forms in its cg-2 lane (P = Lx1, A = x0, I = x1) and
// reaches the whole chain by row_newbcast from lanes 2, 6, 10, 14.
//
// Arithmetic: in BOTH builds each derivative is the SAME sequence of roundings as the 4-lane kernel's RHS of that
// build (tolerance mode: explicit fma() in both kernels; strict: the reference's expression tree per compartment,
// see rhs_quad below; the zero-coefficient terms add an exact 0), the stage sums and the error norm are per element:
// a chain's log-likelihood and step counts are bit-identical whichever of the two kernels ran it
// (tests/test_gpu_parity.py).  The formulas in this header comment are the tolerance-mode ones.
// Everything around the RHS (integrate_times bookkeeping, controller, schedule cache, observer) is the 4-lane
// kernel's code with 3 slots instead of 11; the likelihood passes and their workspace layout are shared.

constexpr int QUAD_LANES = 16;                 // lanes per chain
constexpr int QUAD_CPW = WAVE / QUAD_LANES;    // chains per wave
constexpr int QUAD_SLOTS = 3;

template <int CTRL>
__device__ __forceinline__ double quad_rot(double v) { return dpp_move<CTRL>(v); }
constexpr int QROT_LEFT = 0x93;  // quad_perm:[3,0,1,2]: lane cg reads lane cg - 1
constexpr int QROT_NEXT = 0x39;  // quad_perm:[1,2,3,0]: lane cg reads lane cg + 1

// Per-lane conditions of the time loop as 64-bit lane masks in scalar registers.  A comparison's result IS such a mask
// (v_cmp writes an SGPR pair); taken as one (ballot of the bare comparison), combined with scalar and / or / andn2 and
// tested with s_cmp, a wave-level question ("does any active chain ...?") costs no vector instruction -- `__ballot(a
// && b) != 0` made the compiler materialise a 0 / 1 vector and compare it again, two issue slots of a lone wave per
// question, five questions per RK attempt.  lane_of() hands a mask back to the vector unit as a select condition.
// Phase pads of the strict build's RK body (DESIGN_HISTORY.md, "instruction fetch"): one 4-byte s_nop behind stage i when bit i
// of SEPAIHRD_STRICT_STAGE_PADS is set.  A lone wave is fed ~1.9 bytes of instructions per cycle and a run of 8-byte encodings
// that starts 4 bytes off an 8-byte boundary issues every 5.2 cycles instead of 4.2-4.3; the body is almost purely such
// encodings and each 4-byte one in it flips the phase of what follows.  Round 3 chose the masks on the plain compile; since the
// strict build goes through csrc/phase_pass.py too, the pass sets the phase and the pads only cost issue slots: for the
// round-4 layout tools/phase_pad_search.py (compile -> pass -> assembled addresses) finds NO pad best for both solvers
// (0 of 462 / 432 eight-byte encodings off phase inside runs either way).  The knobs stay for placement experiments.
#ifndef SEPAIHRD_STRICT_STAGE_PADS
#define SEPAIHRD_STRICT_STAGE_PADS 0
#endif
#define SEP_STAGE_PAD(i, v) do { if ((SEPAIHRD_STRICT_STAGE_PADS >> (i)) & 1) asm volatile("s_nop 0" : "+v"(v)); } while (0)  // tied to the stage's first derivative: it stays where it is written
#ifndef SEPAIHRD_STRICT_HEAD_PADS_CK
#define SEPAIHRD_STRICT_HEAD_PADS_CK 0
#endif
#ifndef SEPAIHRD_STRICT_STAGE_PADS_CK
#define SEPAIHRD_STRICT_STAGE_PADS_CK 0
#endif
#define SEP_STAGE_PAD_CK(i, v) do { if ((SEPAIHRD_STRICT_STAGE_PADS_CK >> (i)) & 1) asm volatile("s_nop 0" : "+v"(v)); } while (0)
#define SEP_PHASE_PAD(n) do { if ((n) >= 1) asm volatile("s_nop 0"); if ((n) >= 2) asm volatile("s_nop 0"); if ((n) >= 3) asm volatile("s_nop 0"); } while (0)
using lanemask = unsigned long long;
__device__ __forceinline__ lanemask lanes_where(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool lane_of(lanemask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// min / max of two numbers neither of which is a NaN, without the canonicalising v_max_f64 x, x, x the compiler puts in
// front of fmin / fmax of a value it cannot prove quiet (a select result, a loop-carried step size)
__device__ __forceinline__ double min_plain(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

#if SEPAIHRD_ARITH_FMA
struct QuadModel {
    double theta_inf, m[4];  // m = 0 in the lanes that hold no S (cg != 0): their lambda and flow_SE are exact zeros
    double cO1, cL1;                  // slot 1: E, P, I, H
    double cO0, cX0, cL0;             // slot 0: S, -, A, ICU
    double a1, a2, a3, a4, a5;        // slot 2: CumICU, CumH, R, D
};

// The contact sum of one right-hand-side call as ONE fixed instruction sequence: the pressure (cg-2 lanes: P + A + theta I;
// meaningless, finite and unused in the other lanes; h_infec / N rides in q.m), then lambda_i = sum_j m_ij pressure_j, j ascending,
// one v_fmac_f64_dpp per term; fma(m_0, p_0, +0.0) = round(m_0 p_0) is the 4-lane kernel's first term.  The first DPP read of the
// pressure needs two wait states behind its VALU write.  They hold instructions the call needs anyway -- the accumulator's zero
// and the first half of the rotation Nx1 of slot 1 that only dx[2] reads (its second half goes between the first two terms, where
// the compiler put it too) -- instead of an s_nop (an issue slot of a lone wave like any other); a call whose dx[2] nobody
// reads (WANT2 = false: the second stage's) puts the zero and an fma of the caller's there: fill = fma(fa, fb, fc), any
// product-sum the caller needs next that does not depend on this call (the first term of the next stage's sum).
// x[1] itself was written at least three instructions earlier: Lx1's two moves and the addition separate it from this block.
template <bool WANT2>
__device__ __forceinline__ void contact_sum(const QuadModel& q, const double x1, const double lx1_plus_x0, double& lambda, double& Nx1,
                                            double& fill, const double fa, const double fb, const double fc) {
    double pressure = lx1_plus_x0;  // v_fmac: fma(theta, x1, Lx1 + x0)
    if constexpr (WANT2) {
        int lo, hi;
        asm("v_fmac_f64_e32 %0, %4, %5\n\t"
            "v_mov_b64_e32 %1, 0\n\t"
            "v_mov_b32_dpp %2, %6 quad_perm:[1,2,3,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f64_dpp %1, %0, %8 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
            "v_mov_b32_dpp %3, %7 quad_perm:[1,2,3,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f64_dpp %1, %0, %9 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %1, %0, %10 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %1, %0, %11 row_newbcast:14 row_mask:0xf bank_mask:0xf"
            : "+v"(pressure), "=&v"(lambda), "=&v"(lo), "=&v"(hi)
            : "v"(q.theta_inf), "v"(x1), "v"(__double2loint(x1)), "v"(__double2hiint(x1)), "v"(q.m[0]), "v"(q.m[1]), "v"(q.m[2]), "v"(q.m[3]));
        Nx1 = __hiloint2double(hi, lo);
    } else {
        asm("v_fmac_f64_e32 %0, %3, %4\n\t"
            "v_mov_b64_e32 %1, 0\n\t"
            "v_fma_f64 %2, %9, %10, %11\n\t"
            "v_fmac_f64_dpp %1, %0, %5 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %1, %0, %6 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %1, %0, %7 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %1, %0, %8 row_newbcast:14 row_mask:0xf bank_mask:0xf"
            : "+v"(pressure), "=&v"(lambda), "=&v"(fill)
            : "v"(q.theta_inf), "v"(x1), "v"(q.m[0]), "v"(q.m[1]), "v"(q.m[2]), "v"(q.m[3]), "v"(fa), "v"(fb), "v"(fc));
        Nx1 = 0.0;
    }
}

// The body of both forms below.  WANT2 = false: dx[2] comes back as 0 and fill = fma(fa, fb, fc) is formed on the way.
template <bool WANT2>
__device__ __forceinline__ void rhs_quad_body(const QuadModel& q, const double (&x)[QUAD_SLOTS], double (&dx)[QUAD_SLOTS],
                                              double beta_eff, double& fill, const double fa, const double fb, const double fc) {
    const double Lx1 = quad_rot<QROT_LEFT>(x[1]);
    const double Nx0 = quad_rot<QROT_NEXT>(x[0]);
    double lambda, Nx1;
    contact_sum<WANT2>(q, x[1], Lx1 + x[0], lambda, Nx1, fill, fa, fb, fc);
    lambda *= beta_eff;
    const double lambda_val = (0.0 < lambda) ? lambda : 0.0;
    const double W = lambda_val * x[0];  // lambda_i S_i in the cg-0 lanes; exactly 0 elsewhere (their contact row is zero)
    // explicit association (zero-coefficient terms add an exact 0): per compartment this is the 4-lane kernel's
    // tolerance-mode expression, e.g. dI = fma(-(gamma_I + h + d_comm), I, (gamma_p - p gamma_p) P),
    // dR = fma(g_ICU, ICU, fma(g_A, A, fma(g_H, H, g_I I))), dD = fma(d_ICU, ICU, fma(d_comm, I, d_H H))
    dx[1] = fma(q.cO1, x[1], fma(q.cL1, Lx1, W));
    dx[0] = fma(q.cO0, x[0], fma(q.cX0, x[1], fma(q.cL0, Lx1, -W)));
    if constexpr (WANT2) dx[2] = fma(q.a5, Nx0, fma(q.a4, x[0], fma(q.a3, Lx1, fma(q.a2, Nx1, q.a1 * x[1]))));
    else dx[2] = 0.0;
}
// the right-hand side
__device__ __forceinline__ void rhs_quad(const QuadModel& q, const double (&x)[QUAD_SLOTS], double (&dx)[QUAD_SLOTS], double beta_eff) {
    double unused = 0.0;
    rhs_quad_body<true>(q, x, dx, beta_eff, unused, 0.0, 0.0, 0.0);
}
// the right-hand side of a call whose dx[2] the caller never reads (it comes back as 0); returns fma(fa, fb, fc), formed inside
// the contact sum's hazard window: every argument is required, there is no form of this call without the fill
__device__ __forceinline__ double rhs_quad_slots01_fill(const QuadModel& q, const double (&x)[QUAD_SLOTS], double (&dx)[QUAD_SLOTS],
                                                        double beta_eff, const double fa, const double fb, const double fc) {
    double fill;
    rhs_quad_body<false>(q, x, dx, beta_eff, fill, fa, fb, fc);
    return fill;
}

// acc += (cur * coefficient IDX of the chain's row) * k for the terms after the first of ONE stage sum, all slots in a single
// fixed sequence: slot 1 first -- its quad rotation is what the right-hand side behind the sum starts with, and the other slots'
// terms separate its last write from that DPP read -- then slot 0, then (SL = 3) slot 2.  Per slot the terms in the order
// stage_term adds them one by one: the same fmas on the same operands.  One asm statement per sum, not one per term: the
// compiler counts an asm statement as no wait state at all and pads between two of them that touch the same register.
#define SEP_QLINE(t, s) "v_fmac_f64_dpp %[a" #s "], %[v" #t "], %[w" #t #s "] row_newbcast:%[n" #t "] row_mask:0xf bank_mask:0xf\n\t"
#define SEP_QTERM2(t) SEP_QLINE(t, 1) SEP_QLINE(t, 0)
#define SEP_QTERM3(t) SEP_QLINE(t, 1) SEP_QLINE(t, 0) SEP_QLINE(t, 2)
#define SEP_QIN2(t, IDX, k) [v##t] "v"((IDX) < 16 ? vecA : vecB), [n##t] "n"((IDX) & 15), [w##t##1] "v"(k[1]), [w##t##0] "v"(k[0])
#define SEP_QIN3(t, IDX, k) SEP_QIN2(t, IDX, k), [w##t##2] "v"(k[2])
#define SEP_QACC2(acc) [a1] "+v"(acc[1]), [a0] "+v"(acc[0])
#define SEP_QACC3(acc) SEP_QACC2(acc), [a2] "+v"(acc[2])

// The RK stages of one attempt of the 16-lane form: the stages of rk_stages_row_coef (sepaihrd_kernels.hip; a change to a
// tableau's stage structure there has to be made here too) for three values per lane, with
// the leading factor of every sum taken from vector B (lead<>: fl(cur * c) formed in lane IDX is the product every lane used
// to form from a 64-bit literal -- the same bits, and eight literals, two scalar registers each, leave a kernel that sits at the
// scalar-register limit), each sum's later terms as one sequence (above), and without the stage values nobody reads: slot 2
// of a lane holds output quadratures that no right-hand side reads, so xt[2] is never formed, and k2 has no weight in the
// solution or the error estimate of either tableau, so k2[2] is not either.
template <int IDX>
__device__ __forceinline__ double lead(double vecB) { return dpp_bcast_row<IDX, 0xf, IDX, 0x0>(vecB); }

template <int SOLVER>
__device__ __forceinline__ void rk_stages_quad(const QuadModel& q, const double vecA, const double vecB, const double (&x)[QUAD_SLOTS],
                                               double (&k1)[QUAD_SLOTS], double (&k2)[QUAD_SLOTS], double (&k3)[QUAD_SLOTS],
                                               double (&k4)[QUAD_SLOTS], double (&k5)[QUAD_SLOTS], double (&k6)[QUAD_SLOTS],
                                               double (&k7)[QUAD_SLOTS], double (&xnew)[QUAD_SLOTS], double (&xerr)[QUAD_SLOTS],
                                               const double (&bks)[7]) {
    double xt[QUAD_SLOTS];
    xt[2] = 0.0;
    auto first_term = [&](double (&acc)[QUAD_SLOTS], double f1, int slots) {
        acc[0] = fma(f1, k1[0], x[0]);
        acc[1] = fma(f1, k1[1], x[1]);
        if (slots == 3) acc[2] = fma(f1, k1[2], x[2]);
    };
    if (SOLVER == 0) {
        first_term(xt, lead<QL_STAGE2>(vecB), 2);
        {   // the third stage's first term of slot 1 rides in the second stage's contact sum
            const double f1 = lead<QL_STAGE3>(vecB);
            const double xt1 = rhs_quad_slots01_fill(q, xt, k2, bks[1], f1, k1[1], x[1]);
            xt[0] = fma(f1, k1[0], x[0]);
            xt[1] = xt1;
        }
        asm(SEP_QTERM2(1) : SEP_QACC2(xt) : SEP_QIN2(1, QD_B32, k2));
        rhs_quad(q, xt, k3, bks[2]);
        first_term(xt, lead<QL_STAGE4>(vecB), 2);
        asm(SEP_QTERM2(1) SEP_QTERM2(2) : SEP_QACC2(xt) : SEP_QIN2(1, QD_B42, k2), SEP_QIN2(2, QD_B43, k3));
        rhs_quad(q, xt, k4, bks[3]);
        first_term(xt, lead<QL_STAGE5>(vecB), 2);
        asm(SEP_QTERM2(1) SEP_QTERM2(2) SEP_QTERM2(3) : SEP_QACC2(xt) : SEP_QIN2(1, QD_B52, k2), SEP_QIN2(2, QD_B53, k3), SEP_QIN2(3, QD_B54, k4));
        rhs_quad(q, xt, k5, bks[4]);
        first_term(xt, lead<QL_STAGE6>(vecB), 2);
        asm(SEP_QTERM2(1) SEP_QTERM2(2) SEP_QTERM2(3) SEP_QTERM2(4)
            : SEP_QACC2(xt) : SEP_QIN2(1, QD_B62, k2), SEP_QIN2(2, QD_B63, k3), SEP_QIN2(3, QD_B64, k4), SEP_QIN2(4, QD_B65, k5));
        rhs_quad(q, xt, k6, bks[5]);
        first_term(xnew, lead<QL_NEW>(vecB), 3);
        asm(SEP_QTERM3(1) SEP_QTERM3(2) SEP_QTERM3(3) SEP_QTERM3(4)
            : SEP_QACC3(xnew) : SEP_QIN3(1, QD_C3, k3), SEP_QIN3(2, QD_C4, k4), SEP_QIN3(3, QD_C5, k5), SEP_QIN3(4, QD_C6, k6));
        rhs_quad(q, xnew, k7, bks[6]);
        // e1 k1 + e3 k3 + ...: the second product rounded, the first fused, as in rk_stages_row_coef
        const double e1 = lead<QL_ERR1>(vecB), e3 = lead<QL_ERR3>(vecB);
        SEP_UNROLL for (int c = 0; c < QUAD_SLOTS; ++c) xerr[c] = fma(e1, k1[c], e3 * k3[c]);
        asm(SEP_QTERM3(1) SEP_QTERM3(2) SEP_QTERM3(3) SEP_QTERM3(4)
            : SEP_QACC3(xerr) : SEP_QIN3(1, QD_DC4, k4), SEP_QIN3(2, QD_DC5, k5), SEP_QIN3(3, QD_DC6, k6), SEP_QIN3(4, QD_DC7, k7));
    } else {
        rhs_quad(q, x, k1, bks[0]);
        first_term(xt, lead<QL_STAGE2>(vecB), 2);
        {   // the third stage's first term of slot 1 rides in the second stage's contact sum
            const double f1 = lead<QL_STAGE3>(vecB);
            const double xt1 = rhs_quad_slots01_fill(q, xt, k2, bks[1], f1, k1[1], x[1]);
            xt[0] = fma(f1, k1[0], x[0]);
            xt[1] = xt1;
        }
        asm(SEP_QTERM2(1) : SEP_QACC2(xt) : SEP_QIN2(1, QK_A32, k2));
        rhs_quad(q, xt, k3, bks[2]);
        first_term(xt, lead<QL_STAGE4>(vecB), 2);
        asm(SEP_QTERM2(1) SEP_QTERM2(2) : SEP_QACC2(xt) : SEP_QIN2(1, QK_A42, k2), SEP_QIN2(2, QK_A43, k3));
        rhs_quad(q, xt, k4, bks[3]);
        first_term(xt, lead<QL_STAGE5>(vecB), 2);
        asm(SEP_QTERM2(1) SEP_QTERM2(2) SEP_QTERM2(3) : SEP_QACC2(xt) : SEP_QIN2(1, QK_A52, k2), SEP_QIN2(2, QK_A53, k3), SEP_QIN2(3, QK_A54, k4));
        rhs_quad(q, xt, k5, bks[4]);
        first_term(xt, lead<QL_STAGE6>(vecB), 2);
        asm(SEP_QTERM2(1) SEP_QTERM2(2) SEP_QTERM2(3) SEP_QTERM2(4)
            : SEP_QACC2(xt) : SEP_QIN2(1, QK_A62, k2), SEP_QIN2(2, QK_A63, k3), SEP_QIN2(3, QK_A64, k4), SEP_QIN2(4, QK_A65, k5));
        rhs_quad(q, xt, k6, bks[5]);
        first_term(xnew, lead<QL_NEW>(vecB), 3);
        asm(SEP_QTERM3(1) SEP_QTERM3(2) SEP_QTERM3(3) : SEP_QACC3(xnew) : SEP_QIN3(1, QK_B3, k3), SEP_QIN3(2, QK_B4, k4), SEP_QIN3(3, QK_B6, k6));
        // here the FIRST product is rounded and the second fused, as in rk_stages_row_coef
        const double e1 = lead<QL_ERR1>(vecB), e3 = lead<QL_ERR3>(vecB);
        SEP_UNROLL for (int c = 0; c < QUAD_SLOTS; ++c) xerr[c] = fma(e3, k3[c], e1 * k1[c]);
        asm(SEP_QTERM3(1) SEP_QTERM3(2) SEP_QTERM3(3) : SEP_QACC3(xerr) : SEP_QIN3(1, QK_DB4, k4), SEP_QIN3(2, QK_DB5, k5), SEP_QIN3(3, QK_DB6, k6));
    }
}

#else
// Strict arithmetic (no contraction): every compartment's derivative is the reference's own expression tree -- the
// same products and the same additions in the same order as the 4-lane kernel's strict RHS -- embedded in one
// template per slot whose unused terms are exact zeros (0 * finite = 0, x + 0 = x, x - 0 = x, 1 * x = x):
//   slot 1   d = ((W + t) - u3 t) - ((v1 x1 + v2 x1) + v3 x1),  t = u2 Lx1
//            e.g. I (cg 2): (gamma_p P - p (gamma_p P)) - ((gamma_I I + h I) + d_comm I)   = flow_PI - I_out
//                 H (cg 3): h I - ((gamma_H H + d_H H) + icu H)                            = flow_IH - H_out
//                 E (cg 0): W - sigma E                                                    = flow_SE - flow_EP
//   slot 0   d = ((u6 t5 + u7 x1) - w1 x0) - W,  t5 = u5 Lx1
//            e.g. A (cg 2): p (gamma_p P) - gamma_A A;  ICU (cg 3): icu H - (gamma_ICU + d_ICU) ICU;  S (cg 0): -W
//   slot 2   d = ((((q1 x0 + q2 x1) + q3 Nx1) + q4 Nx0) + q5 x0) + q6 Lx1
//            e.g. R (cg 2): ((gamma_A A + gamma_I I) + gamma_H H) + gamma_ICU ICU;  D (cg 3): (d_H H + d_ICU ICU) + d_comm I
//            (the reference adds A before I in dR and H before ICU in dD: x0 enters twice so that both orders embed)
struct QuadModel {
    double theta_inf, h_infec, inv_N, a_i, m[4];
    double u2, u3, v1, v2, v3;
    double u5, u6, u7, w1;
    double q1, q2, q3, q4, q5, q6;
};

__device__ __forceinline__ void rhs_quad(const QuadModel& q, const double (&x)[QUAD_SLOTS], double (&dx)[QUAD_SLOTS],
                                         double beta_eff) {
    const double Lx1 = quad_rot<QROT_LEFT>(x[1]);
    const double Nx1 = quad_rot<QROT_NEXT>(x[1]), Nx0 = quad_rot<QROT_NEXT>(x[0]);
    // cg-2 lanes: pi_j = (P + A + theta I) h_infec (1/N), AgeSEPAIHRDModel.cpp:153-157
    const double total_inf = Lx1 + x[0] + q.theta_inf * x[1];
    const double pressure = total_inf * q.h_infec * q.inv_N;
    // lambda_i = 0.0 + M(i,0) pi_0 + ..., j ascending; each value arrives with one v_mov_b64_dpp row_newbcast
    double lambda = q.m[0] * dpp_bcast_row<2, 0xf, 2, 0x0>(pressure);
    lambda += q.m[1] * dpp_bcast_row<6, 0xf, 6, 0x0>(pressure);
    lambda += q.m[2] * dpp_bcast_row<10, 0xf, 10, 0x0>(pressure);
    lambda += q.m[3] * dpp_bcast_row<14, 0xf, 14, 0x0>(pressure);
    lambda *= beta_eff * q.a_i;
    const double lambda_val = (0.0 < lambda) ? lambda : 0.0;
    const double W = lambda_val * x[0];  // flow_SE in the cg-0 lanes; exactly 0 elsewhere (their contact row is zero)
    {
        const double t = q.u2 * Lx1;
        const double flow_in = (W + t) - q.u3 * t;
        const double out = q.v1 * x[1] + q.v2 * x[1] + q.v3 * x[1];
        dx[1] = flow_in - out;
    }
    {
        const double t5 = q.u5 * Lx1;
        const double flow_in = q.u6 * t5 + q.u7 * x[1];
        dx[0] = (flow_in - q.w1 * x[0]) - W;
    }
    dx[2] = q.q1 * x[0] + q.q2 * x[1] + q.q3 * Nx1 + q.q4 * Nx0 + q.q5 * x[0] + q.q6 * Lx1;
}

#endif

// compartment held by (cg, slot); -1 = none: {S, E, CumICU}, {-, P, CumH}, {A, I, R}, {ICU, H, D}.  Arithmetic, not a
// table: a table lookup is a global load, and ANY load inside the time loop makes the compiler wait for vmcnt(0) at
// the loop head -- which on gfx9 also waits for the observer's store of the previous output (stores share the
// counter): ~500 cycles per output of a lone wave.
__device__ __forceinline__ int quad_comp(int cg, int slot) {
    if (slot == 0) return cg == 0 ? 0 : (cg == 1 ? -1 : (cg == 2 ? 3 : 6));
    if (slot == 1) return cg == 0 ? 1 : (cg == 1 ? 2 : (cg == 2 ? 4 : 5));
    return cg == 0 ? 10 : (cg == 1 ? 9 : (cg == 2 ? 7 : 8));
}

// ---------------------------------------------------------------------------------------------------------------
// FUSED form: the likelihood rides on a second wave of the same SIMD.
//
// A lone integrator wave leaves ~10-20 % of its SIMD's issue slots empty (5.3 cycles per instruction against the
// 4.3 two waves sustain), and the separate likelihood pass costs 8 % of the step plus 158 MB of parked increments per
// 4096-chain launch.  Here a workgroup is EIGHT waves on the four SIMDs of one CU (the 256-register allocation lets a
// SIMD hold exactly two): four integrator waves of four chains each, and four consumer waves, one on each
// integrator's SIMD, that evaluate the Poisson terms of the outputs their integrator has passed.  An integrator hands
// each output's twelve increments per chain (3 streams x 4 ages) to its consumer through a ring in LDS; the consumer
// adds the terms in the reference's order (ages ascending within a day, days ascending per stream) with the same
// log_pos, so the log-likelihood has the bits of the separate pass.  No workspace, no HBM traffic beyond theta in and
// the results out.
//
// Pairing: waves w and w + 4 of a workgroup share a SIMD on this hardware (tools/ubench/wave_placement.hip); the
// kernel does not rely on it -- every wave reads its SIMD id (HW_REG_HW_ID) and the two waves of a SIMD split the
// roles; any other placement falls back to roles by wave index (same results, less overlap).
// Protocol per chain: produced = rows written (release), consumed = rows read (release), ring of QUAD_RING rows.
// Every wait is bounded (QUAD_SPIN_LIMIT polls, then status 4 / an early exit) so that no wave can hang the grid.
// ---------------------------------------------------------------------------------------------------------------
constexpr int QUAD_RING = 32;                       // output rows buffered per chain (a power of two)
constexpr int QUAD_BURST = 12;                      // rows the consumer waits for before it starts reading
constexpr int QUAD_UNITS = 4;                       // integrator / consumer pairs per workgroup
constexpr int QUAD_ROW_DOUBLES = QUAD_CPW * 12;     // one output row of a unit: [chain][stream-source 3][age 4]
constexpr int QUAD_SPIN_LIMIT = 1 << 22;
constexpr size_t QUAD_FUSED_MAX_LDS = 144 * 1024;   // of the CU's 160 KiB; beyond it the separate pass is used
constexpr int QUAD_CTRL_INTS = 8 + QUAD_UNITS * (2 * QUAD_CPW + 1 + 3 * QUAD_CPW);  // simd ids | produced, consumed, done, final
constexpr int SEPAIHRD_STATUS_PIPELINE = 4;         // internal: the consumer hand-off timed out (never expected)

SEP_HOST_DEVICE inline size_t quad_unit_doubles(const DevProblem& pb) {
    return (size_t)LDS_REC_DOUBLES + (size_t)QUAD_CPW * (pb.nm + 1) + (size_t)QUAD_CPW * pb.P + (size_t)QUAD_RING * QUAD_ROW_DOUBLES;
}
inline size_t quad_fused_lds_bytes(const DevProblem& pb) {
    const size_t need = ((size_t)times_pad(pb) + pb.nm_pad + QUAD_UNITS * quad_unit_doubles(pb)) * sizeof(double) + QUAD_CTRL_INTS * sizeof(int);
    // never less than half a CU's LDS: ONE workgroup (4 integrator + 4 consumer waves, a pair per SIMD) per CU whatever the
    // register allocation of a future build allows -- the dispatcher pairs up what fits (see split_pays in sepaihrd_kernels.hip)
    constexpr size_t ONE_WORKGROUP_PER_CU = 82 * 1024;
    return need < ONE_WORKGROUP_PER_CU ? ONE_WORKGROUP_PER_CU : need;
}

struct QuadCtrl {  // views into the control words of one unit
    int* produced;  // [CPW] rows written
    int* consumed;  // [CPW] rows read
    int* done;      // [1]   the integrator has left its loop
    int* final_;    // [CPW][3] status, accepted, rejected
};
__device__ __forceinline__ QuadCtrl quad_ctrl(int* base, int unit) {
    int* u = base + 8 + unit * (2 * QUAD_CPW + 1 + 3 * QUAD_CPW);
    return QuadCtrl{u, u + QUAD_CPW, u + 2 * QUAD_CPW, u + 2 * QUAD_CPW + 1};
}
__device__ __forceinline__ int ld_acquire(const int* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_release(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Consumer wave of one unit: lane = 16 chain + 4 stream + age (stream 3 idles).
__device__ __forceinline__ void quad_ll_consumer(const DevProblem& pb, const EvalOutputs& out, const long long chain0, const int B,
                                              const double* ring, const QuadCtrl ctl) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int c = lane >> 4, stream = (lane >> 2) & 3, age = lane & 3;
    const int s_ = stream < 3 ? stream : 0;
    const int src = (s_ == 0) ? 1 : (s_ == 1) ? 2 : 0;  // ring rows hold D, CumH, CumICU; the streams are H, ICU, D
    const bool chain_valid = chain0 + c < B;
    const double* cell = ring + c * 12 + src * 4 + age;
    const double* rec = pb.grid + (size_t)age * 4 + s_;  // + 16 k: {obs_H, obs_ICU, obs_D, t_{k+1}} of (k, age)
    double acc = 0.0;
    int k = 0, spins = 0;
    bool finished = false;
    const double* obs_k = rec;                            // observation of row k: advanced, not re-derived
    while (true) {
        const int fin = ld_acquire(ctl.done);             // read BEFORE produced: done is stored after the last row
        const int avail = ld_acquire(ctl.produced + c);
        // Rows are taken in bursts (a poll costs a third of a row): wait until some chain has QUAD_BURST of them, or
        // the integrator is done; then every chain's lanes walk their own available rows without looking again.
        const bool burst = (avail - k >= QUAD_BURST) || fin != 0;
        if (__ballot(!finished && burst && k < avail) != 0ull) {
            int todo = finished ? 0 : avail - k;          // uniform within a chain's 16 lanes
            while (__ballot(todo > 0) != 0ull) {
                if (todo > 0) {  // a quad = one (chain, stream): uniform here, so the quad broadcasts below are safe
                    if (k >= pb.runup_offset) {
                        double inc = cell[(k & (QUAD_RING - 1)) * QUAD_ROW_DOUBLES];
                        inc = (inc < 0.0) ? 0.0 : inc;    // cwiseMax(0.0)
                        const double obs = *obs_k;
                        const double sim = inc + 1e-10;
                        const double v = obs * log_pos(sim) - sim;
                        const double tv = (obs >= 0.0 && isfinite(obs)) ? v : 0.0;
                        double r = group_bcast<4, 0>(tv);  // ages ascending: the reference's inner loop
                        r += group_bcast<4, 1>(tv);
                        r += group_bcast<4, 2>(tv);
                        r += group_bcast<4, 3>(tv);
                        acc += r;                          // days ascending: log_likelihood += row_sum
                    } else {
                        acc += 0.0;                        // outputs before t = 0: every term is 0
                    }
                    ++k;
                    obs_k += 16;
                    --todo;
                }
            }
            if (!finished && stream == 0 && age == 0) st_release(ctl.consumed + c, k);  // frees the rows for the producer
            spins = 0;
        } else {
            if (fin != 0) {
                // nothing available and the integrator is done: rows produced up to `avail` are all there will be
                if (!finished && k >= ld_acquire(ctl.produced + c)) finished = true;
            }
            if (__ballot(!finished) == 0ull) break;
            if (fin == 0) __builtin_amdgcn_s_sleep(96);   // ~6000 cycles: about one output interval of the integrator
            if (++spins > QUAD_SPIN_LIMIT) break;          // never expected: leave rather than hang the grid
        }
    }
    // total = (hosp + icu) + deaths; NaN / Inf -> lowest() (SEPAIHRDObjectiveFunction.cpp:222-227)
    const double h = dpp_bcast_row<0, 0xf, 0, 0x0>(acc), i = dpp_bcast_row<4, 0xf, 4, 0x0>(acc), d = dpp_bcast_row<8, 0xf, 8, 0x0>(acc);
    if (chain_valid && (lane & 15) == 0) {
        const long long chain = chain0 + c;
        int status = ctl.final_[3 * c + 0];
        if (spins > QUAD_SPIN_LIMIT && status == 0) status = SEPAIHRD_STATUS_PIPELINE;
        double total = (h + i) + d;
        const bool integ_ok = status == 0;
        if (status == 0 && (isnan(total) || isinf(total))) status = 1;
        if (status != 0) total = -DBL_MAX;
        out.loglik[chain] = total;
        if (out.status) out.status[chain] = status;
        if (out.n_accept) out.n_accept[chain] = ctl.final_[3 * c + 1];
        if (out.n_reject) out.n_reject[chain] = ctl.final_[3 * c + 2];
#ifndef SEPAIHRD_STAMPS
        if (out.ll_parts) {
            out.ll_parts[3 * chain + 0] = integ_ok ? h : 0.0;
            out.ll_parts[3 * chain + 1] = integ_ok ? i : 0.0;
            out.ll_parts[3 * chain + 2] = integ_ok ? d : 0.0;
        }
#endif
    }
}

// ARITH only tells the two builds' kernels apart in profiler output (same value as SEPAIHRD_ARITH_FMA)
#if !SEPAIHRD_ARITH_FMA
// Strict build: the step times EVERY tableau coefficient, one product per lane of the chain's 16-lane row (two v_mul_f64 per
// attempt), and each factor reaches the stage code as a row broadcast (v_mov_b64_dpp row_newbcast).  fl(cur * b) formed in
// lane l is the product the stage code used to form in every lane from a 64-bit literal: the same bits, but 26-30 literals
// (two scalar registers each) no longer compete for the scalar file -- the strict headline kernel spilled 62 scalar registers
// into vector lanes and paid ~100 v_readlane / v_writelane per attempt for it.
enum StrictCoefDopri5 { SD_B21 = 0, SD_B31, SD_B32, SD_B41, SD_B42, SD_B43, SD_B51, SD_B52, SD_B53, SD_B54, SD_B61, SD_B62, SD_B63, SD_B64,
                        SD_B65, SD_C1, SD_C3 /* vector B from here */, SD_C4, SD_C5, SD_C6, SD_DC1, SD_DC3, SD_DC4, SD_DC5, SD_DC6, SD_DC7 };
enum StrictCoefCashKarp { SK_A21 = 0, SK_A31, SK_A32, SK_A41, SK_A42, SK_A43, SK_A51, SK_A52, SK_A53, SK_A54, SK_A61, SK_A62, SK_A63, SK_A64,
                          SK_A65, SK_B1, SK_B3 /* vector B from here */, SK_B4, SK_B6, SK_DB1, SK_DB3, SK_DB4, SK_DB5, SK_DB6 };
__device__ const double STRICT_QUAD_COEF[2][2][16] = {
    {{dp::b21, dp::b31, dp::b32, dp::b41, dp::b42, dp::b43, dp::b51, dp::b52, dp::b53, dp::b54, dp::b61, dp::b62, dp::b63, dp::b64, dp::b65,
      dp::c1},
     {dp::c3, dp::c4, dp::c5, dp::c6, dp::dc1, dp::dc3, dp::dc4, dp::dc5, dp::dc6, dp::dc7, 0, 0, 0, 0, 0, 0}},
    {{ck::a21, ck::a31, ck::a32, ck::a41, ck::a42, ck::a43, ck::a51, ck::a52, ck::a53, ck::a54, ck::a61, ck::a62, ck::a63, ck::a64, ck::a65,
      ck::b1},
     {ck::b3, ck::b4, ck::b6, ck::db1, ck::db3, ck::db4, ck::db5, ck::db6, 0, 0, 0, 0, 0, 0, 0, 0}}};
// cur * coefficient IDX of the chain's row
template <int IDX>
__device__ __forceinline__ double strict_coef(double sA, double sB) {
    if constexpr (IDX < 16) return dpp_bcast_row<IDX, 0xf, IDX, 0x0>(sA);
    else return dpp_bcast_row<IDX - 16, 0xf, IDX - 16, 0x0>(sB);
}
#endif

// TRAJ = false: the build without the trajectory output (every evaluation but the parity / ensemble runs): its pointers, masks
// and the skip branch around its stores leave the loop -- the kernel sits at the scalar-register limit, and a branch costs
// a lone wave ~9 cycles even when it is not taken
template <int SOLVER, int ARITH, bool FUSED, bool TRAJ = true>
__global__ __launch_bounds__(FUSED ? 8 * WAVE : WAVE, 2) void sepaihrd_eval_quad_kernel(const DevProblem pb, const double* __restrict__ theta,
                                                                      const int B, const EvalOutputs out,
                                                                      const int cum_chains) {
    constexpr int LPC = 4, NS = QUAD_SLOTS, CPW = QUAD_CPW;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    // ---- roles and LDS carve
    int unit = 0;          // FUSED: which of the workgroup's four (integrator, consumer) pairs
    double* unit_base;     // per-wave (per-unit) region: scratch | bk | theta [| ring]
    double* lds_times;
    double* lds_mends;
    int* ctrl_words = nullptr;
    if constexpr (FUSED) {
        lds_times = lds;
        lds_mends = lds + times_pad(pb);
        double* units0 = lds_mends + pb.nm_pad;
        ctrl_words = reinterpret_cast<int*>(units0 + QUAD_UNITS * quad_unit_doubles(pb));
        const int wave = threadIdx.x / WAVE;
        const int simd = (int)__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4);  // HW_REG_HW_ID bits 5:4
        if (lane == 0) ctrl_words[wave] = simd;
        for (int k = threadIdx.x; k < QUAD_CTRL_INTS - 8; k += 8 * WAVE) ctrl_words[8 + k] = 0;
        for (int k = threadIdx.x; k < pb.nm_pad; k += 8 * WAVE) lds_mends[k] = pb.mends[k];
        for (int k = threadIdx.x; k < pb.T; k += 8 * WAVE) lds_times[k] = pb.times[k];
        stage_log_table(threadIdx.x, 8 * WAVE);  // for the consumer waves' Poisson terms
        __syncthreads();
        int rank = 0, per_simd[4] = {0, 0, 0, 0};
        for (int w = 0; w < 8; ++w) {
            const int sw = ctrl_words[w] & 3;
            per_simd[sw]++;
            if (w < wave && sw == simd) ++rank;
        }
        const bool paired = per_simd[0] == 2 && per_simd[1] == 2 && per_simd[2] == 2 && per_simd[3] == 2;
        const int role = paired ? rank : wave / QUAD_UNITS;   // 0 integrator, 1 consumer
        unit = paired ? simd : wave % QUAD_UNITS;
        unit_base = units0 + (size_t)unit * quad_unit_doubles(pb);
        if (role == 1) {
            __builtin_amdgcn_s_setprio(0);  // the integrator on this SIMD goes first whenever both are ready
            const double* ring = unit_base + LDS_REC_DOUBLES + CPW * (pb.nm + 1) + CPW * pb.P;
            quad_ll_consumer(pb, out, ((long long)blockIdx.x * QUAD_UNITS + unit) * CPW, B, ring, quad_ctrl(ctrl_words, unit));
            return;
        }
    } else {
        lds_times = lds;
        unit_base = lds + times_pad(pb);
        lds_mends = unit_base + LDS_REC_DOUBLES;   // kept where the single-wave layout had it
    }
    if constexpr (FUSED) __builtin_amdgcn_s_setprio(3);
    double* const lds_scratch = unit_base;  // [CPW][LPC][11] initial state exchange (prologue)
    double* const lds_bk = FUSED ? unit_base + LDS_REC_DOUBLES : lds_mends + pb.nm_pad;
    double* const lds_theta = lds_bk + CPW * (pb.nm + 1);
    double* const lds_ring = lds_theta + CPW * pb.P;  // FUSED only
    const QuadCtrl ctl = FUSED ? quad_ctrl(ctrl_words, unit) : QuadCtrl{nullptr, nullptr, nullptr, nullptr};
    // within one wave LDS operations complete in issue order: a fence for the compiler is all a hand-over between
    // lanes of the SAME wave needs; the single-wave form keeps its (free) workgroup barrier
    auto wave_sync = [&]() {
        if constexpr (FUSED) { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }
        else __syncthreads();
    };
    const int grp = lane / QUAD_LANES;
    const int age = (lane >> 2) & 3;
    const int cg = lane & 3;
    const long long chain0 = FUSED ? ((long long)blockIdx.x * QUAD_UNITS + unit) * CPW : (long long)blockIdx.x * CPW;
    const int chains_here = (B - chain0) < CPW ? (int)(B - chain0) : CPW;
    if constexpr (FUSED) {
        if (chains_here <= 0) {  // a whole unit beyond the end of the batch: tell the consumer and leave
            if (lane == 0) st_release(ctl.done, 1);
            return;
        }
    }
    const bool chain_valid = grp < chains_here;
    const int g = chain_valid ? grp : 0;  // lanes past the end of the batch shadow chain 0 of the wave and never store
    const long long chain = chain0 + g;
    const int P = pb.P;

    {
        const int total = chains_here * P;
        const double* src = theta + chain0 * P;
        for (int idx = lane; idx < total; idx += WAVE) {
            const int p = idx % P;
            lds_theta[idx] = constrain(src[idx], pb.lower[p], pb.upper[p], pb.has_bounds[p], pb.constraint_mode);
        }
    }
    if constexpr (!FUSED) {
        for (int k = lane; k < pb.nm_pad; k += WAVE) lds_mends[k] = pb.mends[k];
        for (int k = lane; k < pb.T; k += WAVE) lds_times[k] = pb.times[k];
    }
    wave_sync();
    const double* th = lds_theta + g * P;
    auto scalar_slot = [&](int slot) -> double {
        const int s = pb.src_scalar[slot];
        return s >= 0 ? th[s] : pb.base_scalar[slot];
    };
    auto vec_slot = [&](int field) -> double {
        const int s = pb.src_vec[field * LPC + age];
        return s >= 0 ? th[s] : pb.base_vec[field * LPC + age];
    };

    // ---- theta -> per-lane coefficients (tolerance mode: the 4-lane kernel's folds; strict: the raw fields)
    QuadModel q;
    const double Ni = pb.N[age];
    {
        const double sigma = scalar_slot(SS_SIGMA), gamma_p = scalar_slot(SS_GAMMA_P), gamma_A = scalar_slot(SS_GAMMA_A),
                     gamma_I = scalar_slot(SS_GAMMA_I), gamma_H = scalar_slot(SS_GAMMA_H),
                     gamma_ICU = scalar_slot(SS_GAMMA_ICU);
        const double a = vec_slot(VF_A), h_infec = vec_slot(VF_H_INFEC), p = vec_slot(VF_P), h = vec_slot(VF_H),
                     icu = vec_slot(VF_ICU), d_H = vec_slot(VF_D_H), d_ICU = vec_slot(VF_D_ICU),
                     d_comm = vec_slot(VF_D_COMM);
        const double inv_N = (Ni > 1e-9) ? (1.0 / Ni) : 0.0;
        q.theta_inf = scalar_slot(SS_THETA);
#if SEPAIHRD_ARITH_FMA
        // column j of the contact row carries age class j's h_infec / N, as in the 4-lane kernel
        const double c_inf = h_infec * inv_N;
        // (zero in the lanes without an S: lambda, and with it lambda S, is then an exact 0 there)
        q.m[0] = (cg == 0) ? a * pb.Mrow[age * LPC + 0] * dpp_bcast_row<0, 0xf, 0, 0x0>(c_inf) : 0.0;
        q.m[1] = (cg == 0) ? a * pb.Mrow[age * LPC + 1] * dpp_bcast_row<4, 0xf, 4, 0x0>(c_inf) : 0.0;
        q.m[2] = (cg == 0) ? a * pb.Mrow[age * LPC + 2] * dpp_bcast_row<8, 0xf, 8, 0x0>(c_inf) : 0.0;
        q.m[3] = (cg == 0) ? a * pb.Mrow[age * LPC + 3] * dpp_bcast_row<12, 0xf, 12, 0x0>(c_inf) : 0.0;
        const double pg = rounded_here(p * gamma_p);
        const double r_I = gamma_I + h + d_comm, r_H = gamma_H + d_H + icu, r_ICU = gamma_ICU + d_ICU;
        q.cO1 = (cg == 0) ? -sigma : (cg == 1 ? -gamma_p : (cg == 2 ? -r_I : -r_H));   // E, P, I, H: their own outflow
        q.cL1 = (cg == 1) ? sigma : (cg == 2 ? gamma_p - pg : (cg == 3 ? h : 0.0));     // inflow from the lane to the left: E, P, I
        q.cO0 = (cg == 2) ? -gamma_A : (cg == 3 ? -r_ICU : 0.0);                        // A, ICU
        q.cX0 = (cg == 3) ? icu : 0.0;                                                  // ICU <- H (own lane)
        q.cL0 = (cg == 2) ? pg : 0.0;                                                   // A <- P (lane to the left)
        q.a1 = (cg == 2) ? gamma_I : (cg == 3 ? d_H : 0.0);                             // R <- I, D <- H   (own slot 1)
        q.a2 = (cg == 1) ? h : (cg == 2 ? gamma_H : 0.0);                               // CumH <- I, R <- H (next lane's slot 1)
        q.a3 = (cg == 0) ? icu : (cg == 3 ? d_comm : 0.0);                              // CumICU <- H, D <- I (lane to the left)
        q.a4 = (cg == 2) ? gamma_A : (cg == 3 ? d_ICU : 0.0);                           // R <- A, D <- ICU (own slot 0)
        q.a5 = (cg == 2) ? gamma_ICU : 0.0;                                             // R <- ICU (next lane's slot 0)
#else
        q.h_infec = h_infec;
        q.inv_N = inv_N;
        q.a_i = a;
        SEP_UNROLL
        for (int j = 0; j < LPC; ++j) q.m[j] = (cg == 0) ? pb.Mrow[age * LPC + j] : 0.0;  // lambda = 0 where there is no S
        q.u2 = (cg == 1) ? sigma : (cg == 2 ? gamma_p : (cg == 3 ? h : 0.0));           // t = flow_EP | flow_P_out | flow_IH
        q.u3 = (cg == 2) ? p : 0.0;                                                     // flow_PI = t - p t
        q.v1 = (cg == 0) ? sigma : (cg == 1 ? gamma_p : (cg == 2 ? gamma_I : gamma_H));
        q.v2 = (cg == 2) ? h : (cg == 3 ? d_H : 0.0);
        q.v3 = (cg == 2) ? d_comm : (cg == 3 ? icu : 0.0);
        q.u5 = (cg == 2) ? gamma_p : 0.0;                                               // flow_P_out for flow_PA = p flow_P_out
        q.u6 = (cg == 2) ? p : 0.0;
        q.u7 = (cg == 3) ? icu : 0.0;                                                   // flow_H_ICU
        q.w1 = (cg == 2) ? gamma_A : (cg == 3 ? gamma_ICU + d_ICU : 0.0);
        q.q1 = (cg == 2) ? gamma_A : 0.0;                                               // R: A first ...
        q.q2 = (cg == 2) ? gamma_I : (cg == 3 ? d_H : 0.0);                             // ... then I;  D: H first
        q.q3 = (cg == 1) ? h : (cg == 2 ? gamma_H : 0.0);                               // CumH = h I;  R: + H
        q.q4 = (cg == 2) ? gamma_ICU : 0.0;                                             // R: + ICU
        q.q5 = (cg == 3) ? d_ICU : 0.0;                                                 // D: + ICU
        q.q6 = (cg == 0) ? icu : (cg == 3 ? d_comm : 0.0);                              // CumICU = icu H;  D: + I
#endif
    }

    Schedule sch;
    sch.me = lds_mends;
    {
        double* bkv = lds_bk + grp * (pb.nm + 1);
        for (int j = lane % QUAD_LANES; j <= pb.nm; j += QUAD_LANES) {
            const double beta = (pb.nb > 0) ? scalar_slot(SS_SCHEDULE0 + pb.seg_ib[j]) : scalar_slot(SS_BETA);
            const double kappa = scenario_kappa(pb, chain, pb.seg_ik[j], scalar_slot(SS_SCHEDULE0 + pb.nb + pb.seg_ik[j]));
            bkv[j] = beta * kappa;
        }
        sch.bkv = bkv;
    }

    int status = 0;
    if (pb.kappa_calibrated) {
        bool neg = false;
        for (int k = 1; k < pb.nk; ++k) neg |= (scalar_slot(SS_SCHEDULE0 + pb.nb + k) < 0.0);
        if (neg) status = 1;
    }
    if (!pb.obs_rows_match && pb.init_mode == 0) status = 1;

    // ---- initial state (SEPAIHRDObjectiveFunction.cpp:124-163): each lane prepares its slots, the sum over
    //      E..D runs in compartment order over an LDS copy of the age class
    double x[NS];
    SEP_UNROLL
    for (int s = 0; s < NS; ++s) {
        const int c = quad_comp(cg, s);
        x[s] = (c >= 0) ? pb.init_state[c * LPC + age] : 0.0;
    }
    if (pb.init_mode != 1) {
        const double runup_days = scalar_slot(SS_RUNUP_DAYS);
        const double seed_exposed = scalar_slot(SS_SEED_EXPOSED);
        const bool seeded = (pb.init_mode == 0 && runup_days > 0 && seed_exposed > 0);
        SEP_UNROLL
        for (int s = 0; s < NS; ++s) {
            const int c = quad_comp(cg, s);
            if (seeded) {
                if (c == 1) x[s] = seed_exposed * pb.age_fraction[age];
                else if (c >= 2) x[s] = 0.0;
            } else if (c >= 1 && c <= 8) {
                x[s] *= scalar_slot(SS_E0_MULT + (c - 1));
            }
        }
        double* cell = lds_scratch + (grp * LPC + age) * NUM_COMP;
        SEP_UNROLL
        for (int s = 0; s < NS; ++s) {
            const int c = quad_comp(cg, s);
            if (c >= 0) cell[c] = x[s];
        }
        wave_sync();
        double sum = 0;
        for (int c = 1; c < NUM_POP_COMP; ++c) sum += cell[c];
        if (group_any<QUAD_LANES>(sum > Ni || (pb.init_mode == 2 && sum < 0), lane)) status = 1;
        if (cg == 0) x[0] = Ni - sum;
    }
    wave_sync();

    int n_acc = 0, n_rej = 0;
    const int T = pb.T;

    // observer: the lane's own increment stream, always its slot 2 (D in cg 3, CumH in cg 1, CumICU in cg 0; cg 2 holds R: none)
    const int which = (cg == 3) ? 0 : (cg == 1 ? 1 : 2);  // cum rows are D, CumH, CumICU
    double* const cum_lane = FUSED ? nullptr : out.cum + cum_index(pb.T, (size_t)(chain0 + grp) * LPC + age, 0, which);
    const bool stores = chain_valid && cg != 2;
    auto obs_value = [&]() -> double { return x[2]; };
    double prev = obs_value();
    const int n_real = pb.n;
    double* cum_row = cum_lane;  // row of the next output: advanced per output instead of re-derived from k
    const size_t cum_step = CUM_ROW_DOUBLES;
    lanemask act = lanes_where(status == 0);  // the chains still integrating: loop control lives on the scalar unit
    int cons_seen = 0;  // FUSED: rows the consumer had read when last looked at (per chain, lanes of a chain agree)
    int* const my_produced = FUSED ? ctl.produced + grp : nullptr;
    const int* const my_consumed = FUSED ? ctl.consumed + grp : nullptr;
    double* const ring_cell = lds_ring + grp * 12 + which * 4 + age;
    const bool ring_writer = cg != 2;
    int ring_budget = 0;  // observer calls the wave may still make before any of its chains could reach a row the consumer has not read
    auto observe_store = [&](lanemask do_m, int k) {
        if constexpr (FUSED) {
            // back-pressure: row k may overwrite row k - QUAD_RING only after the consumer has read it.  The consumer
            // is a row or two behind, so the cached count almost always suffices (one LDS read per ~QUAD_RING rows).
            // The question is asked on the scalar unit.  A call writes at most one row per chain, so after
            // the consumers' counts were last read the wave may make min over its chains of (consumed + QUAD_RING - next row)
            // calls without looking again: a scalar decrement and one branch per call instead of a vector comparison handed
            // to the scalar unit and branched on (25 cycles of a lone wave, tools/ubench/frontend.hip).
            if (__builtin_expect(ring_budget <= 0, 0)) {
                int spins = 0;
                do {
                    cons_seen = ld_acquire(my_consumed);
                    if ((do_m & lanes_where(k >= cons_seen + QUAD_RING)) == 0ull) break;
                    __builtin_amdgcn_s_sleep(2);
                } while (++spins < QUAD_SPIN_LIMIT);
                const lanemask stuck = do_m & lanes_where(k >= cons_seen + QUAD_RING);
                if (stuck != 0ull) {
                    if (lane_of(stuck)) status = SEPAIHRD_STATUS_PIPELINE;
                    act &= ~stuck;
                    do_m &= ~stuck;
                }
                // k is the lane's next row whether it writes now or not; a chain that has left the loop writes nothing more
                const int slack = lane_of(act) ? cons_seen + QUAD_RING - k : QUAD_RING;
                const int s0 = __builtin_amdgcn_readlane(slack, 0), s1 = __builtin_amdgcn_readlane(slack, 16),
                          s2 = __builtin_amdgcn_readlane(slack, 32), s3 = __builtin_amdgcn_readlane(slack, 48);
                ring_budget = __builtin_amdgcn_readfirstlane(min(min(s0, s1), min(s2, s3)));  // kept in a scalar register: the call's test is s_cmp + branch
            }
            --ring_budget;
        }
        if (lane_of(do_m)) {
            const double v = obs_value();
            if constexpr (FUSED) {
                if (ring_writer) ring_cell[(k & (QUAD_RING - 1)) * QUAD_ROW_DOUBLES] = v - prev;
                if (cg == 0 && age == 0) st_release(my_produced, k + 1);  // after the row (release orders the wave's LDS writes)
            } else {
                if (stores) *cum_row = v - prev;
                cum_row += cum_step;
            }
            prev = v;
            if constexpr (TRAJ) {
            if (out.traj != nullptr && chain_valid && age < n_real) {
                double* tdst = out.traj + ((size_t)chain * pb.T + k) * (NUM_COMP * n_real) + age;
                SEP_UNROLL
                for (int s = 0; s < NS; ++s) {
                    const int c = quad_comp(cg, s);
                    if (c >= 0) tdst[c * n_real] = x[s];
                }
            }
            }
        }
    };

    int k_next = 1;
    double t = pb.times[0];
    double dt = pb.dt_hint;
    int fails = 0;
    int attempts = 0;  // the same for every lane: scalar
    double t_next = (T > 1) ? pb.times[1] : t;
    // the grid time after next, read one whole output interval ahead of its use: a lone wave would otherwise sit out
    // the LDS latency at every output (this form has the registers for it; the 4-lane integrator does not)
    double t_after = (T > 2) ? pb.times[2] : t_next;
    observe_store(act, 0);
    if (T <= 1) act = 0ull;

    sch.lo = INFINITY; sch.hi = -INFINITY; sch.bk = 0.0;
    double k1[NS];
    if (SOLVER == 0) {
        int c0, c1;
        segment_index2(sch, pb.nm_pad, t, t, c0, c1);
        rhs_quad(q, x, k1, sch.bkv[c0]);
    }
    const double eps_abs = pb.abs_tol, eps_rel = pb.rel_tol;
#if SEPAIHRD_ARITH_FMA
    const double coefA = QUAD_COEF[SOLVER][0][lane & 15], coefB = QUAD_COEF[SOLVER][1][lane & 15];
#else
    const double coefA = STRICT_QUAD_COEF[SOLVER][0][lane & 15], coefB = STRICT_QUAD_COEF[SOLVER][1][lane & 15];
#endif

#ifdef SEPAIHRD_STAMPS
    unsigned long long st0 = 0, st1 = 0, st2 = 0, st3 = 0, st4 = 0;
    unsigned long long acc_head = 0, acc_body = 0, acc_err = 0, acc_tail = 0;
#endif
    // One RK attempt of every chain of the wave: stages, error norm, step-size rule, accept / reject, observer.
    // bks: beta*kappa at the seven stage times.  Inlined at its two call sites (see the loop).
    auto attempt = [&](const double cur, const double vecA, const double vecB, const double (&bks)[7]) __attribute__((always_inline)) {
        const bool active = lane_of(act);
        (void)active;
        SEP_STAMP(st1);
        double k2[NS], k3[NS], k4[NS], k5[NS], k6[NS], k7[NS];
        double xnew[NS], xerr[NS];
#if SEPAIHRD_ARITH_FMA
        rk_stages_quad<SOLVER>(q, vecA, vecB, x, k1, k2, k3, k4, k5, k6, k7, xnew, xerr, bks);
#else
        double xt[NS];
        if (SOLVER == 0) {
            { const double f1 = strict_coef<SD_B21>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c) xt[c] = x[c] + f1 * k1[c];
              rhs_quad(q, xt, k2, bks[1]); }
            SEP_STAGE_PAD(0, k2[0]);
            { const double f1 = strict_coef<SD_B31>(vecA, vecB), f2 = strict_coef<SD_B32>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c];
              rhs_quad(q, xt, k3, bks[2]); }
            SEP_STAGE_PAD(1, k3[0]);
            { const double f1 = strict_coef<SD_B41>(vecA, vecB), f2 = strict_coef<SD_B42>(vecA, vecB), f3 = strict_coef<SD_B43>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c];
              rhs_quad(q, xt, k4, bks[3]); }
            SEP_STAGE_PAD(2, k4[0]);
            { const double f1 = strict_coef<SD_B51>(vecA, vecB), f2 = strict_coef<SD_B52>(vecA, vecB), f3 = strict_coef<SD_B53>(vecA, vecB), f4 = strict_coef<SD_B54>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c];
              rhs_quad(q, xt, k5, bks[4]); }
            SEP_STAGE_PAD(3, k5[0]);
            { const double f1 = strict_coef<SD_B61>(vecA, vecB), f2 = strict_coef<SD_B62>(vecA, vecB), f3 = strict_coef<SD_B63>(vecA, vecB), f4 = strict_coef<SD_B64>(vecA, vecB),
                           f5 = strict_coef<SD_B65>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c] + f5 * k5[c];
              rhs_quad(q, xt, k6, bks[5]); }
            SEP_STAGE_PAD(4, k6[0]);
            { const double f1 = strict_coef<SD_C1>(vecA, vecB), f3 = strict_coef<SD_C3>(vecA, vecB), f4 = strict_coef<SD_C4>(vecA, vecB), f5 = strict_coef<SD_C5>(vecA, vecB),
                           f6 = strict_coef<SD_C6>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xnew[c] = x[c] + f1 * k1[c] + f3 * k3[c] + f4 * k4[c] + f5 * k5[c] + f6 * k6[c];
              rhs_quad(q, xnew, k7, bks[6]); }
            SEP_STAGE_PAD(5, k7[0]);
            { const double e1 = strict_coef<SD_DC1>(vecA, vecB), e3 = strict_coef<SD_DC3>(vecA, vecB), e4 = strict_coef<SD_DC4>(vecA, vecB), e5 = strict_coef<SD_DC5>(vecA, vecB),
                           e6 = strict_coef<SD_DC6>(vecA, vecB), e7 = strict_coef<SD_DC7>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xerr[c] = e1 * k1[c] + e3 * k3[c] + e4 * k4[c] + e5 * k5[c] + e6 * k6[c] + e7 * k7[c]; }
        } else {
            rhs_quad(q, x, k1, bks[0]);
            SEP_STAGE_PAD_CK(0, k1[0]);
            { const double f1 = strict_coef<SK_A21>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c) xt[c] = x[c] + f1 * k1[c];
              rhs_quad(q, xt, k2, bks[1]); }
            SEP_STAGE_PAD_CK(1, k2[0]);
            { const double f1 = strict_coef<SK_A31>(vecA, vecB), f2 = strict_coef<SK_A32>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c];
              rhs_quad(q, xt, k3, bks[2]); }
            SEP_STAGE_PAD_CK(2, k3[0]);
            { const double f1 = strict_coef<SK_A41>(vecA, vecB), f2 = strict_coef<SK_A42>(vecA, vecB), f3 = strict_coef<SK_A43>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c) xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c];
              rhs_quad(q, xt, k4, bks[3]); }
            SEP_STAGE_PAD_CK(3, k4[0]);
            { const double f1 = strict_coef<SK_A51>(vecA, vecB), f2 = strict_coef<SK_A52>(vecA, vecB), f3 = strict_coef<SK_A53>(vecA, vecB), f4 = strict_coef<SK_A54>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c];
              rhs_quad(q, xt, k5, bks[4]); }
            SEP_STAGE_PAD_CK(4, k5[0]);
            { const double f1 = strict_coef<SK_A61>(vecA, vecB), f2 = strict_coef<SK_A62>(vecA, vecB), f3 = strict_coef<SK_A63>(vecA, vecB), f4 = strict_coef<SK_A64>(vecA, vecB),
                           f5 = strict_coef<SK_A65>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xt[c] = x[c] + f1 * k1[c] + f2 * k2[c] + f3 * k3[c] + f4 * k4[c] + f5 * k5[c];
              rhs_quad(q, xt, k6, bks[5]); }
            SEP_STAGE_PAD_CK(5, k6[0]);
            { const double f1 = strict_coef<SK_B1>(vecA, vecB), f3 = strict_coef<SK_B3>(vecA, vecB), f4 = strict_coef<SK_B4>(vecA, vecB), f6 = strict_coef<SK_B6>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xnew[c] = x[c] + f1 * k1[c] + f3 * k3[c] + f4 * k4[c] + f6 * k6[c]; }
            { const double e1 = strict_coef<SK_DB1>(vecA, vecB), e3 = strict_coef<SK_DB3>(vecA, vecB), e4 = strict_coef<SK_DB4>(vecA, vecB), e5 = strict_coef<SK_DB5>(vecA, vecB),
                           e6 = strict_coef<SK_DB6>(vecA, vecB);
              SEP_UNROLL for (int c = 0; c < NS; ++c)
                  xerr[c] = e1 * k1[c] + e3 * k3[c] + e4 * k4[c] + e5 * k5[c] + e6 * k6[c]; }
        }

#endif

#ifdef SEPAIHRD_PHASE_NOPS_TAIL
        SEP_PHASE_PAD(SEPAIHRD_PHASE_NOPS_TAIL);
#endif
        // default_error_checker / default_step_adjuster: see the 4-lane kernel
        SEP_STAMP(st2);
        double sc[NS], ea[NS];
        lanemask over = 0ull;
        SEP_UNROLL
        for (int c = 0; c < NS; ++c) {
            sc[c] = eps_abs + eps_rel * (fabs(x[c]) + cur * fabs(k1[c]));
            ea[c] = fabs(xerr[c]);
            over |= lanes_where(ea[c] > sc[c]);
        }
        const lanemask grow_relevant = lanes_where(dt < pb.max_gap) & lanes_where(4.5000001 * cur > dt);
        double err = 0.0;
        if ((act & (over | grow_relevant)) != 0ull) {
            SEP_UNROLL
            for (int c = 0; c < NS; ++c) err = max_keep(err, quotient(ea[c], sc[c]));
            err = group_max<QUAD_LANES>(err);
        }
        const lanemask reject = lanes_where(err > 1.0);
        ++attempts;
        const lanemask dec_m = act & reject;
        const lanemask inc_m = act & ~reject & lanes_where(err < 0.5) & grow_relevant;
        // Whatever only a rejection or a change of the step size touches lives in the block that only those
        // attempts (40 %) enter -- every branch costs a lone wave 9-15 cycles and every vector instruction ~5
        // (tools/ubench/frontend.hip).  When no chain of the wave rejects or grows, cur_after = cur <= dt: dt keeps its value
        // (max(dt, cur) = dt), every active chain accepted (its count of consecutive failures is 0) and nothing can give up.
        // (Control code only: both arithmetic builds share it, measured in each -- the strict build has two code placements 8 %
        // apart, DESIGN.md 4, and this form sits in the fast one.)
        const lanemask acc_m = act & ~reject;
        const bool acc = lane_of(acc_m);
        if (__builtin_expect((dec_m | inc_m) != 0ull, 0)) {  // 40 % of the attempts: the other 60 % fall through
            const double arg = max_moved_uniform(err, 1.0 / 3125.0);  // 5^-5: the floor of the increase rule; a rejected step has err > 1
            const bool rej = lane_of(dec_m);
            const double expo = rej ? -1.0 / (4 - 1) : -1.0 / 5;
            const double pw = 9.0 / 10.0 * pow_ctl(arg, expo);
            const double f = fmax(pw, 1.0 / 5.0);  // the floor of the decrease rule; an increase has pw > 1 (err < 0.5)
            const double cur_after = lane_of(dec_m | inc_m) ? cur * f : cur;
            dt = rej ? cur_after : (acc ? max_moved(dt, cur_after) : dt);
            n_rej += rej ? 1 : 0;
            const lanemask gave_up = dec_m & lanes_where(fails >= 500);
            if (lane_of(gave_up)) status = 2;
            act &= ~gave_up;
            fails = acc ? 0 : fails + (rej ? 1 : 0);
        } else {
            fails = 0;
        }
        n_acc += acc ? 1 : 0;
        SEP_STAMP(st3);
        {
            if (acc) {
                t += cur;
                SEP_UNROLL
                for (int c = 0; c < NS; ++c) x[c] = xnew[c];
                if (SOLVER == 0) {
                    SEP_UNROLL
                    for (int c = 0; c < NS; ++c) k1[c] = k7[c];
                }
            }
            const lanemask reached_m = acc_m & ~lanes_where((t_next - t) > DBL_EPSILON);
            if (__builtin_expect(reached_m != 0ull, 1)) {  // 72 % of the attempts end on an output time
                // the grid time after next is requested BEFORE the observer's LDS traffic and taken after it: one wait
                // covers both (a lone wave sits out every LDS round trip it waits for: ~100 cycles per output each)
                const double t_fetch = lds_times[(k_next + 2 < T) ? k_next + 2 : T - 1];
                observe_store(reached_m, k_next);
                if (lane_of(reached_m)) {
                    t = t_next;
                    ++k_next;
                    t_next = t_after;
                    t_after = t_fetch;
                }
                act &= ~(reached_m & lanes_where(k_next >= T));
            }
        }
        SEP_STAMP(st4);
    };
    // the build-side guard (the same attempt for every chain of the wave) rides in the loop condition: one branch, not two
    while (act != 0ull && attempts < pb.max_attempts) {
#ifdef SEPAIHRD_PHASE_NOPS_HEAD  // placement experiments (make -C csrc variant): 4-byte pads that shift the code behind them
        SEP_PHASE_PAD(SEPAIHRD_PHASE_NOPS_HEAD);
#endif
#if !SEPAIHRD_ARITH_FMA
        if constexpr (SOLVER == 1) SEP_PHASE_PAD(SEPAIHRD_STRICT_HEAD_PADS_CK);  // the strict Cash-Karp body's phase (see SEP_STAGE_PAD)
#endif
        SEP_STAMP(st0);
        // the minimum for every lane, then a select: an inline-asm instruction inside a lane-conditional block makes the
        // compiler keep a skip branch around it (asm counts as unsafe with an empty EXEC), and that branch is taken every attempt
        double cur_m;
        {
            const double gap = t_next - t;
            asm volatile("v_min_f64 %0, %1, %2" : "=v"(cur_m) : "v"(dt), "v"(gap));
        }
        const double cur = lane_of(act) ? cur_m : 1.0;  // a finished chain idles on a harmless step
#if SEPAIHRD_ARITH_FMA
        // the chain's step times sixteen (+10) tableau coefficients, one per lane of its row.  Their first DPP read is the
        // second stage's leading factor, behind the segment test below; that no DPP read of ANY inline-asm operand follows
        // its VALU write within two wait states is checked on the listing (tools/check_dpp_hazards.py, run by the test suite)
        double vecA, vecB;
        asm("v_mul_f64 %1, %2, %4\n\tv_mul_f64 %0, %2, %3" : "=&v"(vecA), "=&v"(vecB) : "v"(cur), "v"(coefA), "v"(coefB));  // B first: it is read first
#else
        const double vecA = cur * coefA, vecB = cur * coefB;  // the strict build's factors: strict_coef<>() hands them out
#endif
        // beta(t) kappa(t) of the stage times.  Every stage of nearly every attempt lies in the segment (lo, hi] the chain
        // is known to be in: one value, no look-up.  When some chain has left its segment the cached segment is found
        // again (LDS), and ONLY when a step straddles a breakpoint -- stages in different segments; never on a grid whose
        // outputs include the breakpoints, since no step crosses an output -- the attempt runs through the second copy
        // of the attempt code below, which takes a value per stage.  Two copies instead of one with merged inputs: a
        // merge made the common path copy its one value into seven registers and shuttle the cached segment between
        // two register sets on every attempt (15 moves of ~375 instructions).  Same arithmetic in both copies.
        const double tmin = (SOLVER == 0) ? fma(cur, dp::a2, t) : t;           // first stage time that is evaluated afresh
        const double tmax = (SOLVER == 0) ? t + cur : fma(ck::c5, cur, t);     // last one
        const lanemask in_seg = lanes_where(tmin > sch.lo) & lanes_where(tmax <= sch.hi);
        // beta*kappa at the seven stage times of a step that leaves the cached segment (c_lo, c_hi: segments of the first and
        // the last stage time); lanes that stay inside one segment get its value seven times
        auto stage_values = [&](double (&bks)[7], int c_lo, int c_hi, double v_lo, double v_hi) __attribute__((always_inline)) {
            double tau[7];
            if (SOLVER == 0) {
                tau[0] = t;
                tau[1] = t + cur * dp::a2; tau[2] = t + cur * dp::a3; tau[3] = t + cur * dp::a4;
                tau[4] = t + cur * dp::a5; tau[5] = t + cur; tau[6] = t + cur;
            } else {
                tau[0] = t;
                tau[1] = t + ck::c2 * cur; tau[2] = t + ck::c3 * cur; tau[3] = t + ck::c4 * cur;
                tau[4] = t + ck::c5 * cur; tau[5] = t + ck::c6 * cur; tau[6] = t + cur;
            }
            if (lanes_where(c_hi > c_lo + 1) == 0ull) {
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
        };
#if SEPAIHRD_ARITH_FMA
        if (__builtin_expect((act & ~in_seg) != 0ull, 0)) {  // rare: the common path falls through
            int c_lo, c_hi;
            segment_index2(sch, pb.nm_pad, tmin, tmax, c_lo, c_hi);
            const double v_lo = sch.bkv[c_lo], v_hi = sch.bkv[c_hi];
            const lanemask straddles = act & lanes_where(c_hi > c_lo);
            sch.lo = (c_hi > 0) ? sch.me[c_hi - 1] : -INFINITY;
            sch.hi = (c_hi < pb.nm) ? sch.me[c_hi] : INFINITY;
            sch.bk = v_hi;
            if (straddles != 0ull) {  // the second copy of the attempt code: a value per stage
                double bks[7];
                stage_values(bks, c_lo, c_hi, v_lo, v_hi);
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
                attempt(cur, vecA, vecB, bks);
                continue;
            }
            // every LDS read of this (rare) path is complete before it rejoins: the stage code then needs no
            // s_waitcnt of its own -- each one costs a lone wave an issue slot on EVERY attempt
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
        }
        const double one_value[7] = {sch.bk, sch.bk, sch.bk, sch.bk, sch.bk, sch.bk, sch.bk};
        attempt(cur, vecA, vecB, one_value);
#else
        // strict build: ONE copy of the attempt code, the stage values merged into it (its stage code is twice the size
        // and lives off scalar registers for its tableau constants; a second copy cost it 4 %)
        double bks[7];
        if (__builtin_expect((act & ~in_seg) != 0ull, 0)) {  // rare: the common path falls through
            int c_lo, c_hi;
            segment_index2(sch, pb.nm_pad, tmin, tmax, c_lo, c_hi);
            const double v_lo = sch.bkv[c_lo], v_hi = sch.bkv[c_hi];
            stage_values(bks, c_lo, c_hi, v_lo, v_hi);
            sch.lo = (c_hi > 0) ? sch.me[c_hi - 1] : -INFINITY;
            sch.hi = (c_hi < pb.nm) ? sch.me[c_hi] : INFINITY;
            sch.bk = v_hi;
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
        } else {
            SEP_UNROLL
            for (int s = 0; s < 7; ++s) bks[s] = sch.bk;
        }
        attempt(cur, vecA, vecB, bks);
#endif
#ifdef SEPAIHRD_STAMPS
        acc_head += st1 - st0; acc_body += st2 - st1; acc_err += st3 - st2; acc_tail += st4 - st3;
#endif
    }

    if (lane_of(act)) status = 3;  // chains still integrating when the guard ended the loop
#ifdef SEPAIHRD_STAMPS
    if (chain_valid && age == 0 && cg == 0 && out.ll_parts) {  // diagnostic build: the wave's section totals
        double* dbg = out.ll_parts + 3 * chain;
        if (grp == 0) { dbg[0] = (double)acc_head; dbg[1] = (double)acc_body; dbg[2] = (double)acc_err; }
        if (grp == 1) { dbg[0] = (double)acc_tail; dbg[1] = (double)attempts; dbg[2] = 0.0; }
    }
#endif
    if constexpr (FUSED) {
        // hand the integrator's verdict to the consumer, then the flag that says no more rows will come
        if (age == 0 && cg == 0) {
            ctl.final_[3 * grp + 0] = status;
            ctl.final_[3 * grp + 1] = n_acc;
            ctl.final_[3 * grp + 2] = n_rej;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) st_release(ctl.done, 1);
    } else {
        if (chain_valid && age == 0 && cg == 0) {
            out.wstatus[chain] = status;  // the likelihood pass finishes the evaluation
            if (out.n_accept) out.n_accept[chain] = n_acc;
            if (out.n_reject) out.n_reject[chain] = n_rej;
        }
    }
}

// Up to this many chains (one wave per SIMD: 1024 waves of 4 chains) the 16-lane form is launched; beyond it some
// SIMDs would hold two of its waves while the 4-lane kernel still has at most one wave per SIMD and fewer
// instructions in total (measured, Dopri5: 4096 chains 0.67 vs 0.96 ms, 6144 chains 1.06 vs 1.01 ms).
constexpr int QUAD_MAX_CHAINS = 4096;

// The small-batch form evaluates the likelihood on consumer waves of its own workgroup; the ensemble summaries
// (force_split) use the separate pass: they read the parked increments.  Experiment builds: SEPAIHRD_FUSED_LL=0 keeps
// the separate pass everywhere (A/B measurements).
inline bool quad_fused_wanted() {
#ifdef SEPAIHRD_EXPERIMENTS
    static const int mode = [] {
        const char* e = getenv("SEPAIHRD_FUSED_LL");
        return e == nullptr ? 1 : atoi(e);
    }();
    return mode != 0;
#else
    return true;
#endif
}

// fused: the likelihood on consumer waves (EvalForm::QuadFused), else as a separate pass (choose_form decides)
template <int SOLVER>
int launch_quad(const DevProblem& pb, const double* d_theta, int B, const EvalOutputs& out, void* stream, bool fused) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (fused) {
        const int wgs = (B + QUAD_UNITS * QUAD_CPW - 1) / (QUAD_UNITS * QUAD_CPW);
        static const bool lds_limit_raised = [] {  // dynamic LDS beyond the default 64 KiB needs the opt-in
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&sepaihrd_eval_quad_kernel<SOLVER, SEPAIHRD_ARITH_FMA, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)QUAD_FUSED_MAX_LDS) == hipSuccess;
        }();
        if (!lds_limit_raised && quad_fused_lds_bytes(pb) > 64 * 1024) return -3;
        if (out.traj == nullptr) {
            static const bool lds_limit_raised_plain = [] {
                return hipFuncSetAttribute(reinterpret_cast<const void*>(&sepaihrd_eval_quad_kernel<SOLVER, SEPAIHRD_ARITH_FMA, true, false>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)QUAD_FUSED_MAX_LDS) == hipSuccess;
            }();
            if (!lds_limit_raised_plain && quad_fused_lds_bytes(pb) > 64 * 1024) return -3;
            hipLaunchKernelGGL((sepaihrd_eval_quad_kernel<SOLVER, SEPAIHRD_ARITH_FMA, true, false>), dim3(wgs), dim3(8 * WAVE), quad_fused_lds_bytes(pb),
                               st, pb, d_theta, B, out, 0);
            if (out.ev_after_integrator) (void)hipEventRecord(static_cast<hipEvent_t>(out.ev_after_integrator), st);
            return hipGetLastError() == hipSuccess ? 0 : -3;
        }
        hipLaunchKernelGGL((sepaihrd_eval_quad_kernel<SOLVER, SEPAIHRD_ARITH_FMA, true>), dim3(wgs), dim3(8 * WAVE), quad_fused_lds_bytes(pb), st,
                           pb, d_theta, B, out, 0);
        if (out.ev_after_integrator) (void)hipEventRecord(static_cast<hipEvent_t>(out.ev_after_integrator), st);
        return hipGetLastError() == hipSuccess ? 0 : -3;
    }
    if (out.cum == nullptr || out.rows == nullptr || out.wstatus == nullptr) return -5;  // see needs_workspace_one()
    const size_t lds = eval_lds_bytes(pb);
    const int blocks = (B + QUAD_CPW - 1) / QUAD_CPW;
    const int ll_blocks = (B + 15) / 16;             // the likelihood passes keep the 4-lane column layout
    const int cum_chains = ll_blocks * 16;
    hipLaunchKernelGGL((sepaihrd_eval_quad_kernel<SOLVER, SEPAIHRD_ARITH_FMA, false>), dim3(blocks), dim3(WAVE), lds, st, pb, d_theta, B, out, cum_chains);
    if (out.ev_after_integrator) (void)hipEventRecord(static_cast<hipEvent_t>(out.ev_after_integrator), st);
    if (out.force_split == FORCE_SPLIT_PARK_ONLY) return hipGetLastError() == hipSuccess ? 0 : -3;  // the caller's own pass follows
    hipLaunchKernelGGL((sepaihrd_ll_terms_kernel<4>), dim3(ll_blocks, (pb.T + LL_DAYS_PER_BLOCK - 1) / LL_DAYS_PER_BLOCK),
                       dim3(WAVE * LL_DAYS_PER_BLOCK), 0, st, pb, B, out, cum_chains);
    hipLaunchKernelGGL(sepaihrd_ll_reduce_kernel, dim3((B + 15) / 16), dim3(WAVE), 0, st, pb, B, out, cum_chains, pb.T);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
