// csrc/sepaihrd_dev_common.inc -- device helpers shared by the fp64 kernels (sepaihrd_kernels.hip, compiled twice) and
// the fp32-state kernels (sepaihrd_kernels_f32.hip).  Included inside namespace sepaihrd { namespace { ... } }.
//   cross-lane helpers (DPP), Butcher tableaus as Boost.Odeint writes them, applyConstraints, the merged beta*kappa
//   schedule lookup, the fp64 natural log of the Poisson term.

// ----------------------------------------------------------------------------------
// cross-lane helpers: a chain is LPC adjacent lanes
// ----------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// row_newbcast (gfx90a+): lane LA of each 16-lane row into the lanes of banks BA, then (BB != 0) lane LB into
// the lanes of banks BB; a bank = four adjacent lanes.  No LDS traffic and nothing to wait for, unlike
// ds_bpermute behind __shfl (the n = 16 RHS did 32 of those per call with ~15 waits: LDS latency, not
// arithmetic, set its pace).
template <int LA, int BA, int LB, int BB>
__device__ __forceinline__ double dpp_bcast_row(double v) {
    // row_newbcast is the one DPP control the double-precision ALU accepts on 64-bit operands (gfx90a+):
    // v_mov_b64_dpp, one instruction per value.  First move into ALL banks (no "old" value to materialise), the
    // second overwrites banks BB only.
    (void)BA;
    double r = __builtin_amdgcn_update_dpp(0.0, v, 0x150 + LA, 0xf, 0xf, true);
    if constexpr (BB != 0) r = __builtin_amdgcn_update_dpp(r, v, 0x150 + LB, 0xf, BB, false);
    return r;
}

// acc += m * (lane LANE of src's 16-lane row), in the lanes of banks BANKS: v_fmac_f64 with its first source through
// DPP row_newbcast -- the broadcast costs no instruction of its own.  Inline asm is opaque to the hazard pass, so the
// first term of a chain carries the two wait states a DPP read needs after the VALU write of `src`.
template <int LANE, int BANKS, bool FIRST>
__device__ __forceinline__ void fmac_row_bcast(double& acc, double src, double m) {
    if constexpr (FIRST)
        asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:%4"
            : "+v"(acc) : "v"(src), "v"(m), "n"(LANE), "n"(BANKS));
    else
        asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:%4"
            : "+v"(acc) : "v"(src), "v"(m), "n"(LANE), "n"(BANKS));
}

// A value the optimiser may not look through.  The tolerance build folds per-chain constants once per evaluation, among them
// pg = p gamma_p and gamma_p - pg; under -ffp-contract=fast the compiler is free to turn the latter into fma(-p, gamma_p, gamma_p)
// -- one rounding instead of two -- and whether it does depends on the code around it (round 4: the 16-lane form did, the
// 4-lane form did not, and their trajectories parted in the 16th digit).  Every form passes pg through this, so the
// difference is a plain subtraction of a rounded product everywhere.
__device__ __forceinline__ double rounded_here(double v) {
    asm volatile("" : "+v"(v));
    return v;
}

// value held by lane J of my chain group
template <int LPC, int J>
__device__ __forceinline__ double group_bcast(double v) {
    if constexpr (LPC == 1) {
        return v;
    } else if constexpr (LPC == 2) {
        return dpp_move<(J) | (J << 2) | ((2 + J) << 4) | ((2 + J) << 6)>(v);  // quad_perm
    } else if constexpr (LPC == 4) {
        return dpp_move<J * 0x55>(v);  // quad_perm:[J,J,J,J]
    } else if constexpr (LPC == 16) {
        return dpp_bcast_row<J, 0xf, J, 0x0>(v);  // row_newbcast:J -- lane J of every 16-lane row
    } else if constexpr (LPC == 8) {
        // two chains per 16-lane row: banks 0-1 (lanes 0-7) take lane J, banks 2-3 (lanes 8-15) take lane 8+J
        return dpp_bcast_row<J, 0x3, 8 + J, 0xc>(v);
    } else {
        return __shfl(v, J, LPC);
    }
}

// Row sums of one output day for the three streams: rs[s] = ((t_0 + t_1) + t_2) + ... over the ages of my chain, ascending
// (calculateSingleLogLikelihood's inner loop, SEPAIHRDObjectiveFunction.cpp:264-276; "0.0 +" dropped: value-identical).
// Sixteen ages = a DPP row: every term after the first is ONE instruction, v_fmac_f64_dpp with the factor 1.0 -- the
// product is exact, the sum rounds once, the bits are v_add_f64's -- instead of a broadcast move plus an add (31 -> 16
// instructions per stream); the three chains alternate, so no instruction reads what the one before it wrote.
#ifndef SEPAIHRD_ROW_SUM_FMAC
#define SEPAIHRD_ROW_SUM_FMAC 1  // 0: broadcast move + add per term (A/B builds, make -C csrc variant)
#endif
template <int LPC>
__device__ __forceinline__ void row_sums3(const double (&tv)[3], double (&rs)[3]) {
    if constexpr (LPC == 16 && SEPAIHRD_ROW_SUM_FMAC != 0) {
        rs[0] = group_bcast<16, 0>(tv[0]);
        rs[1] = group_bcast<16, 0>(tv[1]);
        rs[2] = group_bcast<16, 0>(tv[2]);
        // the factor is made HERE, once per output day: as a loop invariant it would hold two registers through the whole RK
        // body of a kernel that already spills (256 registers, two waves per SIMD)
        double one;
        asm volatile("v_mov_b64 %0, 1.0" : "=v"(one));
        [&]<int... J>(std::integer_sequence<int, J...>) {
            ((fmac_row_bcast<J + 1, 0xf, false>(rs[0], tv[0], one), fmac_row_bcast<J + 1, 0xf, false>(rs[1], tv[1], one),
              fmac_row_bcast<J + 1, 0xf, false>(rs[2], tv[2], one)), ...);
        }(std::make_integer_sequence<int, 15>{});
    } else {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            double r = group_bcast<LPC, 0>(tv[s]);
            [&]<int... J>(std::integer_sequence<int, J...>) {
                ((r += group_bcast<LPC, J + 1>(tv[s])), ...);
            }(std::make_integer_sequence<int, LPC - 1>{});
            rs[s] = r;
        }
    }
}

// NaN-ignoring max (std::max(init, v) with init never NaN: odeint's norm_inf).  fmax = v_max_f64 returns
// the non-NaN operand, which is exactly (m < v) ? v : m for a non-NaN m -- one instruction instead of three.
__device__ __forceinline__ double max_keep(double m, double v) { return fmax(m, v); }

// The same instruction without the compiler's canonicalisation of the DPP-moved operand (fmax on a value that comes out
// of a lane move gets a v_max_f64 x, x, x in front of it: the move's result is not known to be a quiet number).  The
// operands here are error quotients that already went through an FP64 instruction.
__device__ __forceinline__ double max_moved(double m, double v) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(m), "v"(v));
    return r;
}

// max(m, c) with a wave-uniform c (scalar operand): for a value that came out of group_max
__device__ __forceinline__ double max_moved_uniform(double m, double c) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(m), "s"(c));
    return r;
}

template <int LPC>
__device__ __forceinline__ double group_max(double m) {
    if constexpr (LPC == 1) {
        return m;
    } else if constexpr (LPC == 2) {
        return max_moved(m, dpp_move<0xB1>(m));  // quad_perm:[1,0,3,2]
    } else if constexpr (LPC == 4) {
        m = max_moved(m, dpp_move<0xB1>(m));
        return max_moved(m, dpp_move<0x4E>(m));  // quad_perm:[2,3,0,1]
    } else if constexpr (LPC == 8 || LPC == 16) {
        m = max_moved(m, dpp_move<0xB1>(m));   // quad_perm:[1,0,3,2]
        m = max_moved(m, dpp_move<0x4E>(m));   // quad_perm:[2,3,0,1]: every quad holds its max
        m = max_moved(m, dpp_move<0x141>(m));  // row_half_mirror: lane i <-> 7 - i within each 8 lanes
        if constexpr (LPC == 16) m = max_moved(m, dpp_move<0x140>(m));  // row_mirror: lane i <-> 15 - i
        return m;
    } else {
#pragma unroll
        for (int off = LPC / 2; off > 0; off >>= 1) m = max_keep(m, __shfl_xor(m, off));
        return m;
    }
}

// any() over my chain group
template <int LPC>
__device__ __forceinline__ bool group_any(bool pred, int lane) {
    const unsigned long long b = __ballot(pred);
    if constexpr (LPC == 64) {
        return b != 0ull;
    } else {
        const unsigned long long mask = ((1ull << LPC) - 1ull) << (lane & ~(LPC - 1));
        return (b & mask) != 0ull;
    }
}

// ----------------------------------------------------------------------------------
// tableaus, written as Boost.Odeint writes them: quotients of doubles; the Dopri5 error
// weights are DIFFERENCES of rounded quotients (runge_kutta_dopri5.hpp do_step_impl).
// ----------------------------------------------------------------------------------
namespace dp {
constexpr double a2 = 1.0 / 5, a3 = 3.0 / 10, a4 = 4.0 / 5, a5 = 8.0 / 9;
constexpr double b21 = 1.0 / 5;
constexpr double b31 = 3.0 / 40, b32 = 9.0 / 40;
constexpr double b41 = 44.0 / 45, b42 = -56.0 / 15, b43 = 32.0 / 9;
constexpr double b51 = 19372.0 / 6561, b52 = -25360.0 / 2187, b53 = 64448.0 / 6561, b54 = -212.0 / 729;
constexpr double b61 = 9017.0 / 3168, b62 = -355.0 / 33, b63 = 46732.0 / 5247, b64 = 49.0 / 176,
                 b65 = -5103.0 / 18656;
constexpr double c1 = 35.0 / 384, c3 = 500.0 / 1113, c4 = 125.0 / 192, c5 = -2187.0 / 6784, c6 = 11.0 / 84;
constexpr double dc1 = c1 - 5179.0 / 57600, dc3 = c3 - 7571.0 / 16695, dc4 = c4 - 393.0 / 640,
                 dc5 = c5 - (-92097.0 / 339200), dc6 = c6 - 187.0 / 2100, dc7 = -1.0 / 40;
}  // namespace dp
namespace ck {
constexpr double c2 = 1.0 / 5, c3 = 3.0 / 10, c4 = 3.0 / 5, c5 = 1.0, c6 = 7.0 / 8;
constexpr double a21 = 1.0 / 5;
constexpr double a31 = 3.0 / 40, a32 = 9.0 / 40;
constexpr double a41 = 3.0 / 10, a42 = -9.0 / 10, a43 = 6.0 / 5;
constexpr double a51 = -11.0 / 54, a52 = 5.0 / 2, a53 = -70.0 / 27, a54 = 35.0 / 27;
constexpr double a61 = 1631.0 / 55296, a62 = 175.0 / 512, a63 = 575.0 / 13824, a64 = 44275.0 / 110592,
                 a65 = 253.0 / 4096;
constexpr double b1 = 37.0 / 378, b3 = 250.0 / 621, b4 = 125.0 / 594, b6 = 512.0 / 1771;
constexpr double db1 = 37.0 / 378 - 2825.0 / 27648, db3 = 250.0 / 621 - 18575.0 / 48384,
                 db4 = 125.0 / 594 - 13525.0 / 55296, db5 = -277.0 / 14336, db6 = 512.0 / 1771 - 1.0 / 4;
}  // namespace ck
// runge_kutta_fehlberg78 (Fehlberg 1968): every coefficient one quotient of two integers, rounded once.  Zero entries
// are left out.  The error weights db_i = b_i - bhat_i are exact (+-41/840 at stages 1, 11, 12, 13; zero elsewhere).
namespace f78 {
constexpr double c2 = 2.0 / 27, c3 = 1.0 / 9, c4 = 1.0 / 6, c5 = 5.0 / 12, c6 = 1.0 / 2, c7 = 5.0 / 6, c8 = 1.0 / 6,
                 c9 = 2.0 / 3, c10 = 1.0 / 3, c11 = 1.0 / 1, c13 = 1.0 / 1;
constexpr double a2_1 = 2.0 / 27;
constexpr double a3_1 = 1.0 / 36, a3_2 = 1.0 / 12;
constexpr double a4_1 = 1.0 / 24, a4_3 = 1.0 / 8;
constexpr double a5_1 = 5.0 / 12, a5_3 = -25.0 / 16, a5_4 = 25.0 / 16;
constexpr double a6_1 = 1.0 / 20, a6_4 = 1.0 / 4, a6_5 = 1.0 / 5;
constexpr double a7_1 = -25.0 / 108, a7_4 = 125.0 / 108, a7_5 = -65.0 / 27, a7_6 = 125.0 / 54;
constexpr double a8_1 = 31.0 / 300, a8_5 = 61.0 / 225, a8_6 = -2.0 / 9, a8_7 = 13.0 / 900;
constexpr double a9_1 = 2.0 / 1, a9_4 = -53.0 / 6, a9_5 = 704.0 / 45, a9_6 = -107.0 / 9, a9_7 = 67.0 / 90, a9_8 = 3.0 / 1;
constexpr double a10_1 = -91.0 / 108, a10_4 = 23.0 / 108, a10_5 = -976.0 / 135, a10_6 = 311.0 / 54, a10_7 = -19.0 / 60,
                 a10_8 = 17.0 / 6, a10_9 = -1.0 / 12;
constexpr double a11_1 = 2383.0 / 4100, a11_4 = -341.0 / 164, a11_5 = 4496.0 / 1025, a11_6 = -301.0 / 82, a11_7 = 2133.0 / 4100,
                 a11_8 = 45.0 / 82, a11_9 = 45.0 / 164, a11_10 = 18.0 / 41;
constexpr double a12_1 = 3.0 / 205, a12_6 = -6.0 / 41, a12_7 = -3.0 / 205, a12_8 = -3.0 / 41, a12_9 = 3.0 / 41, a12_10 = 6.0 / 41;
constexpr double a13_1 = -1777.0 / 4100, a13_4 = -341.0 / 164, a13_5 = 4496.0 / 1025, a13_6 = -289.0 / 82, a13_7 = 2193.0 / 4100,
                 a13_8 = 51.0 / 82, a13_9 = 33.0 / 164, a13_10 = 12.0 / 41, a13_12 = 1.0 / 1;
constexpr double b6 = 34.0 / 105, b7 = 9.0 / 35, b8 = 9.0 / 35, b9 = 9.0 / 280, b10 = 9.0 / 280, b12 = 41.0 / 840, b13 = 41.0 / 840;
constexpr double db1 = -41.0 / 840, db11 = -41.0 / 840, db12 = 41.0 / 840, db13 = 41.0 / 840;
}  // namespace f78

#include "sepaihrd_constrain.inc"  // reflect_bound, constrain: the one text of the constraint rule

// Merged beta*kappa schedule of one chain.  Segment j = (mends[j-1], mends[j]], value index = #(mends < t).
struct Schedule {
    const double* me;   // LDS: merged end times, +inf padded to an even count (block-uniform)
    const double* bkv;  // LDS: this chain's beta*kappa per merged segment [nm + 1]
    double lo, hi, bk;  // cached segment (lo, hi] and its value
};

// segment indices of two times in one pass over the merged end times (uniform LDS broadcast reads)
__device__ __forceinline__ void segment_index2(const Schedule& s, int nm_pad, double ta, double tb, int& ca,
                                               int& cb) {
    ca = 0; cb = 0;
    for (int j = 0; j < nm_pad; j += 2) {
        const double2 e = *reinterpret_cast<const double2*>(s.me + j);
        ca += (ta > e.x) ? 1 : 0; ca += (ta > e.y) ? 1 : 0;
        cb += (tb > e.x) ? 1 : 0; cb += (tb > e.y) ? 1 : 0;
    }
}

#define SEP_UNROLL _Pragma("unroll")

// ----------------------------------------------------------------------------------
// natural log of the strict build's step-size controller (pow_ctl: exp(c log x)).  Argument reduction x = 2^k (1+f),
// sqrt(1/2) <= 1+f < sqrt(2), s = f/(2+f), log(1+f) = f - (f^2/2 - s (f^2/2 + R(s^2))) with the classic degree-14 minimax R
// (error < 2^-58.45 on the reduced interval); < 1 ulp overall in ~40 instructions, no branches, no table.  It was the Poisson
// term's log as well through round 4's first builds; that one is log_pos() below now.
// ----------------------------------------------------------------------------------
__device__ __forceinline__ double log_ctl(double x) {
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    constexpr double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                     Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                     Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                     Lg7 = 1.479819860511658591e-01;
    int k = __builtin_amdgcn_frexp_exp(x);          // x = m * 2^k, m in [0.5, 1)
    double m = __builtin_amdgcn_frexp_mant(x);
    const bool low = m < 0.70710678118654752440;
    m = low ? m + m : m;                            // [sqrt(1/2), sqrt(2))
    k = low ? k - 1 : k;
    const double f = m - 1.0;
    const double dk = (double)k;
    // s = f / (2 + f): denominator in [1.70, 2.42], so a Newton-refined reciprocal and one residual
    // correction give the correctly rounded quotient's neighbourhood (<= 1 ulp) without the IEEE
    // division's scaling / fix-up instructions
    const double den = 2.0 + f;
    double r = __builtin_amdgcn_rcp(den);           // ~2^-26 relative
    r = fma(fma(-den, r, 1.0), r, r);               // one Newton step: ~2^-52 (a second one, rounds 1-3, bought nothing: the
    double sdiv = f * r;                            // residual correction below only needs r to ~2^-30)
    sdiv = fma(fma(-den, sdiv, f), r, sdiv);
    const double z = sdiv * sdiv;
    const double w = z * z;
    const double t1 = w * fma(w, fma(w, Lg6, Lg4), Lg2);
    const double t2 = z * fma(w, fma(w, fma(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    // x = +inf or NaN (a blown-up state) comes out as NaN: den = inf, r = 0, 0 * inf.  The reference's log(+inf) = +inf turns
    // its Poisson term into obs inf - inf = NaN as well, and a NaN total is lowest() either way (SEPAIHRDObjectiveFunction.cpp:227):
    // no select for the pass-through.
    return dk * ln2_hi - ((hfsq - fma(sdiv, hfsq + R, dk * ln2_lo)) - f);
}

// ----------------------------------------------------------------------------------
// natural log for the Poisson term: the table path of glibc's double-precision log (sysdeps/ieee754/dbl-64/e_log.c, FMA
// variant -- the libm the CPU build links), same operations in the same order, on the constants csrc/sepaihrd_glibc_log.inc
// holds: x = 2^k z, the 128-entry table gives invc ~ 1/c and logc ~ log(c) for the c nearest z, r = z invc - 1 (|r| < 2^-7,
// one fma), log x = k ln2 + logc + log1p(r) with a degree-5 polynomial and a two-term head.  ~22 instructions and one
// 16-byte LDS read against ~40 and a quarter-rate reciprocal for log_ctl(): three logs per lane and output day are a tenth
// of a saturating batch's step (DESIGN.md 4).  Outside glibc's near-one window [1 - 2^-4, 1 + 0x1.09p-4) the result is
// std::log's, bit for bit; inside it glibc switches to a longer polynomial for the sake of the RELATIVE error of a result
// near zero, which a term obs log(sim) of a sum near 1e5 has no use for: the table path stays within 1e-17 absolute there (7.2e-18 over
// 1e7 arguments; tests/test_gpu_parity.py compares both regimes with the host's log).  Domain: x >= 1e-10 (sim + epsilon), normal numbers.
// +inf or NaN (a blown-up state) gives a finite number here; the term obs log(sim) - sim is then -inf or NaN by its second
// half and the total fails the finiteness check exactly as the reference's does (SEPAIHRDObjectiveFunction.cpp:227).
// The table lives in LDS (2 KB per block; stage_log_table() + a barrier in every kernel that takes logs).
// ----------------------------------------------------------------------------------
__shared__ __attribute__((aligned(16))) double lds_log_table[128][2];
static_assert(sizeof(double) * 128 * 2 == LOG_TABLE_LDS_BYTES, "sepaihrd_device.h budgets the table");

struct LogTable {
#pragma push_macro("SEP_LOG_CONST")
#undef SEP_LOG_CONST
#define SEP_LOG_CONST static constexpr
#include "sepaihrd_glibc_log.inc"
#pragma pop_macro("SEP_LOG_CONST")
};
// the 2 KB in global memory that stage_log_table() copies from
__device__ const double2 global_log_table[128] = {
#define SEP_E(i) {LogTable::GLOG_T[i][0], LogTable::GLOG_T[i][1]}
#define SEP_E8(i) SEP_E(i), SEP_E(i + 1), SEP_E(i + 2), SEP_E(i + 3), SEP_E(i + 4), SEP_E(i + 5), SEP_E(i + 6), SEP_E(i + 7)
    SEP_E8(0), SEP_E8(8), SEP_E8(16), SEP_E8(24), SEP_E8(32), SEP_E8(40), SEP_E8(48), SEP_E8(56),
    SEP_E8(64), SEP_E8(72), SEP_E8(80), SEP_E8(88), SEP_E8(96), SEP_E8(104), SEP_E8(112), SEP_E8(120)
#undef SEP_E8
#undef SEP_E
};

__device__ __forceinline__ void stage_log_table(int tid, int nthreads) {
    for (int i = tid; i < 128; i += nthreads) *reinterpret_cast<double2*>(lds_log_table[i]) = global_log_table[i];
}

#ifndef SEPAIHRD_POISSON_LOG_TABLE
#define SEPAIHRD_POISSON_LOG_TABLE 1  // 0: the table-free log of rounds 1-3 (A/B builds, make -C csrc variant)
#endif
// the table entry of x and the reduced argument z: everything of log_pos() before its first floating-point operation
struct LogLookup { double2 e; double z; int k; };
__device__ __forceinline__ LogLookup log_lookup(double x) {
    // ix - OFF, OFF = 0x3fe6000000000000: its low word is zero, so the high words alone carry the subtraction
    const int hi_w = __double2hiint(x);
    const int tmp = hi_w - 0x3fe60000;
    const int i = (tmp >> 13) & 127;           // (tmp >> 45) % 128 of the 64-bit form
    LogLookup L;
    L.k = tmp >> 20;                           // (int64_t)tmp >> 52
    L.z = __hiloint2double(hi_w - (L.k << 20), __double2loint(x));  // ix - (tmp & 0xfff << 52)
    L.e = *reinterpret_cast<const double2*>(lds_log_table[i]);
    return L;
}
__device__ __forceinline__ double log_finish(const LogLookup& L) {
    constexpr double LN2HI = 0x1.62e42fefa3800p-1, LN2LO = 0x1.ef35793c76730p-45;  // GLOG_LN2HI / _LO
    constexpr double A0 = -0x1.0000000000001p-1, A1 = 0x1.555555551305bp-2, A2 = -0x1.fffffffeb4590p-3,
                     A3 = 0x1.999b324f10111p-3, A4 = -0x1.55575e506c89fp-3;        // GLOG_A
    const double invc = L.e.x, logc = L.e.y;
    const double r = fma(L.z, invc, -1.0);
    const double kd = (double)L.k;
    const double w = fma(kd, LN2HI, logc);
    const double hi = r + w;
    const double t39 = (w - hi) + r;
    const double lo = fma(kd, LN2LO, t39);
    const double r2 = r * r;
    const double t42 = fma(r2, A0, lo);
    const double t43 = r * r2;
    const double t45 = fma(r, A2, A1);
    const double t47 = fma(r, A4, A3);
    const double t49 = fma(t47, r2, t45);
    const double t51 = fma(t43, t49, t42);
    return t51 + hi;
}
__device__ __forceinline__ double log_pos(double x) {
#if !SEPAIHRD_POISSON_LOG_TABLE
    return log_ctl(x);
#endif
    return log_finish(log_lookup(x));
}
// The three logs of one output day (streams H, ICU, D of a lane's age class): all three table reads leave before the first
// of them is waited for.  Left to itself the compiler finishes one log before it starts the next -- three LDS round trips
// per output, which a kernel at one or two waves per SIMD sits out.  Same operations per log: same bits as log_pos().
__device__ __forceinline__ void log_pos3(const double (&x)[3], double (&out)[3]) {
#if !SEPAIHRD_POISSON_LOG_TABLE
    out[0] = log_ctl(x[0]); out[1] = log_ctl(x[1]); out[2] = log_ctl(x[2]);
    return;
#endif
    const LogLookup a = log_lookup(x[0]), b = log_lookup(x[1]), c = log_lookup(x[2]);
    __builtin_amdgcn_sched_barrier(0);  // nothing of the evaluation moves above the third read
    out[0] = log_finish(a); out[1] = log_finish(b); out[2] = log_finish(c);
}

