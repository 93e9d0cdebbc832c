// csrc/sepaihrd_particle_wide.hip -- the wide form of the bootstrap particle filter of the stochastic SEPAIHRD model on gfx950
// (sepaihrd_particle_loglik_wide): the particles of a theta in device memory, J up to 65 536, the work of
// one output segment spread over the whole device.  The rules are csrc/sepaihrd_particle.inc and the interval walk is
// csrc/sepaihrd_stoch_sepaihrd.inc's lane_interval, the texts csrc/sepaihrd_particle.hip and the host twin compile too: for
// J within sepaihrd_particle_max_particles the results are the bits of sepaihrd_particle_loglik, for every J those of the twin.
// Plain launches one after another on one stream carry the order: no cooperative launch, no barrier across workgroups.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <vector>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_particle.inc"
#include "sepaihrd_particle_states_device.h"
#include "sepaihrd_particle_wide_device.h"
#include "sepaihrd_stoch_sepaihrd_device.h"

namespace sepaihrd {
namespace {

namespace epi = sepaihrd_stoch_epi;
namespace pf = sepaihrd_particle;

// 256 lanes per block in the propagation, as in stoch_epi_step_kernel: the model step's registers (not the block) bound the
// waves per SIMD, and small blocks spread a chunk of few particles over more CUs.  1024 lanes in the normalisation: one
// workgroup owns a theta's row, and every round of the scans ends in one barrier, so the widest block makes the fewest strides.
constexpr int WIDE_STEP_BLOCK = 256, WIDE_SCAN_BLOCK = 1024, WIDE_FILL_BLOCK = 256, WIDE_FILL_SLICES = 32;
constexpr int WIDE_LDS_J = 1024;  // up to this J the four scan buffers are LDS (32 KiB), beyond it the scratch in device memory

// Where the particles of one chunk of Bc thetas live (the scratch of csrc/sepaihrd_particle_wide_device.h, doubles first).
struct ChunkScratch {
    double* lw;      // [Bc][J]
    double* C[2];    // [Bc][J] each
    double* Q[2];    // [Bc][J] each
    int32_t* anc;    // [Bc][J]
    int32_t* state;  // [2][Bc][11][J][lpc]
};
ChunkScratch carve(void* base, size_t Bc, int J) {
    const size_t row = Bc * (size_t)J;
    ChunkScratch s;
    s.lw = static_cast<double*>(base);
    s.C[0] = s.lw + row;
    s.C[1] = s.C[0] + row;
    s.Q[0] = s.C[1] + row;
    s.Q[1] = s.Q[0] + row;
    s.anc = reinterpret_cast<int32_t*>(s.Q[1] + row);
    s.state = s.anc + row;
    return s;
}

// ---- the outputs before the first segment: what a skipped row and an invalid theta leave
struct WideFill {
    int J, Tp, n;
    const int32_t* status;  // [B]
    double *loglik, *increments, *ess, *final_state;
};
// block (b, slice): loglik 0, every increment 0 and every ESS NaN for a valid theta (the weighted rows overwrite theirs);
// -DBL_MAX and NaN throughout for an invalid one, its final state included
__global__ __launch_bounds__(WIDE_FILL_BLOCK) void wide_fill_kernel(const WideFill f) {
    const size_t b = blockIdx.x;
    const size_t first = (size_t)blockIdx.y * WIDE_FILL_BLOCK + threadIdx.x, stride = (size_t)WIDE_FILL_SLICES * WIDE_FILL_BLOCK;
    const bool bad = f.status[b] != 0;
    const double qnan = __builtin_nan("");
    if (first == 0) f.loglik[b] = bad ? -DBL_MAX : 0.0;
    for (size_t t = first; t < (size_t)f.Tp; t += stride) {
        if (f.increments != nullptr) f.increments[b * f.Tp + t] = bad ? qnan : 0.0;
        if (f.ess != nullptr) f.ess[b * f.Tp + t] = qnan;
    }
    if (bad && f.final_state != nullptr) {
        const size_t final_doubles = (size_t)f.J * epi::NUM_COMP * f.n;
        for (size_t i = first; i < final_doubles; i += stride) f.final_state[b * final_doubles + i] = qnan;
    }
}

// ---- one segment of output rows k_first .. k_last of one chunk
struct WideSegment {
    int Bc, J, m, W;
    uint64_t seed;
    uint32_t b0;             // the chunk's first theta: its position in the call (the stream coordinate s of slot (bl, p) is b0 + bl)
    int k_first, k_last;     // k_first = 0: the particles start from the initial counts of their model-values row
    int cur;                 // the copy to read; the segment's end goes to copy cur ^ 1
    int gather;              // the previous segment ended in a resampling: slot p continues slot anc[p]
    int weighted;            // row k_last is weighted: lw is written
    const double* values;    // [Bc][W], the chunk's rows
    const int32_t* status;   // [Bc]
    int32_t* state;
    const int32_t* anc;
    double* lw;
};

// the dispersed instantiation's arguments: the segment and the three k, +inf where a series stays Poisson
struct WideSegmentNB : WideSegment {
    double k_H, k_ICU, k_D;
};

__device__ size_t state_index(int Bc, int J, int lpc, int copy, int bl, int c, int p, int age) {
    return particle_wide_state_index(Bc, J, lpc, copy, bl, c, p, age);
}

// One lane per (theta of the chunk, particle, age class), slots along bl J + p, the lpc lanes of a particle adjacent: in every
// load and store of a count consecutive lanes touch consecutive words (the gather through anc, non-decreasing in p, nearly so).
// The 11 counts stay in registers through the segment's rows; the previous-row CumH, CumICU and D of csrc/sepaihrd_particle.inc
// are the counts at the start of the segment's last interval (every row, weighted or not, takes the increments: the host twin's
// walk) and are never stored.  Lanes of padded ages, of invalid thetas and of the slots past the chunk's last carry zeros, take
// part in the exchanges, draw nothing (binomial(0, .) returns at once) and store nothing.
//
// NB = "some series is dispersed": the false instantiation is the Poisson kernel, argument for argument; the true one takes the
// three k in its argument struct and weighs each series by a kernel-uniform test on its k (pf::series_term).
template <bool NB>
__global__ __launch_bounds__(WIDE_STEP_BLOCK) void wide_propagate_kernel(const DevProblem pb, const std::conditional_t<NB, WideSegmentNB, WideSegment> s) {
    const int n = pb.n, lpc = pb.lpc, J = s.J;
    const size_t gl = (size_t)blockIdx.x * WIDE_STEP_BLOCK + threadIdx.x;
    const size_t idx = gl / (size_t)lpc;
    const int age = (int)(gl % (size_t)lpc);
    const bool in_range = idx < (size_t)s.Bc * (size_t)J;
    const int bl = in_range ? (int)(idx / (size_t)J) : 0;
    const int p = in_range ? (int)(idx % (size_t)J) : 0;
    const bool real_age = age < n;
    const bool ok = in_range && real_age && s.status[bl] == 0;
    const int row_age = real_age ? age : 0;  // padded lanes read age 0's entries and use none of them
    const epi::RowLayout L{n, pb.nb, pb.nk};
    const double* row = s.values + (size_t)bl * s.W;
    const uint32_t b = s.b0 + (uint32_t)bl;

    int32_t x[epi::NUM_COMP];
    if (s.k_first == 0) {
#pragma unroll
        for (int c = 0; c < epi::NUM_COMP; ++c) x[c] = ok ? (int32_t)row[L.initial(c, row_age)] : 0;
    } else {
        const int from = (ok && s.gather) ? s.anc[(size_t)bl * J + p] : p;
#pragma unroll
        for (int c = 0; c < epi::NUM_COMP; ++c) x[c] = ok ? s.state[state_index(s.Bc, J, lpc, s.cur, bl, c, from, age)] : 0;
    }
    const epi::LaneConstants lc = epi::lane_constants(row, L, pb.N, pb.Mrow, lpc, age);
    int32_t prevH = x[epi::C_CUM_H], prevICU = x[epi::C_CUM_ICU], prevD = x[epi::C_D];  // row 0: its increments are 0
    for (int k = s.k_first > 0 ? s.k_first : 1; k <= s.k_last; ++k) {
        prevH = x[epi::C_CUM_H]; prevICU = x[epi::C_CUM_ICU]; prevD = x[epi::C_D];
        const double t0 = pb.times[k - 1];
        const double h = (pb.times[k] - t0) / (double)s.m;
        const epi::AgeProbs q = epi::age_probs(row, L, row_age, h);
        epi::lane_interval(x, row, L, lc, pb.beta_ends, pb.kappa_ends, t0, h, q, s.m, s.seed, b, (uint32_t)p, (uint32_t)((k - 1) * s.m), (uint32_t)age,
                           [lpc](double inf, int jj) { return __shfl(inf, jj, lpc); });
    }
    if (ok) {
#pragma unroll
        for (int c = 0; c < epi::NUM_COMP; ++c) s.state[state_index(s.Bc, J, lpc, s.cur ^ 1, bl, c, p, age)] = x[c];
    }
    if (s.weighted) {  // uniform across the launch
        const double qnan = __builtin_nan("");
        double oH = qnan, oICU = qnan, oD = qnan;
        if (real_age) {
            const double* rec = pb.grid + ((size_t)s.k_last * lpc + age) * 4;  // {obs_H, obs_ICU, obs_D, times[k + 1]}
            oH = rec[0]; oICU = rec[1]; oD = rec[2];
        }
        double term;
        if constexpr (NB)
            term = pf::age_term(oH, oICU, oD, x[epi::C_CUM_H] - prevH, x[epi::C_CUM_ICU] - prevICU, x[epi::C_D] - prevD,
                                pf::Dispersion{s.k_H, s.k_ICU, s.k_D});
        else
            term = pf::age_term(oH, oICU, oD, x[epi::C_CUM_H] - prevH, x[epi::C_CUM_ICU] - prevICU, x[epi::C_D] - prevD);
        double lw = 0.0;
        for (int aa = 0; aa < n; ++aa) lw += __shfl(term, aa, lpc);
        if (ok && age == 0) s.lw[(size_t)bl * J + p] = lw;
    }
}

// ---- one weighted row of one chunk: the pointers are the chunk's (theta bl of the chunk at [bl][...])
struct WideRow {
    int J, Tp, t;            // t = k - runup_offset, the row of increments / ess
    uint64_t seed;
    uint32_t b0, k;          // the resampling uniform of theta bl is that of (seed, b0 + bl, k)
    const int32_t* status;   // [Bc]
    const double* lw;        // [Bc][J]
    double *C0, *C1, *Q0, *Q1;  // [Bc][J] each: used where J > WIDE_LDS_J
    int32_t* anc;            // [Bc][J]
    double* loglik;          // [Bc]: the running sum, in time order
    double* increments;      // [Bc][Tp] or null
    double* ess;             // [Bc][Tp] or null
    const double* row_const; // [Tp], the same for every theta: the row constants G of a dispersed call; null on the Poisson path
};

// One workgroup per theta of the chunk; lane i owns the elements i, i + 1024, ... of the row.  The maximum; w and w^2; the two
// inclusive scans in the Kogge-Stone order of csrc/sepaihrd_particle.inc (round d: new[j] = old[j] + old[j - d] for j >= d, else
// old[j]; the rounds ping-pong between two buffers and end in one barrier each -- the barrier also makes a wave's stores to
// device memory visible to the other waves of its workgroup); the increment and the ESS by lane 0; every ancestor by
// pf::ancestor on the final C.  The order of the additions is a function of J alone, so the sums are the bits of the LDS kernel's
// and of the host's.  An invalid theta's block returns at once: wide_fill_kernel wrote its rows.
__global__ __launch_bounds__(WIDE_SCAN_BLOCK) void wide_resample_kernel(const WideRow r) {
    __shared__ double red[WIDE_SCAN_BLOCK / WAVE];
    __shared__ double scan_lds[4][WIDE_LDS_J];
    const int bl = (int)blockIdx.x, tid = (int)threadIdx.x, J = r.J;
    if (r.status[bl] != 0) return;  // uniform across the block
    const size_t base = (size_t)bl * (size_t)J;
    const double* lw = r.lw + base;
    double mx = -__builtin_inf();
    for (int j = tid; j < J; j += WIDE_SCAN_BLOCK) {
        const double v = lw[j];
        mx = v > mx ? v : mx;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(mx, off, WAVE);
        mx = o > mx ? o : mx;
    }
    if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = mx;
    __syncthreads();
    double M = red[0];
    for (int w = 1; w < WIDE_SCAN_BLOCK / WAVE; ++w) M = red[w] > M ? red[w] : M;

    const bool in_lds = J <= WIDE_LDS_J;
    double* c_old = in_lds ? scan_lds[0] : r.C0 + base;
    double* c_new = in_lds ? scan_lds[1] : r.C1 + base;
    double* q_old = in_lds ? scan_lds[2] : r.Q0 + base;
    double* q_new = in_lds ? scan_lds[3] : r.Q1 + base;
    for (int j = tid; j < J; j += WIDE_SCAN_BLOCK) {
        const double w = pf::weight(lw[j], M);
        c_old[j] = w;
        q_old[j] = w * w;
    }
    __syncthreads();
    for (int d = 1; d < J; d <<= 1) {
        for (int j = tid; j < J; j += WIDE_SCAN_BLOCK) {
            double c = c_old[j], q = q_old[j];
            if (j >= d) {
                c += c_old[j - d];
                q += q_old[j - d];
            }
            c_new[j] = c;
            q_new[j] = q;
        }
        __syncthreads();
        double* sw = c_old; c_old = c_new; c_new = sw;
        sw = q_old; q_old = q_new; q_new = sw;
    }
    if (tid == 0) {
        double inc = pf::increment(M, c_old[J - 1], J);
        if (r.row_const != nullptr) inc = pf::increment_with_constant(inc, r.row_const[r.t]);
        r.loglik[bl] += inc;
        if (r.increments != nullptr) r.increments[(size_t)bl * r.Tp + r.t] = inc;
        if (r.ess != nullptr) r.ess[(size_t)bl * r.Tp + r.t] = pf::effective_sample_size(c_old[J - 1], q_old[J - 1]);
    }
    const double u = pf::resample_uniform(r.seed, r.b0 + (uint32_t)bl, r.k);
    for (int i = tid; i < J; i += WIDE_SCAN_BLOCK) r.anc[base + i] = pf::ancestor(c_old, J, u, i);
}

// ---- the particles after the last row: from copy `cur`, through anc where the last row was resampled
struct WideFinal {
    int Bc, J, cur, gather;
    const int32_t* status;   // [Bc]
    const int32_t* state;
    const int32_t* anc;
    double* final_state;     // [Bc][J][11][n], the chunk's
};
__global__ __launch_bounds__(WIDE_STEP_BLOCK) void wide_final_kernel(const DevProblem pb, const WideFinal f) {
    const int n = pb.n, lpc = pb.lpc, J = f.J;
    const size_t gl = (size_t)blockIdx.x * WIDE_STEP_BLOCK + threadIdx.x;
    const size_t idx = gl / (size_t)lpc;
    const int age = (int)(gl % (size_t)lpc);
    if (idx >= (size_t)f.Bc * (size_t)J || age >= n) return;
    const int bl = (int)(idx / (size_t)J), p = (int)(idx % (size_t)J);
    if (f.status[bl] != 0) return;  // NaN already (wide_fill_kernel)
    const int from = f.gather ? f.anc[idx] : p;
    double* dst = f.final_state + idx * (size_t)(epi::NUM_COMP * n) + age;
#pragma unroll
    for (int c = 0; c < epi::NUM_COMP; ++c) dst[(size_t)c * n] = (double)f.state[state_index(f.Bc, J, lpc, f.cur, bl, c, from, age)];
}

unsigned lane_blocks(size_t slots, int lpc) { return (unsigned)((slots * (size_t)lpc + WIDE_STEP_BLOCK - 1) / WIDE_STEP_BLOCK); }

void launch_row(const WideRow& r, int Bc, hipStream_t st) { hipLaunchKernelGGL(wide_resample_kernel, dim3((unsigned)Bc), dim3(WIDE_SCAN_BLOCK), 0, st, r); }

}  // namespace

int launch_particle_filter_wide(const DevProblem& pb, const ParticleWideArgs& a, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int T = pb.T, Tp = pb.T - pb.runup_offset, lpc = pb.lpc, J = a.J;
    if (a.B <= 0 || a.m < 1 || pb.n < 1 || pb.n > epi::MAX_AGES || lpc < pb.n || lpc > epi::MAX_AGES || (lpc & (lpc - 1)) != 0 || Tp <= 0 || J < 1 ||
        J > PARTICLE_WIDE_MAX_J || (uint64_t)a.B * (uint64_t)J >= ((uint64_t)1 << 31) || (uint64_t)T * (uint64_t)a.m >= ((uint64_t)1 << 22) ||
        a.W != epi::RowLayout{pb.n, pb.nb, pb.nk}.width() || a.chunk < 1 || a.chunk > (size_t)a.B || !a.scratch || !a.host_grid || !a.values ||
        !a.status || !a.loglik)
        return -4;
    // a row is weighted when t >= 0 and one of its cells is usable: known from the observations alone
    std::vector<uint8_t> weighted((size_t)T, 0);
    for (int k = pb.runup_offset; k < T; ++k)
        for (int i = 0; i < pb.n; ++i) {
            const double* rec = a.host_grid + ((size_t)k * lpc + i) * 4;
            if (pf::usable(rec[0]) || pf::usable(rec[1]) || pf::usable(rec[2])) weighted[(size_t)k] = 1;
        }
    const size_t final_doubles = (size_t)J * epi::NUM_COMP * pb.n;
    const bool nb = a.row_const != nullptr;
    if (nb && !pf::any_dispersed(pf::Dispersion{a.k_H, a.k_ICU, a.k_D})) return -4;
    if (a.states != nullptr && prepare_particle_states(J) != 0) return -3;
    WideFill f{J, Tp, pb.n, a.status, a.loglik, a.increments, a.ess, a.final_state};
    hipLaunchKernelGGL(wide_fill_kernel, dim3((unsigned)a.B, WIDE_FILL_SLICES), dim3(WIDE_FILL_BLOCK), 0, st, f);
    for (size_t b0 = 0; b0 < (size_t)a.B; b0 += a.chunk) {
        const int Bc = (int)std::min(a.chunk, (size_t)a.B - b0);
        const ChunkScratch sc = carve(a.scratch, (size_t)Bc, J);
        const size_t slots = (size_t)Bc * (size_t)J;
        WideSegmentNB s{};
        s.k_H = a.k_H; s.k_ICU = a.k_ICU; s.k_D = a.k_D;
        s.Bc = Bc; s.J = J; s.m = a.m; s.W = a.W;
        s.seed = a.seed;
        s.b0 = (uint32_t)b0;
        s.values = a.values + b0 * (size_t)a.W; s.status = a.status + b0;
        s.state = sc.state; s.anc = sc.anc; s.lw = sc.lw;
        WideRow r{};
        r.J = J; r.Tp = Tp;
        r.seed = a.seed;
        r.b0 = (uint32_t)b0;
        r.status = s.status; r.lw = sc.lw;
        r.C0 = sc.C[0]; r.C1 = sc.C[1]; r.Q0 = sc.Q[0]; r.Q1 = sc.Q[1];
        r.anc = sc.anc;
        r.loglik = a.loglik + b0;
        r.increments = a.increments ? a.increments + b0 * (size_t)Tp : nullptr;
        r.ess = a.ess ? a.ess + b0 * (size_t)Tp : nullptr;
        r.row_const = a.row_const;
        int cur = 0, gather = 0;
        for (int k = 0; k < T;) {
            int k_last = k;
            while (a.states == nullptr && !weighted[(size_t)k_last] && k_last + 1 < T) ++k_last;
            s.k_first = k; s.k_last = k_last;
            s.cur = cur; s.gather = gather; s.weighted = weighted[(size_t)k_last];
            if (nb)
                hipLaunchKernelGGL(wide_propagate_kernel<true>, dim3(lane_blocks(slots, lpc)), dim3(WIDE_STEP_BLOCK), 0, st, pb, s);
            else
                hipLaunchKernelGGL(wide_propagate_kernel<false>, dim3(lane_blocks(slots, lpc)), dim3(WIDE_STEP_BLOCK), 0, st, pb,
                                   static_cast<const WideSegment&>(s));
            cur ^= 1;
            gather = 0;
            if (s.weighted) {
                r.k = (uint32_t)k_last; r.t = k_last - pb.runup_offset;
                launch_row(r, Bc, st);
                gather = 1;
            }
            if (hipGetLastError() != hipSuccess) return -3;
            if (a.states != nullptr) {  // k_last == k: the row's cloud is copy cur, through anc where the row was resampled
                const int src = launch_particle_states_row(pb, *a.states, Bc, b0, J, k, cur, gather, sc.state, sc.anc, s.status, st);
                if (src != 0) return src;
            }
            k = k_last + 1;
        }
        if (a.final_state != nullptr) {
            WideFinal fin{Bc, J, cur, gather, s.status, sc.state, sc.anc, a.final_state + b0 * final_doubles};
            hipLaunchKernelGGL(wide_final_kernel, dim3(lane_blocks(slots, lpc)), dim3(WIDE_STEP_BLOCK), 0, st, pb, fin);
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd

using namespace sepaihrd;

extern "C" int sepaihrd_particle_wide_max_particles(void) { return PARTICLE_WIDE_MAX_J; }

extern "C" int sepaihrd_particle_wide_validate(int B, int J, int steps_per_interval, int theta_chunk, int n_times, int T_pos, int n_age, char* err,
                                               int errlen) {
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, "particle_loglik_wide: " + msg); return SEPAIHRD_E_INVALID_ARG; };
    if (B < 1) return refuse("B must be >= 1 (parameter vectors)");
    if (n_age < 1 || n_age > sepaihrd_stoch_epi::MAX_AGES) return refuse("n_age must lie in [1, 16]");
    if (J < 1 || J > PARTICLE_WIDE_MAX_J) return refuse("J must lie in [1, 65536] (particles per parameter vector, in device memory)");
    if (theta_chunk < 0) return refuse("theta_chunk must be >= 0 (parameter vectors per pass through the scratch; 0: chosen by the call)");
    if (const char* grid = stoch_epi_grid_refusal(steps_per_interval, n_times, T_pos, n_age)) return refuse(grid);
    if ((uint64_t)B * (uint64_t)J >= ((uint64_t)1 << 31)) return refuse("B x J must stay below 2^31 (particles per call)");
    return SEPAIHRD_OK;
}

// One weighted row through wide_resample_kernel: a chunk of one theta whose position in the call is b.
extern "C" int sepaihrd_particle_wide_resample_device(int device, uint64_t seed, uint32_t b, uint32_t row, const double* logw, int J,
                                                      int32_t* ancestors, double* increment, double* ess, char* err, int errlen) {
    if (!logw || !ancestors || !increment || !ess || J < 1 || J > PARTICLE_WIDE_MAX_J) {
        set_err(err, errlen, "particle_wide_resample_device: need logw, ancestors, increment, ess and J in [1, 65536]");
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (const int drc = select_device(device, err, errlen)) return drc;
    Probe pr;
    double out3[3] = {0.0, 0.0, 0.0};  // {the running sum, increment, ESS}
    const int32_t valid = 0;
    const double* d_logw = pr.in(logw, (size_t)J);
    double *d_scan = pr.out<double>((size_t)4 * J), *d_out3 = pr.in(out3, 3);
    int32_t* d_anc = pr.out<int32_t>((size_t)J);
    const int32_t* d_status = pr.in(&valid, 1);
    if (pr.ready()) {
        WideRow r{};
        r.J = J; r.Tp = 1; r.t = 0;
        r.seed = seed;
        r.b0 = b; r.k = row;
        r.status = d_status; r.lw = d_logw;
        r.C0 = d_scan; r.C1 = d_scan + J; r.Q0 = d_scan + (size_t)2 * J; r.Q1 = d_scan + (size_t)3 * J;
        r.anc = d_anc;
        r.loglik = d_out3; r.increments = d_out3 + 1; r.ess = d_out3 + 2;
        launch_row(r, 1, nullptr);
        pr.fetch(ancestors, d_anc, (size_t)J);
        pr.fetch(out3, d_out3, 3);
    }
    if (const int prc = pr.status("particle_wide_resample_device", err, errlen)) return prc;
    *increment = out3[1];
    *ess = out3[2];
    return SEPAIHRD_OK;
}
