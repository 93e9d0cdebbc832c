// csrc/sepaihrd_particle_states.hip -- the per-row summaries of the wide particle filter on gfx950
// (sepaihrd_particle_filter_states): after every output row the filtered means and quantile bands of the
// 11 counts per age class and of their age totals, over the J particles the next interval starts from.  The rule is
// csrc/sepaihrd_particle_states.inc, the text the host twin compiles too; the filter is csrc/sepaihrd_particle_wide.hip's,
// which calls launch_particle_states_row between its own launches.  Plain launches on one stream: no cooperative launch, no
// barrier across workgroups, no synchronisation.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "sepaihrd_bitonic.inc"
#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_particle_states.inc"
#include "sepaihrd_particle_states_device.h"
#include "sepaihrd_stoch_sepaihrd_device.h"

namespace sepaihrd {
namespace {

namespace epi = sepaihrd_stoch_epi;
namespace ps = sepaihrd_particle_states;

constexpr int STATES_GATHER_BLOCK = 256, STATES_SORT_BLOCK = 1024;

struct StatesRow {
    int Bc, J, n, lpc, pad, T, k, cur, gather, n_probs;
    const int32_t* state;   // the chunk's two copies
    const int32_t* anc;     // [Bc][J]
    const int32_t* status;  // [Bc]
    const double* probs;    // [n_probs]
    double* table;          // [Bc][11][n + 1][pad]
    double* mean;           // the chunk's [Bc][T][11][n + 1]
    double* quantiles;      // the chunk's [Bc][T][11][n + 1][n_probs] or null
};

// One lane per (theta of the chunk, particle, age class), the lpc lanes of a particle adjacent as in wide_propagate_kernel.  A
// lane reads its 11 counts at slot anc[p] (p after an unweighted row), forms the age total by integer exchanges of width lpc
// and stores the values as doubles, the particle index contiguous; lane `age == 0` stores the total.  Lanes of padded ages, of
// invalid thetas and past the chunk's last slot carry zeros, take part in the exchanges and store nothing.
__global__ __launch_bounds__(STATES_GATHER_BLOCK) void states_gather_kernel(const StatesRow r) {
    const int n = r.n, lpc = r.lpc, J = r.J;
    const size_t gl = (size_t)blockIdx.x * STATES_GATHER_BLOCK + threadIdx.x;
    const size_t idx = gl / (size_t)lpc;
    const int age = (int)(gl % (size_t)lpc);
    const bool in_range = idx < (size_t)r.Bc * (size_t)J;
    const int bl = in_range ? (int)(idx / (size_t)J) : 0;
    const int p = in_range ? (int)(idx % (size_t)J) : 0;
    const bool ok = in_range && age < n && r.status[bl] == 0;
    const int from = (ok && r.gather) ? r.anc[(size_t)bl * J + p] : p;
    double* seg = r.table + (size_t)bl * epi::NUM_COMP * (size_t)(n + 1) * (size_t)r.pad + p;
#pragma unroll
    for (int c = 0; c < epi::NUM_COMP; ++c) {
        const int32_t x = ok ? r.state[particle_wide_state_index(r.Bc, J, lpc, r.cur, bl, c, from, age)] : 0;
        long long total = 0;
        for (int aa = 0; aa < n; ++aa) total += (long long)__shfl(x, aa, lpc);
        if (ok) {
            seg[((size_t)c * (n + 1) + age) * (size_t)r.pad] = (double)x;
            if (age == 0) seg[((size_t)c * (n + 1) + n) * (size_t)r.pad] = (double)total;
        }
    }
}

// One workgroup per (theta of the chunk, count, series).  The J values of the segment, +inf up to the power of two Np = pad,
// are sorted ascending by the bitonic network of csrc/sepaihrd_bitonic.inc -- in LDS where Np <= ENSEMBLE_MAX_SAMPLES, in the
// segment itself beyond.  The sum is taken in 64-bit integers before the sort.  Thread 0 writes the mean, thread p quantile p.
// An invalid theta's workgroup writes NaN.
__global__ __launch_bounds__(STATES_SORT_BLOCK) void states_sort_pick_kernel(const StatesRow r) {
    extern __shared__ double lds_seg[];
    __shared__ long long part[STATES_SORT_BLOCK / WAVE];
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x, J = r.J, Np = r.pad;
    const int series = r.n + 1;
    const size_t sid = blockIdx.x;  // (bl 11 + c) (n + 1) + a
    const int bl = (int)(sid / ((size_t)epi::NUM_COMP * series));
    const size_t cell = sid % ((size_t)epi::NUM_COMP * series);
    double* mean = r.mean + ((size_t)bl * r.T + r.k) * epi::NUM_COMP * series + cell;
    double* q = r.quantiles ? r.quantiles + (((size_t)bl * r.T + r.k) * epi::NUM_COMP * series + cell) * r.n_probs : nullptr;
    if (r.status[bl] != 0) {  // uniform across the block
        if (tid == 0) *mean = __builtin_nan("");
        if (q != nullptr)
            for (int p = tid; p < r.n_probs; p += BS) q[p] = __builtin_nan("");
        return;
    }
    double* src = r.table + sid * (size_t)Np;
    const bool in_lds = Np <= ENSEMBLE_MAX_SAMPLES;
    double* seg = in_lds ? lds_seg : src;
    long long sum = 0;
    for (int i = tid; i < Np; i += BS) {
        const double v = i < J ? src[i] : __builtin_inf();
        if (i < J) sum += (long long)v;
        seg[i] = v;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, WAVE);
    if ((tid & (WAVE - 1)) == 0) part[tid / WAVE] = sum;
    __syncthreads();
    bitonic_sort_pow2(seg, Np);
    if (tid == 0) {
        long long total = 0;
        for (int w = 0; w < (BS + WAVE - 1) / WAVE; ++w) total += part[w];
        *mean = ps::mean_of((int64_t)total, J);
    }
    if (q != nullptr)
        for (int p = tid; p < r.n_probs; p += BS) q[p] = sepaihrd_quantile::sorted_quantile(seg, (size_t)J, r.probs[p]);
}

// the dynamic LDS of the sort of `pad` doubles: the segment where it is sorted in LDS, nothing where it is sorted in place
size_t sort_lds_bytes(size_t pad) { return pad <= (size_t)ENSEMBLE_MAX_SAMPLES ? pad * sizeof(double) : 0; }

}  // namespace

int prepare_particle_states(int J) {
    const size_t lds = sort_lds_bytes(particle_states_pad(J));
    if (lds <= 48 * 1024) return 0;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&states_sort_pick_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess
               ? 0
               : -3;
}

int launch_particle_states_row(const DevProblem& pb, ParticleStatesArgs& a, int Bc, size_t b0, int J, int k, int cur, int gather,
                               const int32_t* state, const int32_t* anc, const int32_t* status, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = pb.n, lpc = pb.lpc, T = pb.T, series = n + 1;
    if (Bc < 1 || J < 1 || J > PARTICLE_WIDE_MAX_J || n < 1 || n > epi::MAX_AGES || lpc < n || lpc > epi::MAX_AGES || (lpc & (lpc - 1)) != 0 || k < 0 ||
        k >= T || a.n_probs < 0 || a.n_probs > ps::MAX_PROBS || (a.n_probs > 0 && !a.probs) || (a.state_quantiles && a.n_probs == 0) || !a.table ||
        !a.state_mean || !state || !anc || !status)
        return -4;
    const size_t pad = particle_states_pad(J);
    const size_t row_doubles = (size_t)T * epi::NUM_COMP * series;
    StatesRow r{};
    r.Bc = Bc; r.J = J; r.n = n; r.lpc = lpc; r.pad = (int)pad; r.T = T; r.k = k; r.cur = cur; r.gather = gather; r.n_probs = a.n_probs;
    r.state = state; r.anc = anc; r.status = status; r.probs = a.probs; r.table = a.table;
    r.mean = a.state_mean + b0 * row_doubles;
    r.quantiles = a.state_quantiles ? a.state_quantiles + b0 * row_doubles * (size_t)a.n_probs : nullptr;
    const bool timed = b0 == 0 && a.ev != nullptr && a.used_ev + 2 <= a.n_ev;  // the first chunk's summaries alone
    if (timed) (void)hipEventRecord(static_cast<hipEvent_t>(a.ev[a.used_ev]), st);
    const size_t lanes = (size_t)Bc * (size_t)J * (size_t)lpc;
    hipLaunchKernelGGL(states_gather_kernel, dim3((unsigned)((lanes + STATES_GATHER_BLOCK - 1) / STATES_GATHER_BLOCK)), dim3(STATES_GATHER_BLOCK), 0, st,
                       r);
    const size_t lds = sort_lds_bytes(pad);  // above 48 KiB: prepare_particle_states has raised the kernel's limit
    const int threads = pad / 2 < (size_t)STATES_SORT_BLOCK ? (int)(pad / 2 < (size_t)WAVE ? (size_t)WAVE : pad / 2) : STATES_SORT_BLOCK;  // whole wavefronts
    hipLaunchKernelGGL(states_sort_pick_kernel, dim3((unsigned)((size_t)Bc * epi::NUM_COMP * series)), dim3(threads), lds, st, r);
    if (timed) {
        (void)hipEventRecord(static_cast<hipEvent_t>(a.ev[a.used_ev + 1]), st);
        a.used_ev += 2;
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sepaihrd

using namespace sepaihrd;

extern "C" int sepaihrd_particle_states_validate(int B, int J, int steps_per_interval, int theta_chunk, int n_times, int T_pos, int n_age,
                                                 const double* probs, int n_probs, char* err, int errlen) {
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, "particle_filter_states: " + msg); return SEPAIHRD_E_INVALID_ARG; };
    char msg[256] = "";
    if (sepaihrd_particle_wide_validate(B, J, steps_per_interval, theta_chunk, n_times, T_pos, n_age, msg, (int)sizeof(msg)) != SEPAIHRD_OK) {
        // the wide form's rule under this entry's name
        const std::string text = msg, prefix = "particle_loglik_wide: ";
        return refuse(text.compare(0, prefix.size(), prefix) == 0 ? text.substr(prefix.size()) : text);
    }
    if (n_probs < 0 || n_probs > sepaihrd_particle_states::MAX_PROBS) return refuse("n_probs must lie in [0, 64] (quantile probabilities)");
    if (n_probs > 0 && !probs) return refuse("n_probs > 0 needs probs");
    for (int i = 0; i < n_probs; ++i)
        if (!sepaihrd_particle_states::probability_ok(probs[i])) return refuse("every probability must lie in [0, 1]");
    return SEPAIHRD_OK;
}
