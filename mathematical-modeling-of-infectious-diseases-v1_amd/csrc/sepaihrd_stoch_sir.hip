// csrc/sepaihrd_stoch_sir.hip -- stochastic chain-binomial SIR ensembles on gfx950 (sepaihrd_stoch_sir_*; DESIGN.md
// section 6h): the step kernel, the probe of the binomial sampler and their C ABI.  The model, the stream and the sampler
// are csrc/sepaihrd_stoch.inc, the text the host twin compiles too; the segment sorts and the summaries are
// csrc/sepaihrd_ensemble.hip's.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"
#include "sepaihrd_host_util.h"
#include "sepaihrd_segments.h"
#include "sepaihrd_stoch.inc"
#include "sepaihrd_stoch_device.h"

namespace sepaihrd {
namespace {

using sepaihrd_stoch::Group;
static_assert(sizeof(Group) == sizeof(sepaihrd_stoch_sir_group), "the kernel reads the C ABI's group table in place");

constexpr int STEP_BLOCK = 256;

struct StochStepArgs {
    const Group* groups;   // [G]
    double* state;         // [G][3][R_pad]: row `step0` of every replicate on entry, row step0 + chunk_steps on exit
    double* vals;          // [G][3][chunk_steps][R_pad], replicate fastest; lanes R .. R_pad - 1 hold +inf
    uint64_t seed;
    double h;
    int G, R, R_pad;
    int step0, chunk_steps, steps;
};

// One lane per replicate, groups stacked in the grid's y dimension.  Rows step0 .. step0 + chunk_steps - 1 are stored, each
// store of a wavefront 512 contiguous bytes; the state after the chunk's last row goes back to `state` for the next chunk.
__global__ __launch_bounds__(STEP_BLOCK) void stoch_sir_step_kernel(const StochStepArgs a) {
    const int r = (int)(blockIdx.x * (unsigned)STEP_BLOCK + threadIdx.x);
    if (r >= a.R_pad) return;
    const int stride_blocks = (int)gridDim.y;
    for (int g = (int)blockIdx.y; g < a.G; g += stride_blocks) {
        double* out = a.vals + (size_t)g * 3 * (size_t)a.chunk_steps * (size_t)a.R_pad + (size_t)r;
        const size_t comp_stride = (size_t)a.chunk_steps * (size_t)a.R_pad;
        if (r >= a.R) {  // the padding sorts last
            for (int s = 0; s < a.chunk_steps; ++s)
                for (int c = 0; c < 3; ++c) out[(size_t)c * comp_stride + (size_t)s * a.R_pad] = INFINITY;
            continue;
        }
        const Group grp = a.groups[g];
        const double pR = sepaihrd_stoch::recovery_probability(grp.gamma, a.h);
        double* st = a.state + (size_t)g * 3 * (size_t)a.R_pad + (size_t)r;
        double S = st[0], I = st[(size_t)a.R_pad], R = st[2 * (size_t)a.R_pad];
        for (int s = 0; s < a.chunk_steps; ++s) {
            double* row = out + (size_t)s * a.R_pad;
            row[0] = S;
            row[comp_stride] = I;
            row[2 * comp_stride] = R;
            const int step = a.step0 + s;
            if (step < a.steps - 1) sepaihrd_stoch::sir_step(S, I, R, grp, a.h, pR, a.seed, (uint32_t)g, (uint32_t)r, (uint32_t)step);
        }
        st[0] = S;
        st[(size_t)a.R_pad] = I;
        st[2 * (size_t)a.R_pad] = R;
    }
}

__global__ __launch_bounds__(STEP_BLOCK) void stoch_sir_init_kernel(const Group* groups, double* state, int G, int R_pad) {
    const size_t idx = (size_t)blockIdx.x * STEP_BLOCK + threadIdx.x;
    if (idx >= (size_t)G * R_pad) return;
    const size_t g = idx / (size_t)R_pad, r = idx % (size_t)R_pad;
    const Group grp = groups[g];
    double* st = state + g * 3 * (size_t)R_pad + r;
    st[0] = grp.S0;
    st[(size_t)R_pad] = grp.I0;
    st[2 * (size_t)R_pad] = grp.R0;
}

__global__ __launch_bounds__(STEP_BLOCK) void stoch_binomial_probe_kernel(uint64_t seed, const int32_t* n, const double* p, int count,
                                                                           int32_t* out) {
    const int i = (int)(blockIdx.x * (unsigned)STEP_BLOCK + threadIdx.x);
    if (i >= count) return;
    sepaihrd_stoch::Coord c;
    c.seed = seed; c.group = 0; c.replicate = (uint32_t)i; c.step = 0; c.transition = sepaihrd_stoch::TRANSITION_INFECTION;
    out[i] = sepaihrd_stoch::binomial(c, n[i], p[i]);
}

}  // namespace
}  // namespace sepaihrd

using namespace sepaihrd;

extern "C" {

int64_t sepaihrd_stoch_sir_num_steps(double t_start, double t_end, double h) {
    if (!std::isfinite(t_start) || !std::isfinite(t_end) || !std::isfinite(h) || !(h > 0.0) || !(t_end > t_start)) return SEPAIHRD_E_INVALID_ARG;
    const double n = std::round((t_end - t_start) / h) + 1.0;
    if (!(n >= 1.0) || n > 2147483647.0) return SEPAIHRD_E_INVALID_ARG;
    return (int64_t)n;
}

int sepaihrd_stoch_sir_validate(const sepaihrd_stoch_sir_config* cfg, const sepaihrd_stoch_sir_group* groups, char* err, int errlen) {
    const std::string who = "stoch_sir: ";
    auto refuse = [&](const std::string& msg) { set_err(err, errlen, who + msg); return SEPAIHRD_E_INVALID_ARG; };
    if (!cfg || !groups) return refuse("config and groups must not be NULL");
    if (cfg->abi_version != SEPAIHRD_ABI_VERSION) return refuse("abi_version " + std::to_string(cfg->abi_version) + " is not " + std::to_string(SEPAIHRD_ABI_VERSION));
    if (!std::isfinite(cfg->t_start) || !std::isfinite(cfg->t_end) || !std::isfinite(cfg->h)) return refuse("t_start, t_end and h must be finite");
    if (!(cfg->h > 0.0)) return refuse("h must be > 0");
    if (!(cfg->t_end > cfg->t_start)) return refuse("t_end must be > t_start");
    if (cfg->n_replicates < 1) return refuse("at least one replicate is needed");
    if (cfg->n_replicates > SEPAIHRD_STOCH_SIR_MAX_REPLICATES) return refuse("n_replicates beyond " + std::to_string(SEPAIHRD_STOCH_SIR_MAX_REPLICATES));
    if (cfg->n_groups < 1 || cfg->n_groups > (1 << 30)) return refuse("n_groups must lie in [1, 2^30]");
    if (cfg->keep < 0 || cfg->keep > cfg->n_replicates) return refuse("keep must lie in [0, n_replicates]");
    if (sepaihrd_stoch_sir_num_steps(cfg->t_start, cfg->t_end, cfg->h) < 1) return refuse("t_start, t_end and h give more than 2^31 - 1 steps");
    for (int g = 0; g < cfg->n_groups; ++g) {
        const sepaihrd_stoch_sir_group& p = groups[g];
        const std::string grp = "group " + std::to_string(g) + ": ";
        const double v[6] = {p.N, p.beta, p.gamma, p.S0, p.I0, p.R0};
        for (double x : v) if (!std::isfinite(x)) return refuse(grp + "N, beta, gamma, S0, I0 and R0 must be finite");
        if (!(p.N > 0.0)) return refuse(grp + "N must be > 0");
        if (p.beta < 0.0 || p.gamma < 0.0 || p.S0 < 0.0 || p.I0 < 0.0 || p.R0 < 0.0) return refuse(grp + "beta, gamma, S0, I0 and R0 must be >= 0");
        if (std::fabs((p.S0 + p.I0 + p.R0) - p.N) > 1e-6 * p.N) return refuse(grp + "Initial compartments S0+I0+R0 must sum to N.");
        if (p.N > 2147483647.0) return refuse(grp + "N beyond 2^31 - 1 (the compartments are int)");
        if (std::round(p.S0) + std::round(p.I0) > 2147483647.0) return refuse(grp + "round(S0) + round(I0) beyond 2^31 - 1 (the compartments are int)");
    }
    return SEPAIHRD_OK;
}

int sepaihrd_stoch_sir_run(int device, const sepaihrd_stoch_sir_config* cfg, const sepaihrd_stoch_sir_group* groups, double* stats,
                           double* traj, double* final_state, double* phase_ms, char* err, int errlen) {
    const int vrc = sepaihrd_stoch_sir_validate(cfg, groups, err, errlen);
    if (vrc != SEPAIHRD_OK) return vrc;
    if (!stats) { set_err(err, errlen, "stoch_sir: stats must not be NULL"); return SEPAIHRD_E_INVALID_ARG; }
    if (cfg->keep > 0 && !traj) { set_err(err, errlen, "stoch_sir: keep > 0 needs traj"); return SEPAIHRD_E_INVALID_ARG; }
    const int G = cfg->n_groups, R = cfg->n_replicates, keep = traj ? cfg->keep : 0;
    const int steps = (int)sepaihrd_stoch_sir_num_steps(cfg->t_start, cfg->t_end, cfg->h);
    const SegmentPlan plan = plan_segments((size_t)R);  // a segment: the R replicates of one (group, compartment, step)
    const int R_pad = (int)plan.pad;
    const bool in_lds = plan.in_lds;
    // a step of the chunk: G x 3 rows of R_pad doubles, and as much again of sort scratch beyond the LDS sort
    const uint64_t budget = cfg->max_workspace_bytes ? cfg->max_workspace_bytes : SEPAIHRD_STOCH_SIR_DEFAULT_WORKSPACE;
    const uint64_t step_bytes = (uint64_t)G * 3 * (uint64_t)R_pad * sizeof(double) * (in_lds ? 1 : 2);
    uint64_t cs64 = budget / step_bytes;
    if (cs64 < 1) cs64 = 1;
    if (cs64 > (uint64_t)steps) cs64 = (uint64_t)steps;
    const uint64_t max_segments = ((uint64_t)1 << 31) - 1;  // the summaries index segments with int
    if ((uint64_t)G * 3 * cs64 > max_segments) cs64 = max_segments / ((uint64_t)G * 3);
    if (cs64 < 1) { set_err(err, errlen, "stoch_sir: too many groups for one chunk"); return SEPAIHRD_E_INVALID_ARG; }
    const int cs = (int)cs64;

    const int drc = select_device(device, err, errlen);
    if (drc != SEPAIHRD_OK) return drc;
    CallScratch sc(5);
    auto hip_fail = [&](const char* what) {
        set_err(err, errlen, std::string("stoch_sir: ") + what + ": " + hipGetErrorString(hipGetLastError()));
        return SEPAIHRD_E_HIP;
    };
    if (hipStreamCreate(&sc.stream) != hipSuccess) return hip_fail("hipStreamCreate");
    for (Event& e : sc.ev) if (hipEventCreate(&e) != hipSuccess) return hip_fail("hipEventCreate");
    hipStream_t st = sc.stream;

    Group* d_groups = nullptr;
    double *d_state = nullptr, *d_vals = nullptr, *d_stats = nullptr, *d_sort = nullptr;
    const size_t chunk_doubles = (size_t)G * 3 * (size_t)cs * (size_t)R_pad;
    size_t sort_doubles = 0;
    if (!in_lds) {  // the segmented sort takes groups of segments of fewer than 2^31 keys
        const size_t cap = (((size_t)1 << 31) - 1) / (size_t)R_pad * (size_t)R_pad;
        sort_doubles = chunk_doubles < cap ? chunk_doubles : cap;
    }
    if (!sc.alloc(&d_groups, (size_t)G) || !sc.alloc(&d_state, (size_t)G * 3 * R_pad) || !sc.alloc(&d_vals, chunk_doubles) ||
        !sc.alloc(&d_stats, (size_t)G * 12 * steps) || (!in_lds && !sc.alloc(&d_sort, sort_doubles))) {
        set_err(err, errlen, "stoch_sir: device allocation failed (lower max_workspace_bytes)");
        return SEPAIHRD_E_HIP;
    }
    if (hipMemcpyAsync(d_groups, groups, (size_t)G * sizeof(Group), hipMemcpyHostToDevice, st) != hipSuccess) return hip_fail("hipMemcpyAsync");
    hipLaunchKernelGGL(stoch_sir_init_kernel, dim3((unsigned)(((size_t)G * R_pad + STEP_BLOCK - 1) / STEP_BLOCK)), dim3(STEP_BLOCK), 0, st,
                       d_groups, d_state, G, R_pad);

    std::vector<double> stage;  // [G 3 cs][keep]: the kept replicates of a chunk, transposed into traj on the host
    if (keep > 0) stage.resize((size_t)G * 3 * (size_t)cs * (size_t)keep);
    double ms_acc[3] = {0.0, 0.0, 0.0};
    const unsigned grid_y = (unsigned)(G < 65535 ? G : 65535);
    for (int step0 = 0; step0 < steps; step0 += cs) {
        const int n = steps - step0 < cs ? steps - step0 : cs;
        StochStepArgs a{};
        a.groups = d_groups; a.state = d_state; a.vals = d_vals; a.seed = cfg->seed; a.h = cfg->h;
        a.G = G; a.R = R; a.R_pad = R_pad; a.step0 = step0; a.chunk_steps = n; a.steps = steps;
        (void)hipEventRecord(sc.ev[0], st);
        hipLaunchKernelGGL(stoch_sir_step_kernel, dim3((unsigned)((R_pad + STEP_BLOCK - 1) / STEP_BLOCK), grid_y), dim3(STEP_BLOCK), 0, st, a);
        (void)hipEventRecord(sc.ev[1], st);
        if (hipGetLastError() != hipSuccess) return hip_fail("step kernel launch");
        StochSummaryArgs s{};
        s.G = G; s.R = R; s.R_pad = R_pad; s.chunk_steps = n; s.step0 = step0; s.steps = steps;
        s.vals = d_vals; s.stats = d_stats; s.sort_scratch = d_sort; s.sort_scratch_doubles = sort_doubles;
        double summary_ms = 0.0;
        if (phase_ms) { s.ev[0] = sc.ev[3]; s.ev[1] = sc.ev[4]; s.summary_ms = &summary_ms; }
        const int rc = launch_stoch_sir_summaries(s, st);
        if (rc != 0) {
            set_err(err, errlen, "stoch_sir: the summaries failed (" + std::to_string(rc) + "): " + hipGetErrorString(hipGetLastError()));
            return rc == -4 ? SEPAIHRD_E_UNSUPPORTED : SEPAIHRD_E_HIP;
        }
        (void)hipEventRecord(sc.ev[2], st);
        if (keep > 0) {
            // rows of the chunk buffer are R_pad apart; the first `keep` doubles of each
            if (hipMemcpy2DAsync(stage.data(), (size_t)keep * sizeof(double), d_vals, (size_t)R_pad * sizeof(double), (size_t)keep * sizeof(double),
                                 (size_t)G * 3 * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess)
                return hip_fail("hipMemcpy2DAsync");
        }
        if (hipStreamSynchronize(st) != hipSuccess) return hip_fail("a kernel of this chunk failed");
        if (phase_ms) {
            float t_step = 0.0f, t_rest = 0.0f;
            (void)hipEventElapsedTime(&t_step, sc.ev[0], sc.ev[1]);
            (void)hipEventElapsedTime(&t_rest, sc.ev[1], sc.ev[2]);
            ms_acc[0] += t_step;
            ms_acc[1] += (double)t_rest - summary_ms;
            ms_acc[2] += summary_ms;
        }
        for (int g = 0; g < G && keep > 0; ++g)
            for (int c = 0; c < 3; ++c)
                for (int s2 = 0; s2 < n; ++s2) {
                    const double* row = stage.data() + (((size_t)g * 3 + c) * (size_t)n + s2) * (size_t)keep;
                    for (int k = 0; k < keep; ++k) traj[(((size_t)g * keep + k) * 3 + c) * (size_t)steps + (size_t)(step0 + s2)] = row[k];
                }
    }
    if (hipMemcpy(stats, d_stats, (size_t)G * 12 * steps * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return hip_fail("hipMemcpy(stats)");
    if (final_state) {
        std::vector<double> fs((size_t)G * 3 * R_pad);
        if (hipMemcpy(fs.data(), d_state, fs.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return hip_fail("hipMemcpy(state)");
        for (int g = 0; g < G; ++g)
            for (int r = 0; r < R; ++r)
                for (int c = 0; c < 3; ++c) final_state[((size_t)g * R + r) * 3 + c] = fs[((size_t)g * 3 + c) * R_pad + r];
    }
    if (phase_ms) for (int i = 0; i < 3; ++i) phase_ms[i] = ms_acc[i];
    return SEPAIHRD_OK;
}

int sepaihrd_stoch_sir_binomial_device(int device, uint64_t seed, const int32_t* n, const double* p, int count, int32_t* out, char* err,
                                       int errlen) {
    if (!n || !p || !out || count < 1) { set_err(err, errlen, "stoch_sir_binomial_device: need n, p, out and count >= 1"); return SEPAIHRD_E_INVALID_ARG; }
    for (int i = 0; i < count; ++i)
        if (n[i] < 0 || std::isnan(p[i])) { set_err(err, errlen, "stoch_sir_binomial_device: n must be >= 0 and p a number"); return SEPAIHRD_E_INVALID_ARG; }
    const int drc = select_device(device, err, errlen);
    if (drc != SEPAIHRD_OK) return drc;
    Probe pr;
    const int32_t* d_n = pr.in(n, (size_t)count);
    const double* d_p = pr.in(p, (size_t)count);
    int32_t* d_out = pr.out<int32_t>((size_t)count);
    if (pr.ready()) {
        hipLaunchKernelGGL(stoch_binomial_probe_kernel, dim3((unsigned)((count + STEP_BLOCK - 1) / STEP_BLOCK)), dim3(STEP_BLOCK), 0, nullptr, seed,
                           d_n, d_p, count, d_out);
        pr.fetch(out, d_out, (size_t)count);
    }
    return pr.status("stoch_sir_binomial_device", err, errlen);
}

}  // extern "C"
