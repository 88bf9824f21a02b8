// epipf_kernels.hip -- the particle-filter kernels for MI355X (gfx950) and their launchers.
//
// One filter step (pmcmc.py:177-231) is ONE kernel launch, batched over independent chains: a 1-D grid of
// (chain, particle block of WG lanes) pairs, one particle per lane, placed so that each chain's blocks share one
// XCD's L2 (step_block, epipf_step.hpp; EPIPF_XCD_MAP=0: the 2-D grid y = chain, x = block):
//
//   step p:  [scan of the previous step's block sums in LDS -> total, log-likelihood]
//            [multinomial draw U_j -> certified two-level CDF search -> ancestor a_j]   (pmcmc.py:183-193)
//            [gather parent state hidden[p-1][a_j] -> Gillespie SSA over [0,1]]          (pmcmc.py:195-220)
//            [store hidden[p][j]; weight against Y[p]; in-block scan; block sum]         (pmcmc.py:178-181, next step)
//
// so the weights, the in-block CDF and the block sums of step p are produced by the same lanes that
// produced the states, and the next launch only reads them.  The init kernel draws the Poisson initial
// states (pmcmc.py:156-175) and the first weights.
#include "epipf_kernels.hpp"

namespace epipf {

// particle_path_sampler, pmcmc.py:236-248 (one lane per chain; T dependent loads)
__global__ void path_sample_kernel(PathArgs a) {
    const int chain = blockIdx.x * blockDim.x + threadIdx.x;
    if (chain >= a.n_chains) return;
    int32_t* out = a.traj + (size_t)chain * a.T * a.C;
    if (a.status[chain] != 0) {                      // degenerate or skipped in the last run: its history rows may be
        for (int i = 0; i < a.T * a.C; ++i) out[i] = 0;   // stale or unwritten, so it is not walked (zeros returned)
        return;
    }
    const int pick = a.chosen ? a.chosen[chain] : a.cp[chain].chosen;   // epipf_path_sample / epipf_run_sampled
    if (pick < 0) {                                  // no path asked of this chain
        for (int i = 0; i < a.T * a.C; ++i) out[i] = 0;
        return;
    }
    int chosen = checked_index(pick, a.N);
    const int32_t* hid = a.hidden + (size_t)chain * a.hist_stride;
    const int32_t* anc = a.ancestry + (size_t)chain * a.anc_stride;
    for (int c = 0; c < a.C; ++c) out[(size_t)(a.T - 1) * a.C + c] = hid[((size_t)(a.T - 1) * a.N + chosen) * a.C + c];
    for (int p = a.T - 2; p >= 0; --p) {
        chosen = checked_index(anc[(size_t)p * a.N + chosen], a.N);       // ancestry[p], as the reference
        for (int c = 0; c < a.C; ++c) out[(size_t)p * a.C + c] = hid[((size_t)p * a.N + chosen) * a.C + c];
    }
}

// Standalone resampler over caller-supplied weights and uniforms (same scan + search code as the filter).
template <int WG>
__global__ __launch_bounds__(WG) void resample_scan_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int j = blockIdx.x * WG + threadIdx.x;
    const double w = (j < a.N) ? a.w[j] : 0.0;
    const double loc = block_inclusive_scan<WG>(w, smem);
    a.wraw[j] = w;
    a.wloc[j] = loc;
    if (threadIdx.x == WG - 1) a.bsum[blockIdx.x] = loc;
}

template <int WG>
__global__ __launch_bounds__(WG) void resample_search_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* red = smem + 2 * kLogTabEntries;
    double* bsum = red + 16;
    double* bpex = bsum + a.B;
    const int j = blockIdx.x * WG + threadIdx.x;
    const double total = scan_block_sums<WG>(a.bsum, a.B, bpex, bsum, red);
    if (!(total > 0.0)) {
        if (j == 0) *a.status = 1;
        return;
    }
    const double U = (j < a.N) ? a.u[j] : 0.0;
    bool certified = true, ambiguous = false;      // standalone resampler: no reference weights, ref_k = 0
    int anc = 0;
    if (j < a.N) anc = resample_search<WG>(U, bpex, bsum, a.B, total, a.wloc, a.N, a.cert_k, certified, 0.0, ambiguous);
    if (__any(!certified)) {
        const int e = resample_exact_wave(!certified, U, a.wraw, a.N);
        if (!certified) {
            anc = e;
            atomicAdd(a.fallbacks, 1ull);
        }
    }
    if (j < a.N) a.out[j] = checked_index(anc, a.N);
}

// ------------------------------------------------------------------------------- launchers
// blocks per prefix segment: the smallest power of two with at most kMaxSegments segments
int prefix_segment(int B) {
    int S = 1;
    while ((B + S - 1) / S > kMaxSegments) S <<= 1;
    return S;
}

size_t step_lds_bytes(int B, int wg) { return step_lds_bytes_seg(B, prefix_segment(B), wg); }

size_t step_lds_bytes_seg(int B, int S, int wg) {
    if (S == 1) return sizeof(LogTab) * kLogTabEntries + sizeof(double) * (size_t)(16 + B + B + wg);
    return sizeof(LogTab) * kLogTabEntries + sizeof(double) * (size_t)(16 + 2 * ((B + S - 1) / S));
}

static size_t resample_lds_bytes(int B, int wg) {
    return sizeof(LogTab) * kLogTabEntries + sizeof(double) * (size_t)(16 + B + B + wg);
}

template <int WG>
static hipError_t launch_model(const StepArgs& a, int model, int G, int obs, int n_chains, const FilterStreams& fs) {
    // G = 5..8: the instances of epipf_kernels_wide.hip, one lane per particle only
    if (model >= kSubgroups && G > kMaxLaneG) return a.lanes > 1 ? hipErrorInvalidValue : launch_filter_wide(a, model, G, obs, n_chains, fs);
    switch (model) {
        case kSIR: return launch_obs<kSIR, 1, WG>(a, obs, n_chains, fs);
        case kSEIR: return launch_obs<kSEIR, 1, WG>(a, obs, n_chains, fs);
        case kSubgroups:
            switch (G) {
                case 1: return launch_obs<kSubgroups, 1, WG>(a, obs, n_chains, fs);
                case 2: return launch_obs<kSubgroups, 2, WG>(a, obs, n_chains, fs);
                case 3: return launch_obs<kSubgroups, 3, WG>(a, obs, n_chains, fs);
                case 4: return launch_obs<kSubgroups, 4, WG>(a, obs, n_chains, fs);
            }
            break;
        case kSubgroups2:
            switch (G) {
                case 1: return launch_obs<kSubgroups2, 1, WG>(a, obs, n_chains, fs);
                case 2: return launch_obs<kSubgroups2, 2, WG>(a, obs, n_chains, fs);
                case 3: return launch_obs<kSubgroups2, 3, WG>(a, obs, n_chains, fs);
                case 4: return launch_obs<kSubgroups2, 4, WG>(a, obs, n_chains, fs);
            }
            break;
    }
    return hipErrorInvalidValue;
}

// 64-thread init and step blocks; a.wg particles per block: 64, or kGroupBlock for lane-group runs of W >= 8
hipError_t launch_filter(const StepArgs& a, int model, int G, int obs, int n_chains, const FilterStreams& fs) {
    if (!(a.wg == 64 || (a.wg == kGroupBlock && a.lanes >= 8))) return hipErrorInvalidValue;
    return launch_model<64>(a, model, G, obs, n_chains, fs);
}

hipError_t launch_path_sample(const PathArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(path_sample_kernel, dim3((a.n_chains + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_simulate(const SimArgs& a, int model, int G, hipStream_t s) {
    switch (model) {
        case kSIR: sim_t<kSIR, 1>(a, s); break;
        case kSEIR: sim_t<kSEIR, 1>(a, s); break;
        default:
            switch (G) {
                case 1: sim_t<kSubgroups, 1>(a, s); break;
                case 2: sim_t<kSubgroups, 2>(a, s); break;
                case 3: sim_t<kSubgroups, 3>(a, s); break;
                case 4: sim_t<kSubgroups, 4>(a, s); break;
                default: return launch_simulate_wide(a, G, s);
            }
    }
    return hipGetLastError();
}

hipError_t launch_simulate_path(const SimPathArgs& a, int model, int G, hipStream_t s) {
    switch (model) {
        case kSIR: sim_path_t<kSIR, 1>(a, s); break;
        case kSEIR: sim_path_t<kSEIR, 1>(a, s); break;
        default:
            switch (G) {
                case 1: sim_path_t<kSubgroups, 1>(a, s); break;
                case 2: sim_path_t<kSubgroups, 2>(a, s); break;
                case 3: sim_path_t<kSubgroups, 3>(a, s); break;
                case 4: sim_path_t<kSubgroups, 4>(a, s); break;
                default: return launch_simulate_path_wide(a, G, s);
            }
    }
    return hipGetLastError();
}

hipError_t launch_resample(const ResampleArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(resample_scan_kernel<256>, dim3(a.B), dim3(256), sizeof(double) * 16, s, a);
    hipLaunchKernelGGL(resample_search_kernel<256>, dim3(a.B), dim3(256), resample_lds_bytes(a.B, 256), s, a);
    return hipGetLastError();
}

}  // namespace epipf
