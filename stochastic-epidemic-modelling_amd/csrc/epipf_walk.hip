// epipf_walk.hip -- time-varying rates on MI355X (gfx950), DESIGN.md §18: the random-walk filter and the smoother of
// its parameter history (epipf_walk.hpp).
//
// walk_init_kernel / walk_step_kernel filter with theta per particle, one pass: one lane per particle, one wave per
// block, on the shared phases of epipf_step.hpp (step_total, step_degenerate, step_log_zeta, step_ancestor, step_count,
// step_store_weights, init_state, init_weights), with the per-lane SSA of IF2 (the certified f32 loop, then the exact
// loop for the lanes it hands back).  Their own:
//   - every chain starts (status OK); there is one pass, so no iteration offset on the filter index;
//   - the half-widths read per chain from a device array (a chain of the batch may walk with its own step width);
//   - the swarm addressed in theta_hist: step p gathers the ancestor's theta from row p - 1 and stores the jittered
//     theta in row p, so the whole history of the parameters stays on the device;
//   - no finish kernel: there is no next iteration to start and no swarm mean to reduce.
// walk_smooth_kernel is smooth_lag_kernel's backward window (epipf_smooth_lag.hip) followed, per quantity, by a
// fixed-order mean and a most-significant-digit radix select of the weighted quantiles.
#include "epipf_walk.hpp"

#include <algorithm>

#include "epipf_if2_perturb.hpp"
#include "epipf_step.hpp"

namespace epipf {

template <int MODEL, int OBS>
__global__ __launch_bounds__(64) void walk_init_kernel(WalkArgs a) {
    constexpr int C = Shape<MODEL, 1>::C;
    constexpr int D = (MODEL == kSIR) ? 2 : 3;
    constexpr int WG = 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const BlockPos bp = step_block(s);
    const int chain = bp.chain;
    const int j = bp.b * WG + (int)threadIdx.x;
    const ChainParam cp = s.cp[chain];
    if (bp.b == 0 && threadIdx.x == 0) s.status[chain] = kStatusOk;
    double x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    if (j < s.N) {
        init_particle<MODEL, 1>(s, cp, j, x);
        init_state<C>(s, chain, j, x);
        double th[D], hw[D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            th[c] = a.start[((size_t)chain * D + c) * s.N + j];
            hw[c] = a.hw[(size_t)chain * D + c];
        }
        if2_perturb_hw<D>(th, hw, (uint32_t)j, kDomainIf2, cp);          // step 0
        double* row = a.hist + (size_t)chain * a.chain_stride;           // day 0
#pragma unroll
        for (int c = 0; c < D; ++c) row[(size_t)c * s.N + j] = th[c];
    }
    init_weights<WG>(s, smem, bp, j, j < s.N, true, WG - 1, [&] {
        return particle_weight<MODEL, 1, OBS>(x, s.Y, cp, s.cp + chain, s.lf, s.lf_max,
                                              s.hidden + (size_t)chain * s.hist_stride + (size_t)j * C);
    });
}

template <int MODEL, int OBS>
__global__ __launch_bounds__(64) void walk_step_kernel(WalkArgs a, int p) {
    constexpr int C = Shape<MODEL, 1>::C;
    constexpr int K = Shape<MODEL, 1>::K;
    constexpr int D = (MODEL == kSIR) ? 2 : 3;
    constexpr int WG = 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    LogTab* tab = step_logtab(smem);
    const BlockPos bp = step_block(s);
    const int chain = bp.chain;
    const int tid = threadIdx.x;
    const int j = bp.b * WG + tid;
    if (s.status[chain] != 0) return;
    const ChainParam cp = s.cp[chain];
    const size_t wprev = step_half(s, chain, p - 1, s.wstride), wcur = step_half(s, chain, p, s.wstride);
    const size_t bprev = step_half(s, chain, p - 1, s.bstride), bcur = step_half(s, chain, p, s.bstride);
    const double total = step_total(s, smem, bprev);
    if (!(total > 0.0)) {
        step_degenerate(s, bp, p);
        return;
    }
    step_log_zeta(s, bp, p, total);
    int anc = step_ancestor<false>(s, smem, cp, p, j, total, wprev, bprev);
    // the ancestor's theta of day p - 1, jittered and kept as day p's: this particle's rates
    double x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    const uint32_t ptag = ((uint32_t)p & 0xFFFFFFu) | kDomainSSA;
    ChainParam lcp = cp;
    bool fast_ok = true, eligible = false;
    int nev = 0, iters = 0;
    if (j < s.N) {
        anc = checked_index(anc, s.N);
        s.ancestry[(size_t)chain * s.anc_stride + (size_t)p * s.N + j] = anc;
        const double* from = a.hist + (size_t)chain * a.chain_stride + (size_t)(p - 1) * D * s.N;
        double* to = a.hist + (size_t)chain * a.chain_stride + (size_t)p * D * s.N;
        double th[D], hw[D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            th[c] = from[(size_t)c * s.N + anc];
            hw[c] = a.hw[(size_t)chain * D + c];
        }
        if2_perturb_hw<D>(th, hw, (uint32_t)j, ((uint32_t)p & 0xFFFFFFu) | kDomainIf2, cp);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            to[(size_t)c * s.N + j] = th[c];
            lcp.theta[c] = th[c];
            lcp.thetaf[c] = (float)th[c];
        }
        const int32_t* hp = s.hidden + (size_t)chain * s.hist_stride + ((size_t)(p - 1) * s.N + anc) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (double)hp[c];
        fast_ok = fast_propagate<MODEL, 1>(x, lcp, (uint32_t)j, ptag, 1.0, nev, iters, eligible);
    }
    // lanes the f32 loop could not run or could not certify: the exact loop from the untouched parent state, per lane
    // (one wave per block, so the test is block-uniform and the barrier legal)
    if (__any(!fast_ok)) {
        for (int i = tid; i < kLogTabEntries; i += WG) tab[i] = s.logtab[i];
        __syncthreads();
        if (!fast_ok) nev = exact_propagate<MODEL, 1>(x, lcp, (uint32_t)j, ptag, 1.0, tab, iters);
    }
    step_count(s, nev, iters, !fast_ok);                 // lanes past N hold fast_ok = true
    double w = 0.0;
    if (j < s.N) {
        int32_t* hc = s.hidden + (size_t)chain * s.hist_stride + ((size_t)p * s.N + j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) hc[c] = (int32_t)x[c];
        if (p + 1 < s.T) w = particle_weight<MODEL, 1, OBS>(x, s.Y + (size_t)p * K, cp, s.cp + chain, s.lf, s.lf_max, hc);
    }
    step_store_weights(s, smem, bp.b, j, p, w, wcur, bcur);
}

template <int MODEL, int OBS>
static hipError_t launch_walk_t(const WalkArgs& a, int n_chains, const FilterStreams& fs) {
    const StepArgs& s0 = a.s;
    const size_t lds = step_lds_bytes(s0.B, 64);
    launch_chain_groups(s0, n_chains, fs, 64, [&](int, const StepArgs& sg, int, dim3 grid, hipStream_t st) {
        WalkArgs ag = a;
        ag.s = sg;
        hipLaunchKernelGGL((walk_init_kernel<MODEL, OBS>), grid, dim3(64), lds, st, ag);
        for (int p = 1; p < s0.T; ++p) hipLaunchKernelGGL((walk_step_kernel<MODEL, OBS>), grid, dim3(64), lds, st, ag, p);
    });
    return hipGetLastError();
}

hipError_t launch_walk(const WalkArgs& a, int model, int obs, int n_chains, const FilterStreams& fs) {
    if (a.s.wg != 64 || a.s.lanes != 1 || !a.hw || !a.start || !a.hist) return hipErrorInvalidValue;
    if (model == kSIR && a.d == 2)
        return obs == kBinomial ? launch_walk_t<kSIR, kBinomial>(a, n_chains, fs) : launch_walk_t<kSIR, kNormal>(a, n_chains, fs);
    if (model == kSEIR && a.d == 3)
        return obs == kBinomial ? launch_walk_t<kSEIR, kBinomial>(a, n_chains, fs) : launch_walk_t<kSEIR, kNormal>(a, n_chains, fs);
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------------ the reduction
namespace {
// As in epipf_smooth_lag.hip: the rows are written and read by different threads of one workgroup between barriers,
// through relaxed workgroup-scope atomics in both address spaces.
__device__ __forceinline__ uint32_t row_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void row_store(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void row_add(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Quantity k of particle i on one day: th [d][N] and hid [N][C] are the day's rows.  `+ 0.0` turns -0.0 into +0.0, so
// every value is >= +0.0 or +inf and its bit pattern orders as the number does.  No contraction (-ffp-contract=off).
__device__ __forceinline__ double walk_value(const double* th, const int32_t* hid, int k, int i, int N, int C, int d,
                                             double pop) {
    if (k < d) return th[(size_t)k * N + i] + 0.0;
    const double den = th[(size_t)(d - 1) * N + i] * pop;
    if (den == 0.0) return __builtin_inf();
    const double num = th[i] * (double)hid[(size_t)i * C];
    return num / den + 0.0;
}
}  // namespace

// One workgroup per (chain, day p); blockDim.x is a multiple of 64.  First smooth_lag_kernel's window: e(p) - p scatter
// steps, each closed by one workgroup barrier, leave m[p] in `cur` (no step: m = 1, no row touched).  Then per
// quantity k:
//   mean      thread t adds m v over i = t, t + blockDim, ... in ascending i; the 64 lanes of a wave combine by the xor
//             butterfly at offsets 32, 16, 8, 4, 2, 1 (a + b is commutative, so every lane holds the same bits); thread 0
//             adds the waves' sums in wave order and divides by N.  No floating-point atomic: the same bits on every run.
//   quantiles the values' uint64 patterns order as the values, so the rank's holder is found digit by digit from the top:
//             eight passes of a 256-bin weight histogram (integer LDS atomics) over the particles that match the prefix
//             found so far, wave 0 scanning the bins to the one that holds the rank.  Up to kWalkQGroup quantiles share a
//             pass.  Integers only, hence exact and independent of the order of arrival.
// Every loop bound that encloses a barrier is the same for all threads of the workgroup.
template <bool LDS>
__global__ __launch_bounds__(kSmoothThreads) void walk_smooth_kernel(WalkSmoothArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_rows[];   // [2][N] when LDS
    __shared__ uint32_t rhist[kWalkQGroup][256];
    __shared__ double wsum[kSmoothThreads / 64];
    __shared__ unsigned long long sel_prefix[kWalkQGroup];
    __shared__ uint32_t sel_rank[kWalkQGroup];
    __shared__ int live_n;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int ci = (int)blockIdx.x / a.days;
    const int chain = a.chain0 + ci;
    const int p = a.day0 + (int)blockIdx.x % a.days;
    const int T = a.T, N = a.N, C = a.C, d = a.d, V = a.d + 1;
    if (a.status && a.status[chain] != 0) return;        // uniform over the workgroup; the host zeroed the outputs
    const int32_t* hid = a.hidden + (size_t)chain * a.hist_stride + (size_t)p * N * C;
    const int32_t* anc = a.ancestry + (size_t)chain * a.anc_stride;
    const double* th = a.theta + (size_t)chain * a.theta_stride + (size_t)p * d * N;
    const int steps = min(a.lag, T - 1 - p);
    const bool walk = steps > 0;
    uint32_t* cur;
    if constexpr (LDS) cur = lds_rows;
    else cur = a.mrows + (size_t)blockIdx.x * 2 * (size_t)N;
    uint32_t* oth = cur + N;

    if (walk)
        for (int i = tid; i < N; i += nt) {
            row_store(&cur[i], 1u);
            row_store(&oth[i], 0u);
        }
    if (tid == 0) live_n = 0;
    __syncthreads();
    for (int q = p + steps - 1; q >= p; --q) {
        const int32_t* aq = anc + (size_t)(q + a.shift) * N;   // q + shift <= e(p) <= T-1
        for (int j = tid; j < N; j += nt) {
            const uint32_t m = row_load(&cur[j]);
            if (m) {
                row_store(&cur[j], 0u);
                row_add(&oth[checked_index(aq[j], N)], m);
            }
        }
        __syncthreads();
        uint32_t* t = cur;
        cur = oth;
        oth = t;
    }
    // surviving lineages: the trip count is the same for every thread, so all 64 lanes are active at the ballot
    for (int base = 0; base < N; base += nt) {
        const int i = base + tid;
        uint32_t m = 0u;
        if (i < N) m = walk ? row_load(&cur[i]) : 1u;
        const unsigned long long live = __ballot(m != 0u);
        if (lane == 0 && live) atomicAdd(&live_n, __popcll(live));
    }
    __syncthreads();
    if (tid == 0) a.lineages[(size_t)chain * T + p] = live_n;

    for (int k = 0; k < V; ++k) {
        double acc = 0.0;
        for (int i = tid; i < N; i += nt) {
            const uint32_t m = walk ? row_load(&cur[i]) : 1u;
            if (m) acc = acc + (double)m * walk_value(th, hid, k, i, N, C, d, a.pop);
        }
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);   // all lanes active, acc set in all
        if (lane == 0) wsum[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int w = 0; w < nt / 64; ++w) tot = tot + wsum[w];
            a.mean[((size_t)chain * T + p) * V + k] = tot / (double)N;
        }
        for (int g0 = 0; g0 < a.n_q; g0 += kWalkQGroup) {
            const int ng = min(kWalkQGroup, a.n_q - g0);
            if (tid < ng) {
                sel_prefix[tid] = 0ull;
                sel_rank[tid] = a.ranks[g0 + tid];
            }
            for (int sh = 56; sh >= 0; sh -= 8) {
                for (int i = tid; i < ng * 256; i += nt) (&rhist[0][0])[i] = 0u;
                __syncthreads();                          // the bins are clear, the prefixes of the last pass visible
                unsigned long long pre[kWalkQGroup];
#pragma unroll
                for (int g = 0; g < kWalkQGroup; ++g) pre[g] = g < ng ? sel_prefix[g] : 0ull;
                for (int i = tid; i < N; i += nt) {
                    const uint32_t m = walk ? row_load(&cur[i]) : 1u;
                    if (!m) continue;
                    const unsigned long long bits =
                        (unsigned long long)__double_as_longlong(walk_value(th, hid, k, i, N, C, d, a.pop));
                    const unsigned long long top = sh == 56 ? 0ull : bits >> (sh + 8);
                    const uint32_t digit = (uint32_t)(bits >> sh) & 255u;
#pragma unroll
                    for (int g = 0; g < kWalkQGroup; ++g)
                        if (g < ng && top == pre[g]) atomicAdd(&rhist[g][digit], m);
                }
                __syncthreads();
                if (tid < 64) {                           // wave 0, all 64 lanes: lane l owns bins 4l .. 4l + 3
                    for (int g = 0; g < ng; ++g) {
                        const uint32_t rank = sel_rank[g];
                        uint32_t h[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) h[t] = rhist[g][4 * lane + t];
                        const uint32_t own = h[0] + h[1] + h[2] + h[3];
                        uint32_t incl = own;
                        for (int o = 1; o < 64; o <<= 1) {
                            const uint32_t up = __shfl_up(incl, o, 64);
                            if (lane >= o) incl += up;
                        }
                        uint32_t below = incl - own;      // weight in the bins before this lane's
                        if (below < rank && rank <= incl) {   // one lane: the prefix's weight is at least the rank
                            int t = 0;
                            while (t < 3 && below + h[t] < rank) below += h[t++];
                            sel_prefix[g] = (pre[g] << 8) | (unsigned long long)(4 * lane + t);
                            sel_rank[g] = rank - below;
                        }
                    }
                }
                __syncthreads();                          // wave 0 has read the bins before they are cleared
            }
            if (tid < ng)
                a.quant[(((size_t)chain * a.n_q + g0 + tid) * T + p) * V + k] =
                    __longlong_as_double((long long)sel_prefix[tid]);
        }
        __syncthreads();                                  // wsum, sel_prefix and sel_rank are free for the next quantity
    }
}

hipError_t launch_walk_smooth(const WalkSmoothArgs& a, hipStream_t s) {
    if (a.n < 1 || a.N < 1 || a.N > kSmoothMaxN || a.T < 1 || a.C < 1 || a.d < 1 || a.d > kIf2MaxD || a.lag < 0 ||
        a.lag > a.T - 1 || a.day0 < 0 || a.days < 1 || a.day0 + a.days > a.T || a.n_q < 0 || (a.n_q > 0 && !a.ranks) ||
        (long long)a.n * a.days > (1 << 24))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.n * a.days)), block((unsigned)smooth_threads(a.N));
    if (a.mrows) {
        hipLaunchKernelGGL(walk_smooth_kernel<false>, grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (a.N > kSmoothLdsMaxN) return hipErrorInvalidValue;
    const size_t lds = 2 * sizeof(uint32_t) * (size_t)a.N;
    if (lds > kSmoothLdsDefault / 2) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&walk_smooth_kernel<true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(walk_smooth_kernel<true>, grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace epipf
