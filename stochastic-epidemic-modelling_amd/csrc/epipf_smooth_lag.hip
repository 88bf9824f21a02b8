// epipf_smooth_lag.hip -- the fixed-lag particle smoother's kernel (epipf_smooth_lag.hpp): one
// backward window of integer multiplicities per (chain, day).  Its histogram goes to smooth_quantile_kernel
// (epipf_smooth.hip) unchanged.
#include "epipf_smooth_lag.hpp"

#include "epipf_device.hpp"

namespace epipf {

namespace {
// As in epipf_smooth.hip: the rows are written and read by different threads of one workgroup between barriers, through
// relaxed workgroup-scope atomics in both address spaces.
__device__ __forceinline__ uint32_t row_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void row_store(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void row_add(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
}  // namespace

// One workgroup per (chain, day p); blockDim.x is a multiple of 64.  The window's e(p) - p steps, each closed by one
// workgroup barrier:
//   scatter  w[q][a[q+shift][j]] += w[q+1][j] for the j with w[q+1][j] > 0; thread j clears w[q+1][j] on the way, so
//            the row is all zeros when it becomes w[q-1]'s
// then one gather on day p: the i with m[p][i] > 0 add m h to the workgroup's [C] sums and to the histogram.  A window of
// no steps (L = 0, or p = T-1) has m = 1 and touches no row.
template <bool LDS>
__global__ __launch_bounds__(kSmoothThreads) void smooth_lag_kernel(SmoothLagArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_rows[];   // [2][N] when LDS
    __shared__ unsigned long long acc[kSmoothMaxC];
    __shared__ int live_n;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int ci = (int)blockIdx.x / a.days;             // chain of this launch
    const int chain = a.chain0 + ci;
    const int p = a.day0 + (int)blockIdx.x % a.days;
    const int T = a.T, N = a.N, C = a.C;
    // degenerate or skipped in the last run: not walked (the host zeroed the outputs); uniform over the workgroup
    if (a.status && a.status[chain] != 0) return;
    const int32_t* hid = a.hidden + (size_t)chain * a.hist_stride;
    const int32_t* anc = a.ancestry + (size_t)chain * a.anc_stride;
    const int steps = min(a.lag, T - 1 - p);              // e(p) - p, the same for every thread
    const bool walk = steps > 0;
    uint32_t* cur;                                       // w[q+1]
    if constexpr (LDS) cur = lds_rows;
    else cur = a.mrows + (size_t)blockIdx.x * 2 * (size_t)N;
    uint32_t* oth = cur + N;                             // w[q]; all zeros when the scatter of step q begins
    uint32_t* hist = a.hist ? a.hist + ((size_t)ci * T + (size_t)p) * C * (size_t)a.bins : nullptr;
    const uint32_t bins = (uint32_t)a.bins;

    if (walk)
        for (int i = tid; i < N; i += nt) {
            row_store(&cur[i], 1u);
            row_store(&oth[i], 0u);
        }
    if (tid < kSmoothMaxC) acc[tid] = 0ull;
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
    // the trip count is the same for every thread, and a wave leaves an iteration as a whole: all 64 lanes are active
    // at the ballot and the shuffles, and the values they exchange were set with all 64 active
    for (int base = 0; base < N; base += nt) {
        const int i = base + tid;
        uint32_t m = 0u;
        if (i < N) m = walk ? row_load(&cur[i]) : 1u;
        const unsigned long long live = __ballot(m != 0u);
        if (live == 0ull) continue;
        const int32_t* h = hid + ((size_t)p * N + (size_t)(i < N ? i : 0)) * C;
        for (int c = 0; c < C; ++c) {
            unsigned long long v = 0ull;
            if (m) {
                const uint32_t x = (uint32_t)h[c];
                v = (unsigned long long)m * x;
                // a value outside the histogram is dropped, never stored
                if (hist && x < bins) atomicAdd(&hist[(size_t)c * bins + x], m);
            }
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) atomicAdd(&acc[c], v);
        }
        if (lane == 0) atomicAdd(&live_n, __popcll(live));
    }
    __syncthreads();
    if (tid < C) a.sums[((size_t)chain * T + (size_t)p) * C + tid] = acc[tid];
    if (tid == 0) a.lineages[(size_t)chain * T + p] = live_n;
}

hipError_t launch_smooth_lag(const SmoothLagArgs& a, hipStream_t s) {
    if (a.n < 1 || a.N < 1 || a.N > kSmoothMaxN || a.T < 1 || a.C < 1 || a.C > kSmoothMaxC || a.lag < 0 || a.lag > a.T - 1 ||
        a.day0 < 0 || a.days < 1 || a.day0 + a.days > a.T || (long long)a.n * a.days > kSmoothLagMaxBlocks)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.n * a.days)), block((unsigned)smooth_threads(a.N));
    if (a.mrows) {
        hipLaunchKernelGGL(smooth_lag_kernel<false>, grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (a.N > kSmoothLdsMaxN) return hipErrorInvalidValue;
    const size_t lds = 2 * sizeof(uint32_t) * (size_t)a.N;
    if (lds > kSmoothLdsDefault) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&smooth_lag_kernel<true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(smooth_lag_kernel<true>, grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace epipf
