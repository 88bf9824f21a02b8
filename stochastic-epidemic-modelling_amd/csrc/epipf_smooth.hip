// epipf_smooth.hip -- the particle smoother's kernels (epipf_smooth.hpp): a backward pass of integer
// multiplicities over the resident history, and the quantiles from its value histograms.
#include "epipf_smooth.hpp"

#include "epipf_device.hpp"

namespace epipf {

namespace {
// The multiplicity rows are written and read by different threads of one workgroup between barriers.  Relaxed
// workgroup-scope atomics in both address spaces: in LDS they are plain ds operations, in global memory the loads and
// stores are kept coherent with the atomic adds (which run in L2) for the workgroup's CU.
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

// One workgroup per chain; blockDim.x is a multiple of 64.  Day p's phases, each closed by a workgroup barrier:
//   scatter  m[p][a[p+shift][j]] += m[p+1][j] for the j with m[p+1][j] > 0 (and day p + 1's sums leave LDS)
//   gather   the i with m[p][i] > 0 add m h to the workgroup's [C] sums and to the histogram; row m[p+1] is cleared and
//            becomes m[p-1]'s
// Particles with m = 0 load nothing, and a wave without a live particle skips the day.
template <bool LDS>
__global__ __launch_bounds__(kSmoothThreads) void smooth_kernel(SmoothArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_rows[];   // [2][N] when LDS
    __shared__ unsigned long long acc[2][kSmoothMaxC];   // day p's sums in slot p & 1
    __shared__ int live_n[2];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int chain = a.chain0 + (int)blockIdx.x;
    const int T = a.T, N = a.N, C = a.C;
    // degenerate or skipped in the last run: its history rows may be stale or unwritten, so it is not walked (the host
    // zeroed the outputs); uniform over the workgroup
    if (a.status && a.status[chain] != 0) return;
    const int32_t* hid = a.hidden + (size_t)chain * a.hist_stride;
    const int32_t* anc = a.ancestry + (size_t)chain * a.anc_stride;
    uint32_t* mp;                                        // m[p]
    if constexpr (LDS) mp = lds_rows;
    else mp = a.mrows + (size_t)blockIdx.x * 2 * (size_t)N;
    uint32_t* mq = mp + N;                               // m[p+1]; all zeros when the scatter of day p begins
    unsigned long long* sums = a.sums + (size_t)chain * T * C;
    int32_t* lin = a.lineages + (size_t)chain * T;
    uint32_t* hist = a.hist ? a.hist + (size_t)blockIdx.x * T * C * (size_t)a.bins : nullptr;
    const uint32_t bins = (uint32_t)a.bins;
    const bool walk = !a.predictive;

    if (walk)
        for (int i = tid; i < N; i += nt) {
            row_store(&mp[i], 1u);
            row_store(&mq[i], 0u);
        }
    for (int i = tid; i < 2 * kSmoothMaxC; i += nt) (&acc[0][0])[i] = 0ull;
    if (tid < 2) live_n[tid] = 0;
    __syncthreads();

    for (int p = T - 1; p >= 0; --p) {
        const int s = p & 1;
        if (p < T - 1) {
            // day p + 1 is complete (the barrier that closed its gather): its sums leave LDS and the slot is cleared
            // for day p - 1
            if (tid < C) {
                sums[(size_t)(p + 1) * C + tid] = acc[s ^ 1][tid];
                acc[s ^ 1][tid] = 0ull;
            }
            if (tid == 0) {
                lin[p + 1] = live_n[s ^ 1];
                live_n[s ^ 1] = 0;
            }
            if (walk) {
                uint32_t* t = mp;
                mp = mq;
                mq = t;
                const int32_t* ap = anc + (size_t)(p + a.shift) * N;
                for (int j = tid; j < N; j += nt) {
                    const uint32_t m = row_load(&mq[j]);
                    if (m) row_add(&mp[checked_index(ap[j], N)], m);
                }
            }
            __syncthreads();
        }
        // the trip count is the same for every thread, and a wave leaves an iteration as a whole: all 64 lanes are
        // active at the ballot and the shuffles, and the values they exchange were set with all 64 active
        for (int base = 0; base < N; base += nt) {
            const int i = base + tid;
            uint32_t m = 0u;
            if (i < N) {
                if (walk) {
                    m = row_load(&mp[i]);
                    row_store(&mq[i], 0u);
                } else {
                    m = 1u;
                }
            }
            const unsigned long long live = __ballot(m != 0u);
            if (live == 0ull) continue;
            const int32_t* h = hid + ((size_t)p * N + (size_t)(i < N ? i : 0)) * C;
            for (int c = 0; c < C; ++c) {
                unsigned long long v = 0ull;
                if (m) {
                    const uint32_t x = (uint32_t)h[c];
                    v = (unsigned long long)m * x;
                    // a value outside the histogram is dropped, never stored
                    if (hist && x < bins) atomicAdd(&hist[((size_t)p * C + c) * bins + x], m);
                }
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) atomicAdd(&acc[s][c], v);
            }
            if (lane == 0) atomicAdd(&live_n[s], __popcll(live));
        }
        __syncthreads();
    }
    if (tid < C) sums[tid] = acc[0][tid];
    if (tid == 0) lin[0] = live_n[0];
}

// One wave per (chain, day, compartment) cell: a chunked prefix scan over the cell's bins; rank r falls in the chunk
// whose running count passes it, at the first lane whose inclusive count reaches it.  Four cells per block.
__global__ __launch_bounds__(256) void smooth_quantile_kernel(SmoothQuantArgs a) {
    const int lane = threadIdx.x & 63;
    const size_t TC = (size_t)a.T * a.C;
    const size_t cell = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform, as every exit below
    if (cell >= (size_t)a.n * TC) return;
    const int chain = a.chain0 + (int)(cell / TC);
    if (a.status && a.status[chain] != 0) return;                      // the host zeroed its rows
    const uint32_t* h = a.hist + cell * (size_t)a.bins;
    int32_t* out = a.quant + (size_t)chain * a.n_q * TC + cell % TC;    // + q TC
    uint32_t run = 0u;                                                 // counts of the chunks before this one
    for (int base = 0; base < a.bins && run < a.max_rank; base += 64) {
        const int b = base + lane;
        uint32_t inc = b < a.bins ? h[b] : 0u;
        for (int o = 1; o < 64; o <<= 1) {                             // all 64 lanes active
            const uint32_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        const uint32_t tot = __builtin_amdgcn_readfirstlane(__shfl(inc, 63, 64));
        for (int q = 0; q < a.n_q; ++q) {
            const uint32_t r = a.ranks[q];
            if (run < r && r <= run + tot) {
                const unsigned long long hit = __ballot(run + inc >= r);
                if (lane == 0) out[(size_t)q * TC] = base + (__ffsll((long long)hit) - 1);
            }
        }
        run += tot;
    }
    // dropped values (>= bins): the counts never reach the rank
    for (int q = 0; q < a.n_q; ++q)
        if (a.ranks[q] > run && lane == 0) out[(size_t)q * TC] = a.bins;
}

int smooth_threads(int N) { return N >= kSmoothThreads ? kSmoothThreads : ((N + 63) / 64) * 64; }

hipError_t launch_smooth(const SmoothArgs& a, hipStream_t s) {
    // N <= 2^30: the strided particle indices (up to N + 1024) stay in int
    if (a.n < 1 || a.N < 1 || a.N > kSmoothMaxN || a.T < 1 || a.C < 1 || a.C > kSmoothMaxC) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n), block((unsigned)smooth_threads(a.N));
    if (a.mrows || a.predictive) {
        hipLaunchKernelGGL(smooth_kernel<false>, grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (a.N > kSmoothLdsMaxN) return hipErrorInvalidValue;
    const size_t lds = 2 * sizeof(uint32_t) * (size_t)a.N;
    if (lds > kSmoothLdsDefault) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&smooth_kernel<true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(smooth_kernel<true>, grid, block, lds, s, a);
    return hipGetLastError();
}

hipError_t launch_smooth_quantiles(const SmoothQuantArgs& a, hipStream_t s) {
    const size_t cells = (size_t)a.n * a.T * a.C;
    if (a.n < 1 || a.n_q < 1 || a.bins < 1 || (cells + 3) / 4 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(smooth_quantile_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace epipf
