// epipf_forecast.hpp -- the posterior-predictive forecast kernel (epipf_forecast; the reference's tests/pred_tmps.py
// traj_inf, :55-64, batched), shared by epipf_forecast.hip (SIR, SEIR, subgroups up to G = 4) and
// epipf_forecast_wide.hip (G = 5..8, split off for compile time).
//
// One lane per trajectory: lane j of D R is replicate r = j % R of posterior draw d = j / R, which has its own
// parameters (cp[d]) and its own start state (in[d]).  The lane runs the exact event loop over [0, H] -- the
// reference's continuous path with its clock bit for bit, as simulate_path_kernel -- and bins it into one row per
// day while it runs, so no event ever leaves the device.
#pragma once
#include "epipf_kernels.hpp"

namespace epipf {

// Stream: draw d, replicate r, event k -> Philox counter (k, r, (step & 0xFFFFFF) | kDomainSSA, cp[d].f) under
// cp[d]'s key; the host sets cp[d].f = filter_index + d.  A draw's forecast is therefore simulate_path of R copies of
// its state at filter index filter_index + d, whatever else is in the batch.
//
// Row rule: row `day` (0..H-1) is the state after the last event with time < day + 1; a day without an event repeats
// the previous row.  This is traj_inf's "last index with floor(time) == day, else the previous row" (pred_tmps.py:58-63).
template <int MODEL, int G>
__global__ __launch_bounds__(256) void forecast_kernel(ForecastArgs a) {
    constexpr int C = Shape<MODEL, G>::C;
    __shared__ LogTab tab[kLogTabEntries];
    extern __shared__ unsigned long long bsum[];         // [H][C] block sums (a.lds_sums), flushed once per block
    if (threadIdx.x < kLogTabEntries) tab[threadIdx.x] = a.logtab[threadIdx.x];
    const int HC = a.H * C;
    if (a.lds_sums)
        for (int i = threadIdx.x; i < HC; i += 256) bsum[i] = 0ull;
    __syncthreads();
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x;      // 64-bit: D R may be close to 2^31
    const int j = (int)lane;
    int nev = 0;
    if (lane < (size_t)a.n) {
        const int d = j / a.R;
        const uint32_t r = (uint32_t)(j - d * a.R);
        const ChainParam cp = a.cp[d];                   // per lane: the lanes of a wave may belong to different draws
        const uint32_t ptag = (a.step & 0xFFFFFFu) | kDomainSSA;
        const double tmax = (double)a.H;
        // one daily row: the lane-minor store, the exact integer sums and the value histogram
        auto emit = [&](int day, const int32_t* xs) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const size_t cell = (size_t)day * C + c;
                if (a.rows) a.rows[cell * a.n + j] = xs[c];
                if (a.lds_sums) atomicAdd(&bsum[cell], (unsigned long long)xs[c]);
                else atomicAdd(&a.sums[cell], (unsigned long long)xs[c]);
                // every model conserves the total and bins > the largest start total (host check): the clamp never binds
                if (a.hist) atomicAdd(&a.hist[cell * a.bins + min((uint32_t)xs[c], (uint32_t)a.bins - 1u)], 1u);
            }
        };
        double x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (double)a.in[(size_t)d * C + c];
        SsaState<MODEL, G> st;
        if constexpr (G > kMaxLaneG) st.bind(wide_param(a.cp, a.D, d));
        st.load(x, cp);
        double t = 0.0;
        uint32_t k = 0;
        int day = 0;
        bool alive = st.active();
        // every lane starts at event 0, so k is wave-uniform; event k + 1's block is drawn while event k's f64 work
        // runs (exact_propagate's software pipelining)
        Block rn{0u, 0u, 0u, 0u};
        if (alive) rn = philox(0u, r, ptag, cp.f, cp.k0, cp.k1);
        while (alive) {
            const Block rb = rn;
            ++k;
            rn = philox(__builtin_amdgcn_readfirstlane(k), r, ptag, cp.f, cp.k0, cp.k1);
            SsaState<MODEL, G> nx = st;
            const bool ev = nx.event(rb, t, tmax, cp, tab);
            if (ev) {
                if (day < a.H && (double)(day + 1) <= t) {     // the days that ended before this event: the state before it
                    double xd[C];
                    int32_t xs[C];
                    st.save(xd);
#pragma unroll
                    for (int c = 0; c < C; ++c) xs[c] = (int32_t)xd[c];
                    do {
                        emit(day, xs);
                        ++day;
                    } while (day < a.H && (double)(day + 1) <= t);
                }
                st = nx;
                ++nev;
            }
            alive = ev && st.active();
        }
        // extinction or overshoot: the remaining days hold the final state
        int32_t xs[C];
        st.save(x);
#pragma unroll
        for (int c = 0; c < C; ++c) xs[c] = (int32_t)x[c];
        for (; day < a.H; ++day) emit(day, xs);
    }
    unsigned long long e = (unsigned long long)nev;
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    if ((threadIdx.x & 63) == 0 && e) atomicAdd(a.events, e);
    if (a.lds_sums) {
        __syncthreads();
        for (int i = threadIdx.x; i < HC; i += 256)
            if (bsum[i]) atomicAdd(&a.sums[i], bsum[i]);
    }
}

template <int MODEL, int G>
static void forecast_t(const ForecastArgs& a, hipStream_t s) {
    const size_t lds = a.lds_sums ? sizeof(unsigned long long) * (size_t)a.H * Shape<MODEL, G>::C : 0;
    hipLaunchKernelGGL((forecast_kernel<MODEL, G>), dim3((unsigned)(((size_t)a.n + 255) / 256)), dim3(256), lds, s, a);
}

}  // namespace epipf
