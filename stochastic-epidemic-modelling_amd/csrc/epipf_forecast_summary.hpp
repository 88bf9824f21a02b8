// epipf_forecast_summary.hpp -- path functionals of the posterior-predictive forecast (epipf_forecast_summary; DESIGN.md
// §14.1), shared by epipf_forecast_summary.hip (SIR, SEIR, subgroups up to G = 4) and epipf_forecast_summary_wide.hip
// (G = 5..8, split off for compile time).
//
// The trajectories are forecast_kernel's (epipf_forecast.hpp), bit for bit: lane j of D R is replicate r = j % R of
// draw d = j / R with its own parameters (cp[d]) and start state (in[d]); event k draws from Philox counter
// (k, r, (step & 0xFFFFFF) | kDomainSSA, cp[d].f) under cp[d]'s key, cp[d].f = filter_index + d, on the exact f64 loop
// over [0, H].  No daily row is formed; each lane keeps five numbers of its path instead.
#pragma once
#include "epipf_kernels.hpp"

namespace epipf {

// With i(t) the infectious count after the events up to t (SIR: I; SEIR: I, not E; subgroups: the sum of I_g), per path:
//   peak            the maximum of i over the start state and every accepted event
//   peak_time       the clock value t of the first accepted event after which i == peak (strict >: the first attainment
//                   wins); 0.0 when no event exceeds the start value
//   extinction_time the clock value of the accepted event after which active() is false (SEIR: nobody exposed either);
//                   0.0 when the start state is inactive, +inf when the path is still active at the horizon
//   infections      sum of S_g at the start minus the same of the final state
//   events          accepted events
// Reductions over the n lanes, integer atomics only (exact, independent of arrival order):
//   totals[4]            sum of peak, sum of infections, extinct paths, sum of events
//   peak_hist[bins], infections_hist[bins]   count of each value (or null)
//   peak_day[H]          count of min(floor(peak_time), H - 1)
//   extinct_day[H + 1]   count of min(floor(extinction_time), H - 1) over the extinct paths; bin H: the others.
//                        cumsum(extinct_day)[k] is the number of paths whose forecast row k (epipf_forecast.hpp's row
//                        rule: the state after the last event with time < k + 1) has nobody infected -- except for an
//                        extinction event at exactly t = H, which is in no row but counts in bin H - 1 here
//   extinct_per_draw[D]  extinct paths of each draw (or null)
// The two day histograms take at most 2 H + 1 addresses from all n lanes: each block counts them in LDS and flushes once
// (a.lds_days; global atomics when they do not fit, forecast_summary_lds_days).
template <int MODEL, int G>
__global__ __launch_bounds__(256) void forecast_summary_kernel(ForecastSummaryArgs a) {
    constexpr int C = Shape<MODEL, G>::C;
    __shared__ LogTab tab[kLogTabEntries];
    extern __shared__ uint32_t bday[];                   // [H] peak day, then [H + 1] extinction day (a.lds_days)
    if (threadIdx.x < kLogTabEntries) tab[threadIdx.x] = a.logtab[threadIdx.x];
    const int ND = 2 * a.H + 1;
    if (a.lds_days)
        for (int i = threadIdx.x; i < ND; i += 256) bday[i] = 0u;
    __syncthreads();
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x;      // 64-bit: D R may be close to 2^31
    const int j = (int)lane;
    int nev = 0, peak = 0, infections = 0, gone = 0;
    if (lane < (size_t)a.n) {
        const int d = j / a.R;
        const uint32_t r = (uint32_t)(j - d * a.R);
        const ChainParam cp = a.cp[d];                   // per lane: the lanes of a wave may belong to different draws
        const uint32_t ptag = (a.step & 0xFFFFFFu) | kDomainSSA;
        const double tmax = (double)a.H;
        // susceptibles of a state: column 0 of each group's three (SIR and SEIR: G = 1, column 0)
        auto susceptible = [](const double* x) __attribute__((always_inline)) {
            double s = 0.0;
#pragma unroll
            for (int g = 0; g < G; ++g) s = s + x[3 * g];
            return s;
        };
        double x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (double)a.in[(size_t)d * C + c];
        const double s0 = susceptible(x);
        SsaState<MODEL, G> st;
        if constexpr (G > kMaxLaneG) st.bind(wide_param(a.cp, a.D, d));
        st.load(x, cp);
        double t = 0.0;
        uint32_t k = 0;
        double pk = st.infectious(), pt = 0.0;           // counts are exact integers in doubles
        bool alive = st.active();
        // every lane starts at event 0, so k is wave-uniform; event k + 1's block is drawn while event k's f64 work
        // runs (forecast_kernel's software pipelining)
        Block rn{0u, 0u, 0u, 0u};
        if (alive) rn = philox(0u, r, ptag, cp.f, cp.k0, cp.k1);
        while (alive) {
            const Block rb = rn;
            ++k;
            rn = philox(__builtin_amdgcn_readfirstlane(k), r, ptag, cp.f, cp.k0, cp.k1);
            SsaState<MODEL, G> nx = st;
            const bool ev = nx.event(rb, t, tmax, cp, tab);
            if (ev) {
                st = nx;
                ++nev;
                const double ic = st.infectious();
                const bool up = ic > pk;                 // strict: a later event that reaches the peak again does not move it
                pk = up ? ic : pk;
                pt = up ? t : pt;
            }
            alive = ev && st.active();
        }
        // t is the clock of the last accepted event (0.0 without one): the one that ended the outbreak, if it ended
        const bool extinct = !st.active();
        const double et = extinct ? t : INFINITY;
        st.save(x);
        peak = (int)pk;
        infections = (int)(s0 - susceptible(x));
        gone = extinct ? 1 : 0;
        if (a.peak) {                                    // lane j is [d][r] already: coalesced, no transpose
            a.peak[j] = peak;
            a.peak_time[j] = pt;
            a.extinction_time[j] = et;
            a.infections[j] = infections;
            a.events[j] = nev;
        }
        // every model conserves the total and bins > the largest start total (host check): the clamps never bind
        if (a.peak_hist) {
            atomicAdd(&a.peak_hist[min((uint32_t)peak, (uint32_t)a.bins - 1u)], 1u);
            atomicAdd(&a.infections_hist[min((uint32_t)infections, (uint32_t)a.bins - 1u)], 1u);
        }
        if (a.extinct_per_draw && extinct) atomicAdd(&a.extinct_per_draw[d], 1u);
        // pt and an extinct path's et lie in [0, H]: an event at exactly t = H goes to the last day
        const int pd = min((int)pt, a.H - 1);
        const int ed = extinct ? min((int)t, a.H - 1) : a.H;
        if (a.lds_days) {
            atomicAdd(&bday[pd], 1u);
            atomicAdd(&bday[a.H + ed], 1u);
        } else {
            atomicAdd(&a.peak_day[pd], 1u);
            atomicAdd(&a.extinct_day[ed], 1u);
        }
    }
    unsigned long long tot[4] = {(unsigned long long)peak, (unsigned long long)infections, (unsigned long long)gone,
                                 (unsigned long long)nev};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned long long e = tot[i];
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
        if ((threadIdx.x & 63) == 0 && e) atomicAdd(&a.totals[i], e);
    }
    if (a.lds_days) {
        __syncthreads();
        for (int i = threadIdx.x; i < ND; i += 256)
            if (bday[i]) atomicAdd(i < a.H ? &a.peak_day[i] : &a.extinct_day[i - a.H], bday[i]);
    }
}

template <int MODEL, int G>
static void forecast_summary_t(const ForecastSummaryArgs& a, hipStream_t s) {
    const size_t lds = a.lds_days ? sizeof(uint32_t) * (2 * (size_t)a.H + 1) : 0;
    hipLaunchKernelGGL((forecast_summary_kernel<MODEL, G>), dim3((unsigned)(((size_t)a.n + 255) / 256)), dim3(256), lds,
                       s, a);
}

}  // namespace epipf
