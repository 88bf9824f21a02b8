// abc_smc_kernels.hip -- ABC-SMC (population Monte Carlo ABC; Toni et al. 2009, Beaumont et al. 2009) for the SIR
// model on MI355X: the sequential layer over abc_kernels.hip.
//
// abc_smc_propose_kernel  one lane per trial t of a batch: the ancestor j from the previous weighted population
//                         (numpy legacy choice's searchsorted(cdf, u, 'right')), theta* = theta_prev[j] + s (2u - 1)
//                         per component, the prior-box test, and the trial's predicted length for the sort.
// abc_smc_trials_kernel   abc_trial.hpp's one-lane trial with theta read from the proposal (abc_trial_lane<true>);
//                         proposals outside the box are skipped and come out of abc_distance_kernel as +inf.
// abc_smc_weights_kernel  den_i = sum_j [|theta_i - theta_prev_j| <= s, both components] w_prev_j, summed in j order
//                         (bit-equal to np.cumsum(np.where(mask, w_prev, 0.0))[-1]); one lane per new sample.
//
// Trial t's initial counts and SSA events come from the rejection sampler's counters (c, t, 4<<24, f) and
// (k, t, 5<<24, f); the proposal draws from the new domain 6<<24: block (0, t, 6<<24, f) -> u_sel = U(w0, w1), block
// (1, t, 6<<24, f) -> u_beta = U(w0, w1), u_gamma = U(w2, w3).
#include "abc_trial.hpp"

namespace epipf {

constexpr uint32_t kDomainAbcSmc = 6u << 24;

__global__ __launch_bounds__(256) void abc_smc_propose_kernel(AbcArgs a, AbcSmcArgs m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const size_t n = (size_t)a.n;
    const uint32_t t = a.t0 + (uint32_t)i;
    const Block rs = philox(0u, t, kDomainAbcSmc, a.f, a.k0, a.k1);
    const Block rp = philox(1u, t, kDomainAbcSmc, a.f, a.k0, a.k1);
    const double us = u01(rs.x, rs.y);
    int lo = 0, hi = m.n_prev;                  // searchsorted(cdf, us, side='right'): entries <= us
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m.cdf[mid] <= us) lo = mid + 1;
        else hi = mid;
    }
    const int j = min(lo, m.n_prev - 1);
    const double u[2] = {u01(rp.x, rp.y), u01(rp.z, rp.w)};
    double th[2];
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        th[c] = m.prev_theta[2 * (size_t)j + c] + m.half[c] * (2.0 * u[c] - 1.0);
        inside = inside && th[c] >= a.prior_lo[c] && th[c] <= m.hi[c];
    }
    a.theta[i] = th[0];
    a.theta[n + i] = th[1];
    m.anc[i] = j;
    a.days[i] = inside ? 0 : -1;                // row 0's S: the marker abc_trial_lane<true> and the distance read
    if (a.perm) {                               // outside the box: no events, sorted last
        a.sort_keys[0][i] = inside ? abc_predicted_length(a, (float)th[0], (float)th[1]) : 0u;
        a.sort_vals[0][i] = i;
    }
}

// As abc_trials_kernel: no minimum-waves bound, so the event loop keeps its registers
__global__ __launch_bounds__(256) void abc_smc_trials_kernel(AbcArgs a) {
    __shared__ LogTab tab[kLogTabEntries];
    if (threadIdx.x < kLogTabEntries) tab[threadIdx.x] = a.logtab[threadIdx.x];
    __syncthreads();
    abc_trial_lane<true>(a, tab);
}

// The previous population goes through LDS in tiles of kSmcTile points (beta, gamma, w: 24 B each, 6 KiB a tile, one
// point per thread to stage; LDS never limits the waves per SIMD, and the kernel needs few registers, so no
// minimum-waves bound).  In the inner loop every lane of a wave reads
// the same j: one LDS address per read, a broadcast without bank conflicts.  A lane's sum runs over j = 0 .. n_prev-1
// in order, tile after tile, so its rounding is the sequential sum's; adding +0.0 for a point outside the kernel
// leaves the sum as it is, which is what np.where(mask, w, 0.0) adds.
constexpr int kSmcTile = 256;

__global__ __launch_bounds__(256) void abc_smc_weights_kernel(AbcSmcWeightArgs a) {
    __shared__ double pb[kSmcTile], pg[kSmcTile], pw[kSmcTile];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < a.n;
    const double tb = live ? a.theta[2 * (size_t)i] : 0.0, tg = live ? a.theta[2 * (size_t)i + 1] : 0.0;
    const double sb = a.half[0], sg = a.half[1];
    double den = 0.0;
    for (int j0 = 0; j0 < a.n_prev; j0 += kSmcTile) {
        const int mcount = min(kSmcTile, a.n_prev - j0);
        for (int q = threadIdx.x; q < mcount; q += 256) {
            pb[q] = a.prev_theta[2 * (size_t)(j0 + q)];
            pg[q] = a.prev_theta[2 * (size_t)(j0 + q) + 1];
            pw[q] = a.prev_w[j0 + q];
        }
        __syncthreads();
        for (int q = 0; q < mcount; ++q) {
            const bool in = fabs(tb - pb[q]) <= sb && fabs(tg - pg[q]) <= sg;
            den += in ? pw[q] : 0.0;
        }
        __syncthreads();
    }
    if (live) a.den[i] = den;
}

hipError_t launch_abc_smc_trials(const AbcArgs& a0, const AbcSmcArgs& m, hipStream_t s) {
    if (a0.n <= 0) return hipSuccess;
    AbcArgs a = a0;
    a.g0 = 0;                                   // every trial on one lane (lane groups for SMC trials: DESIGN §15)
    a.group_end = 0;
    if (a.n <= 64) a.perm = nullptr;            // one wave: nothing to order, and the sort's launches would dominate
    const dim3 grid((a.n + 255) / 256);
    hipLaunchKernelGGL(abc_smc_propose_kernel, grid, dim3(256), 0, s, a, m);
    if (a.perm) {
        hipError_t e = launch_abc_sort(a, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(abc_smc_trials_kernel, grid, dim3(256), 0, s, a);
    return launch_abc_distance(a, s);
}

hipError_t launch_abc_smc_weights(const AbcSmcWeightArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(abc_smc_weights_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace epipf
