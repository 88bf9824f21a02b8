// epipf_smooth_lag.hpp -- argument block and launcher of the fixed-lag particle smoother (epipf_smooth_lag,
// epipf_smooth_lag_history; kernel in epipf_smooth_lag.hip).
//
// For one chain with history h[T][N][C], a[T][N], shift in {0, 1} (epipf_smooth.hpp) and a lag L >= 0, day p is
// estimated from the particles of day e(p) = min(p + L, T-1) traced back to day p:
//   w[e(p)][i] = 1;   w[q][i] = sum of w[q+1][j] over the j with a[q+shift][j] == i,   q = e(p)-1 .. p;   m[p] = w[p]
//   sums[p][c] = sum_i m[p][i] h[p][i][c];   hist[p][c][v] = sum of m[p][i] over the i with h[p][i][c] == v
//   lineages[p] = #{i : m[p][i] > 0}
// L = 0 is the particle cloud (m = 1), L >= T-1 the smoother of epipf_smooth.hpp.  sum_i m[p][i] = N on every day, so
// the histogram is smooth_quantile_kernel's.  Integers only: every order of arrival gives the same result.
#pragma once
#include "epipf_smooth.hpp"

namespace epipf {

struct SmoothLagArgs {
    int n;                        // chains of this launch
    int chain0;                   // first chain: history, status, sums and lineages are indexed by chain0 + block / days
    int day0, days;               // the days of this launch: one workgroup per (chain, day0 + block % days)
    int T, N, C;
    int shift;                    // 0: a[q] (reference), 1: a[q+1] (genealogy)
    int lag;                      // 0 .. T-1 (the host clamps a larger one)
    int bins;                     // as SmoothArgs
    size_t hist_stride, anc_stride;   // elements per chain of hidden / ancestry
    const int32_t* hidden;
    const int32_t* ancestry;
    const int32_t* status;        // as SmoothArgs
    uint32_t* mrows;              // [n * days][2][N] multiplicity rows in global memory (by block), or null: LDS
    unsigned long long* sums;     // [chains][T][C]
    int32_t* lineages;            // [chains][T]
    uint32_t* hist;               // [n][T][C][bins] (by chain - chain0), zeroed by the host, or null
};

constexpr int kSmoothLagMaxBlocks = 1 << 24;  // workgroups of one launch (the host slices chains and days under it)

hipError_t launch_smooth_lag(const SmoothLagArgs& a, hipStream_t s);

}  // namespace epipf
