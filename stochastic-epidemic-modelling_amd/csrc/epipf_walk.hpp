// epipf_walk.hpp -- time-varying rates: the argument blocks and launchers of the random-walk filter
// and of the smoother of its parameter history (kernels in epipf_walk.hip), shared with epipf_api.cpp.
//
// The pass is one iteration of iterated filtering (epipf_if2.hpp, §17) at M = 1, m = 0 with a half-width vector per
// chain, in which every day's parameters are kept:
//   theta_hist f64 [chain][T][d][N]   theta of the particles after step p in row p, component-major
// The reduction is the fixed-lag smoother's backward window (epipf_smooth_lag.hpp, §16.1) over V = d + 1 doubles per
// particle: the d components and R = (theta[0] S) / (theta[d-1] P), +inf where the denominator is 0.
#pragma once
#include "epipf_if2.hpp"
#include "epipf_smooth.hpp"

namespace epipf {

struct WalkArgs {
    StepArgs s;                  // the filter's layout (hidden, ancestry, status, log_zeta: the context's own)
    int d;
    const double* hw;            // [max_chains][d] half-widths, by chain
    const double* start;         // [max_chains][d][N] the swarm theta_0 is jittered from
    double* hist;                // theta_hist
    size_t chain_stride;         // elements per chain of theta_hist: T d N
};

// The T launches of a call (init and T - 1 steps), the chains split over the streams as launch_if2 splits its
// searches; no host synchronisation.
hipError_t launch_walk(const WalkArgs& a, int model, int obs, int n_chains, const FilterStreams& fs);

constexpr int kWalkMaxV = kIf2MaxD + 1;      // quantities per particle
constexpr int kWalkQGroup = 4;               // quantiles whose radix histograms share one pass over the particles

struct WalkSmoothArgs {
    int n;                        // chains of this launch
    int chain0;                   // first chain: every array below is indexed by chain0 + block / days
    int day0, days;               // one workgroup per (chain, day0 + block % days)
    int T, N, C, d;
    int shift;                    // 0: a[q] (reference), 1: a[q+1] (genealogy)
    int lag;                      // 0 .. T-1
    int n_q;
    double pop;                   // the population total P
    size_t hist_stride, anc_stride, theta_stride;   // elements per chain of hidden / ancestry / theta
    const int32_t* hidden;        // [chain][T][N][C]
    const int32_t* ancestry;      // [chain][T][N]
    const double* theta;          // [chain][T][d][N]
    const int32_t* status;        // only EPIPF_STATUS_OK chains are walked, or null
    const uint32_t* ranks;        // [n_q] max(ceil(q N), 1)
    uint32_t* mrows;              // [n * days][2][N] multiplicity rows in global memory (by block), or null: LDS
    double* mean;                 // [chains][T][V]
    double* quant;                // [chains][n_q][T][V]
    int32_t* lineages;            // [chains][T]
};

hipError_t launch_walk_smooth(const WalkSmoothArgs& a, hipStream_t s);

}  // namespace epipf
