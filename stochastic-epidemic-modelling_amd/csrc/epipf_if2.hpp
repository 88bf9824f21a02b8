// epipf_if2.hpp -- iterated filtering (IF2): the argument block and the launcher of the kernels in
// epipf_if2.hip, shared with epipf_api.cpp (epipf_if2).
//
// One iteration is one pass of the filter (pf_init_kernel / pf_step_kernel, epipf_kernels.hpp) in which every particle
// carries its own parameter vector: jittered at every step on the stream domain 7 << 24, gathered from the particle's
// ancestor at resampling, and used as that lane's rates in the SSA.  A search is a "chain" of the filter's batch: the
// weights, the resampling search, the history and the status are the filter's own buffers and code.
#pragma once
#include "epipf_internal.hpp"

namespace epipf {

constexpr uint32_t kDomainIf2 = 7u << 24;    // theta perturbation draws (domains 0-6: SSA, resampling, init, ABC, ABC-SMC)
constexpr int kIf2MaxD = 3;                  // SIR (beta, gamma), SEIR (beta, alpha, gamma)

// The swarm on the device, component-major so that a wave's loads and stores of one component are contiguous:
//   swarm f64 [2][max_chains][d][N]   theta of the particles after step p in buffer p & 1 (as the weights)
//   start f64 [max_chains][d][N]      the swarm the running iteration started from (what a degenerate search returns)
struct If2Args {
    StepArgs s;                  // the filter's layout; s.log_zeta: this iteration's [max_chains][T] rows
    int d, m, M;                 // components; this iteration; iterations of the call
    double hw[kIf2MaxD];         // this iteration's half-widths
    double* swarm;
    double* start;
    double* mean;                // [max_chains][M][d] swarm means after each completed iteration
    int32_t* done;               // [max_chains] completed iterations
};

// All M x (T + 1) launches of a call (init, T - 1 steps and the end-of-iteration reduction per iteration), the searches
// split over the streams as launch_filter_t splits chains; no host synchronisation.  half_widths [M][d].
hipError_t launch_if2(const If2Args& a, int model, int obs, int n_searches, const double* half_widths,
                      const FilterStreams& fs);

// The end-of-iteration reduction (if2_finish_kernel) of a.m for the n_g searches from a.s.chain0 on, enqueued on st; it
// reads a.d, so it serves every model's swarm (epipf_if2_sub.hip).
void launch_if2_finish(const If2Args& a, int n_g, hipStream_t st);

}  // namespace epipf
