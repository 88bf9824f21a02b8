// epipf_smooth.hpp -- argument blocks and launchers of the particle smoother (epipf_smooth, epipf_smooth_history;
// kernels in epipf_smooth.hip).
//
// For one chain with history h[T][N][C], a[T][N] and shift in {0, 1}:
//   m[T-1][i] = 1;   m[p][i] = sum of m[p+1][j] over the j with a[p+shift][j] == i,   p = T-2 .. 0
//   sums[p][c] = sum_i m[p][i] h[p][i][c];   hist[p][c][v] = sum of m[p][i] over the i with h[p][i][c] == v
//   lineages[p] = #{i : m[p][i] > 0}
// shift 0 is the reference's particle_path_sampler indexing, shift 1 the true genealogy; `predictive` sets m = 1 on
// every day (no backward pass).  Integers only: every order of arrival gives the same result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace epipf {

struct SmoothArgs {
    int n;                        // chains of this launch (one workgroup each)
    int chain0;                   // first chain: history, status, sums and lineages are indexed by chain0 + block
    int T, N, C;
    int shift;                    // 0: a[p] (reference), 1: a[p+1] (genealogy)
    int predictive;               // 1: m = 1 on every day
    int bins;                     // histogram bins per (day, compartment): values 0..bins-1, larger ones are dropped
    size_t hist_stride, anc_stride;   // elements per chain of hidden / ancestry
    const int32_t* hidden;
    const int32_t* ancestry;
    const int32_t* status;        // the last run's chain status (only EPIPF_STATUS_OK chains are walked), or null
    uint32_t* mrows;              // [n][2][N] multiplicity rows in global memory (by block), or null: they live in LDS
    unsigned long long* sums;     // [chains][T][C]
    int32_t* lineages;            // [chains][T]
    uint32_t* hist;               // [n][T][C][bins] (by block), zeroed by the host, or null
};

struct SmoothQuantArgs {
    int n, chain0, T, C, bins, n_q;
    uint32_t max_rank;            // the largest of ranks[]: no cell is scanned past it
    const int32_t* status;        // as SmoothArgs
    const uint32_t* hist;         // [n][T][C][bins] (by chain - chain0)
    const uint32_t* ranks;        // [n_q] max(ceil(q N), 1): the same for every cell, since sum_i m[p][i] = N
    int32_t* quant;               // [chains][n_q][T][C]; `bins` where a cell's counts never reach the rank
};

constexpr int kSmoothThreads = 1024;          // largest workgroup of smooth_kernel (64 up to N = 64, then 64-multiples)
constexpr int kSmoothMaxN = 1 << 30;            // particles per chain
constexpr int kSmoothMaxC = 64;               // compartments whose sums a workgroup keeps in LDS
constexpr int kSmoothLdsMaxN = 16384;         // two uint32 rows of N in LDS up to here (128 KiB), beyond in global memory
constexpr size_t kSmoothLdsDefault = 64 * 1024;   // dynamic LDS a launch may take without opting in

int smooth_threads(int N);
hipError_t launch_smooth(const SmoothArgs& a, hipStream_t s);
hipError_t launch_smooth_quantiles(const SmoothQuantArgs& a, hipStream_t s);

}  // namespace epipf
