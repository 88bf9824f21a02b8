// epipf_if2_sub.hpp -- iterated filtering for the subgroup models at G = 2..kMaxLaneG: the argument
// block and the launcher of the kernels in epipf_if2_sub.hip, shared with epipf_api.cpp
// (epipf_iterated_filtering_subgroups).
//
// The definition is §17's with d = G*G + 1 and theta laid out as beta[G][G] row-major, then gamma (ChainParam::theta's
// layout).  The kernels are epipf_if2.hip's with G as a template parameter; If2Args and its kernels stay as they are
// (their layout is what those kernels' register allocation was measured against), so the wider half-width table has a
// block of its own here.
#pragma once
#include "epipf_if2.hpp"

namespace epipf {

struct If2SubArgs {
    StepArgs s;                  // the filter's layout; s.log_zeta: this iteration's [max_chains][T] rows
    int d, m, M;                 // components (G*G + 1); this iteration; iterations of the call
    double hw[kLaneTheta];       // this iteration's half-widths
    double* swarm;               // f64 [2][max_chains][d][N], as If2Args::swarm
    double* start;               // f64 [max_chains][d][N]
};

// launch_if2 for the subgroup models: a (its hw unused) gives the layout, the buffers and M; G = 2..kMaxLaneG.
hipError_t launch_if2_sub(const If2Args& a, int model, int G, int obs, int n_searches, const double* half_widths,
                          const FilterStreams& fs);

}  // namespace epipf
