// epipf_walk_incidence.hpp -- time-varying rates from reported case counts: the argument blocks and
// launchers of the random-walk filter weighted by incidence reports, and of the kernel that forms the particles' true
// daily flows for the smoother (kernels in epipf_walk_incidence.hip), shared with epipf_api.cpp.
//
// The pass is the union of its two parents: the random-walk filter's parameters (epipf_walk.hpp, §18: theta per particle
// in theta_hist f64 [chain][T][d][N], jittered at every step with the half-widths of its chain) under the incidence
// filter's rows and weights (epipf_incidence.hpp, §19: T = D + 2 rows, the flows as differences of the parent and the
// new state, the ping-pong accumulator int32 [2][max_chains][F][N], the product weight over the reported columns).
#pragma once
#include "epipf_incidence.hpp"

namespace epipf {

struct WalkIncidenceArgs {
    StepArgs s;                  // the filter's layout, T = D + 2 (hidden, ancestry, status, log_zeta: the context's own)
    int d;
    const double* hw;            // [max_chains][d] half-widths, by chain
    const double* start;         // [max_chains][d][N] the swarm theta_0 is jittered from
    double* hist;                // theta_hist, T = D + 2 rows
    size_t chain_stride;         // elements per chain of theta_hist: T d N
    const double* counts;        // [T][F]: rows 0 and T - 1 all NaN, rows 1..D the reports (NaN: not reported)
    int32_t* acc;                // the accumulator, or null (cumulate off)
    size_t acc_half;             // elements of one of its two buffers: max_chains F N
};

// The T launches of a call (init and T - 1 = D + 1 steps), the chains split over the streams as launch_walk and
// launch_incidence split them; no host synchronisation.  rep [T] as launch_incidence's.
// nb: the kNegBin model's constants (obs == kNegBin), else null.
hipError_t launch_walk_incidence(const WalkIncidenceArgs& a, int model, int obs, bool cumulate, const uint8_t* rep,
                                 int n_chains, const FilterStreams& fs, const NegBinArgs* nb = nullptr);

// The true flows of a resident history, for the smoother to reduce as a history of F compartments:
//   flow [n][T][N][F] int32: row 0 zeros; row p >= 1, particle i: the §19 differences of hidden[p-1][ancestry[p][i]] and
//   hidden[p][i] (the day's own flow, whatever the accumulator held)
struct IncidenceFlowArgs {
    int n, T, N;
    size_t hist_stride, anc_stride;   // elements per chain of hidden / ancestry
    const int32_t* hidden;            // [chain][T][N][C]
    const int32_t* ancestry;          // [chain][T][N]
    int32_t* flow;                    // [n][T][N][F], dense
};

hipError_t launch_incidence_flows(const IncidenceFlowArgs& a, int model, hipStream_t s);

}  // namespace epipf
