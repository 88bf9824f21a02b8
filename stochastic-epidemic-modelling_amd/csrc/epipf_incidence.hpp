// epipf_incidence.hpp -- incidence observations: the argument block and launcher of the filter that is
// weighted by reported transition counts instead of the compartments (kernels in epipf_incidence.hip), shared with
// epipf_api.cpp.
//
// The pass is the filter's own loop over T = D + 2 rows (row 0: the initial draw, rows 1..D: the days, row D + 1: one
// more resampling on day D's weights), with the weight of particle j on day p taken from its flows of that day,
//   SIR   infections S' - S, removals R - R'                      SEIR  exposures S' - S, onsets (I + R) - (I' + R'),
//                                                                       removals R - R'
// (x' the parent state hidden[p-1][a_p[j]], x the new one), optionally accumulated since the column's previous report:
//   acc int32 [2][max_chains][F][N]   column-major ping-pong, buffer p & 1 written at step p (and buffer 0 zeroed by
//                                     the init kernel), read at step p + 1 by ancestor
#pragma once
#include "epipf_internal.hpp"

namespace epipf {

constexpr int kIncidenceMaxF = 3;
// The third observation model of the incidence filters alone (EPIPF_OBS_NEGBIN): the report is negative
// binomial with mean probs x flow and the chain's dispersion.  Obs (epipf_device.hpp) stays the filters' two.
constexpr int kNegBin = 2;
__host__ __device__ constexpr int incidence_flows(int model) { return model == kSIR ? 2 : 3; }

struct IncidenceArgs {
    StepArgs s;                  // the filter's layout, T = D + 2 (hidden, ancestry, status, log_zeta: the context's own)
    const double* counts;        // [T][F]: rows 0 and T - 1 all NaN, rows 1..D the reports (NaN: not reported)
    int32_t* acc;                // the accumulator, or null (cumulate off)
    size_t acc_half;             // elements of one of its two buffers: max_chains F N
};

// The negative-binomial model's per-chain constants, in device buffers that no kernel writes, indexed by
// the block's chain and read through EPIPF_CONSTANT (scalar loads).  A trailing argument of the kNegBin instances
// alone: ChainParam, StepArgs and IncidenceArgs stay what the binomial and normal instances were compiled against
// (DESIGN.md §6.5).
struct NegBinArgs {
    const double* coeff;         // [chains][T][F]: c(y, kappa) = lgamma(y + kappa) - lgamma(kappa) - lgamma(y + 1) of the
                                 // chain's dispersion and counts[p][k], binary128 rounded once (0 where not reported)
    const double* chain;         // [chains][2]: kappa, log kappa
};
// the one trailing argument of a kNegBin instance (the other instances have none)
__host__ __device__ inline const NegBinArgs& negbin_args(const NegBinArgs& nb) { return nb; }

// The T launches of a call (init and T - 1 steps), the chains split over the streams as launch_walk splits them; no
// host synchronisation.  rep [T]: bit k of rep[p] set where counts[p][k] is reported (the host's copy of the mask, a
// kernel argument of each step: wave-uniform without a load).
// nb: the kNegBin model's constants (obs == kNegBin), else null.
hipError_t launch_incidence(const IncidenceArgs& a, int model, int obs, bool cumulate, const uint8_t* rep, int n_chains,
                            const FilterStreams& fs, const NegBinArgs* nb = nullptr);

// One column's factor: oracle.binom_pmf(y, n, p) = exp(hi) (1 + lo) of the compensated log pmf with its special cases
// (NaN for a bad p, 0 outside the support), or oracle.norm_pdf(y, n, probs).  Shared by the step kernels of
// epipf_incidence.hip and epipf_walk_incidence.hip.
template <int OBS>
__device__ __forceinline__ double incidence_factor(double y, double n, const ChainParam& cp, const double* lf,
                                                   int lf_max) {
    if constexpr (OBS == kNormal) {
        return normal_pdf(y, n, cp.probs);
    } else {
        const LogW L = binom_logpmf(y, n, cp, lf, lf_max);
        if (isnan(L.hi)) return L.hi;
        const double e = exp(L.hi);
        return fma(e, L.lo, e);
    }
}

// One column's negative-binomial factor (operation for operation): mean m = probs n, a point mass at 0
// where the mean is 0, else exp(L) with L = (c + kappa (log kappa - log t)) + y (log m - log t), t = kappa + m, in plain
// doubles without contraction.  log is glibc's (tab: the table in LDS); c, kappa and log kappa are the host's.  m and
// t are normal doubles: the host refuses subnormal probs and dispersions and a probs large enough to overflow m.
__device__ __forceinline__ double negbin_factor(double y, double n, double rho, double c, double kappa, double logk,
                                                const LogTab* tab) {
    const double m = rho * n;
    if (!(m > 0.0)) return y == 0.0 ? 1.0 : 0.0;
    const double t = kappa + m;
    const double lt = glibc_log(t, tab);
    const double L = (c + kappa * (logk - lt)) + y * (glibc_log(m, tab) - lt);
    return exp(L);
}

}  // namespace epipf
