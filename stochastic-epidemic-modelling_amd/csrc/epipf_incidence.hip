// epipf_incidence.hip -- incidence observations on MI355X (gfx950), DESIGN.md §19 (epipf_incidence.hpp).
//
// incidence_init_kernel / incidence_step_kernel filter on reported flows: one lane per particle, one wave per block, on
// the shared phases of epipf_step.hpp (step_total, step_degenerate, step_log_zeta, step_ancestor, step_count, step_store_weights,
// init_state, init_weights), the chain's own rates, the filter's status prologue (skipped chains) and the per-lane SSA
// (the certified f32 loop, then the exact loop for the lanes it hands back).  Their own, in the step:
//   - the parent state stays in registers across the propagate (int32 [C]);
//   - the day's flows are differences of the parent and the new state (every flow of SIR / SEIR is monotone);
//   - with CUM, a column that was not reported on day p - 1 adds the ancestor's accumulator of that day;
//   - the weight is the product over the reported columns, in column order from 1.0, of the binomial pmf (or normal
//     pdf) of the report given the accumulated flow.  The reported-column masks of days p - 1 and p are kernel
//     arguments, hence wave-uniform: an unreported column loads no count and no table entry.
#include "epipf_incidence.hpp"

#include <algorithm>

#include "epipf_step.hpp"

namespace epipf {

template <int MODEL>
__global__ __launch_bounds__(64) void incidence_init_kernel(IncidenceArgs a) {
    constexpr int C = Shape<MODEL, 1>::C;
    constexpr int F = incidence_flows(MODEL);
    constexpr int WG = 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const BlockPos bp = step_block(s);
    const int chain = bp.chain;
    const int j = bp.b * WG + (int)threadIdx.x;
    const ChainParam cp = s.cp[chain];
    if (bp.b == 0 && threadIdx.x == 0) s.status[chain] = cp.skip ? kStatusSkipped : kStatusOk;
    if (cp.skip) return;
    if (j < s.N) {
        double x[C];
        init_particle<MODEL, 1>(s, cp, j, x);
        init_state<C>(s, chain, j, x);
        if (a.acc) {                                                     // acc_0 = 0, buffer 0
#pragma unroll
            for (int k = 0; k < F; ++k) a.acc[((size_t)chain * F + k) * s.N + j] = 0;
        }
    }
    // row 0 is never reported: every particle weighs 1 (lanes past N: 0)
    init_weights<WG>(s, smem, bp, j, j < s.N, true, WG - 1, [] { return 1.0; });
}

// rep_prev / rep_cur: bit k set where column k of day p - 1 / day p is reported
// NB: empty for the binomial and normal instances, whose signature and code are what they were; the kNegBin instances
// take one NegBinArgs
template <int MODEL, int OBS, bool CUM, class... NB>
__global__ __launch_bounds__(64) void incidence_step_kernel(IncidenceArgs a, int p, int rep_prev, int rep_cur, NB... nb) {
    static_assert(sizeof...(NB) == (OBS == kNegBin ? 1 : 0), "NegBinArgs goes with kNegBin alone");
    constexpr int C = Shape<MODEL, 1>::C;
    constexpr int F = incidence_flows(MODEL);
    constexpr int WG = 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    LogTab* tab = step_logtab(smem);
    const BlockPos bp = step_block(s);
    const int chain = bp.chain;
    const int tid = threadIdx.x;
    const int j = bp.b * WG + tid;
    if (s.status[chain] != 0) return;
    const ChainParam cp = s.cp[chain];
    const int prev = (p - 1) & 1, cur = p & 1;            // the accumulator's halves, as the weights' (step_half)
    const size_t wprev = step_half(s, chain, p - 1, s.wstride), wcur = step_half(s, chain, p, s.wstride);
    const size_t bprev = step_half(s, chain, p - 1, s.bstride), bcur = step_half(s, chain, p, s.bstride);
    const double total = step_total(s, smem, bprev);
    if (!(total > 0.0)) {
        step_degenerate(s, bp, p);
        return;
    }
    step_log_zeta(s, bp, p, total);
    int anc = step_ancestor<false>(s, smem, cp, p, j, total, wprev, bprev);
    // the parent state: propagated in x, kept in xp for the flows
    double x[C];
    int32_t xp[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { x[c] = 0.0; xp[c] = 0; }
    const uint32_t ptag = ((uint32_t)p & 0xFFFFFFu) | kDomainSSA;
    bool fast_ok = true, eligible = false;
    int nev = 0, iters = 0;
    if (j < s.N) {
        anc = checked_index(anc, s.N);
        s.ancestry[(size_t)chain * s.anc_stride + (size_t)p * s.N + j] = anc;
        const int32_t* hp = s.hidden + (size_t)chain * s.hist_stride + ((size_t)(p - 1) * s.N + anc) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xp[c] = hp[c];
            x[c] = (double)xp[c];
        }
        fast_ok = fast_propagate<MODEL, 1>(x, cp, (uint32_t)j, ptag, 1.0, nev, iters, eligible);
    }
    // lanes the f32 loop could not run or could not certify: the exact loop from the untouched parent state, per lane
    // (one wave per block, so the test is block-uniform and the barrier legal)
    // (kNegBin: the weight's logs need the table as well, so a step with a reported column stages it whatever the lanes did)
    bool stage = __any(!fast_ok);
    if constexpr (OBS == kNegBin) stage = stage || (rep_cur != 0 && p + 1 < s.T);
    if (stage) {
        for (int i = tid; i < kLogTabEntries; i += WG) tab[i] = s.logtab[i];
        __syncthreads();
        if (!fast_ok) nev = exact_propagate<MODEL, 1>(x, cp, (uint32_t)j, ptag, 1.0, tab, iters);
    }
    step_count(s, nev, iters, !fast_ok);                 // lanes past N hold fast_ok = true
    double w = 0.0;
    if (j < s.N) {
        int32_t xn[C];
        int32_t* hc = s.hidden + (size_t)chain * s.hist_stride + ((size_t)p * s.N + j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xn[c] = (int32_t)x[c];
            hc[c] = xn[c];
        }
        if (p + 1 < s.T) {                               // the last row is weighted by nothing and followed by no step
            int32_t acc[F];
            acc[0] = xp[0] - xn[0];                                              // S' - S
            if constexpr (MODEL == kSIR) {
                acc[1] = xn[2] - xp[2];                                          // R - R'
            } else {
                acc[1] = (xn[2] + xn[3]) - (xp[2] + xp[3]);                      // (I + R) - (I' + R')
                acc[2] = xn[3] - xp[3];                                          // R - R'
            }
            if constexpr (CUM) {
                const int32_t* from = a.acc + (size_t)prev * a.acc_half + (size_t)chain * F * s.N;
                int32_t* to = a.acc + (size_t)cur * a.acc_half + (size_t)chain * F * s.N;
#pragma unroll
                for (int k = 0; k < F; ++k) {
                    if (!((rep_prev >> k) & 1)) acc[k] += from[(size_t)k * s.N + anc];   // uniform branch
                    to[(size_t)k * s.N + j] = acc[k];
                }
            }
            w = 1.0;
            const double* yrow = a.counts + (size_t)p * F;
            if constexpr (OBS == kNegBin) {
                const NegBinArgs& g = negbin_args(nb...);
                const double EPIPF_CONSTANT* kc = (const double EPIPF_CONSTANT*)g.chain + (size_t)chain * 2;
                const double EPIPF_CONSTANT* crow = (const double EPIPF_CONSTANT*)g.coeff + ((size_t)chain * s.T + p) * F;
                const double kappa = kc[0], logk = kc[1];
#pragma unroll
                for (int k = 0; k < F; ++k)
                    if ((rep_cur >> k) & 1)                                              // uniform branch
                        w = w * negbin_factor(yrow[k], (double)acc[k], cp.probs, crow[k], kappa, logk, tab);
            } else {
#pragma unroll
                for (int k = 0; k < F; ++k)
                    if ((rep_cur >> k) & 1)                                              // uniform branch
                        w = w * incidence_factor<OBS>(yrow[k], (double)acc[k], cp, s.lf, s.lf_max);
            }
        }
    }
    step_store_weights(s, smem, bp.b, j, p, w, wcur, bcur);
}

template <int MODEL, int OBS, bool CUM, class... NB>
static hipError_t launch_incidence_t(const IncidenceArgs& a, const uint8_t* rep, int n_chains, const FilterStreams& fs,
                                     NB... nb) {
    const StepArgs& s0 = a.s;
    const size_t lds = step_lds_bytes(s0.B, 64);
    launch_chain_groups(s0, n_chains, fs, 64, [&](int, const StepArgs& sg, int, dim3 grid, hipStream_t st) {
        IncidenceArgs ag = a;
        ag.s = sg;
        hipLaunchKernelGGL((incidence_init_kernel<MODEL>), grid, dim3(64), lds, st, ag);
        for (int p = 1; p < s0.T; ++p)
            hipLaunchKernelGGL((incidence_step_kernel<MODEL, OBS, CUM, NB...>), grid, dim3(64), lds, st, ag, p,
                               (int)rep[p - 1], (int)rep[p], nb...);
    });
    return hipGetLastError();
}

template <int MODEL>
static hipError_t launch_incidence_m(const IncidenceArgs& a, int obs, bool cumulate, const uint8_t* rep, int n_chains,
                                     const FilterStreams& fs, const NegBinArgs* nb) {
    if (obs == kNegBin)
        return cumulate ? launch_incidence_t<MODEL, kNegBin, true>(a, rep, n_chains, fs, *nb)
                        : launch_incidence_t<MODEL, kNegBin, false>(a, rep, n_chains, fs, *nb);
    if (obs == kBinomial)
        return cumulate ? launch_incidence_t<MODEL, kBinomial, true>(a, rep, n_chains, fs)
                        : launch_incidence_t<MODEL, kBinomial, false>(a, rep, n_chains, fs);
    return cumulate ? launch_incidence_t<MODEL, kNormal, true>(a, rep, n_chains, fs)
                    : launch_incidence_t<MODEL, kNormal, false>(a, rep, n_chains, fs);
}

hipError_t launch_incidence(const IncidenceArgs& a, int model, int obs, bool cumulate, const uint8_t* rep, int n_chains,
                            const FilterStreams& fs, const NegBinArgs* nb) {
    if (a.s.wg != 64 || a.s.lanes != 1 || a.s.T < 3 || !a.counts || !rep || (cumulate && !a.acc))
        return hipErrorInvalidValue;
    if (obs != kBinomial && obs != kNormal && obs != kNegBin) return hipErrorInvalidValue;
    if ((obs == kNegBin) != (nb != nullptr) || (nb && (!nb->coeff || !nb->chain))) return hipErrorInvalidValue;
    if (model == kSIR) return launch_incidence_m<kSIR>(a, obs, cumulate, rep, n_chains, fs, nb);
    if (model == kSEIR) return launch_incidence_m<kSEIR>(a, obs, cumulate, rep, n_chains, fs, nb);
    return hipErrorInvalidValue;
}

}  // namespace epipf
