// epipf_incidence.hip -- incidence observations on MI355X (gfx950), DESIGN.md §19 (epipf_incidence.hpp).
//
// incidence_init_kernel / incidence_step_kernel are walk_init_kernel / walk_step_kernel (epipf_walk.hip) without the
// per-particle parameters and with another weight: one lane per particle, one wave per block, the same block-sum
// prefix, certified search, counters and SSA.  What is new in the step:
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
        int32_t* h = s.hidden + (size_t)chain * s.hist_stride + (size_t)j * C;
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = (int32_t)x[c];
        s.ancestry[(size_t)chain * s.anc_stride + j] = 0;
        if (a.acc) {                                                     // acc_0 = 0, buffer 0
#pragma unroll
            for (int k = 0; k < F; ++k) a.acc[((size_t)chain * F + k) * s.N + j] = 0;
        }
    }
    if (bp.b == 0 && threadIdx.x == 0) s.log_zeta[(size_t)chain * s.T] = 0.0;
    // row 0 is never reported: every particle weighs 1 (lanes past N: 0)
    const double w = j < s.N ? 1.0 : 0.0;
    const size_t wbase = (size_t)chain * s.wstride;                      // buffer 0
    const double loc = block_inclusive_scan<WG>(w, smem);
    s.wraw[wbase + j] = w;                                               // every lane: the in-block search reads the
    s.wloc[wbase + j] = loc;                                             // whole block of the weight layout (B x 64)
    if ((int)threadIdx.x == WG - 1) s.bsum[(size_t)chain * s.bstride + bp.b] = loc;
}

// One column's factor: oracle.binom_pmf(y, n, p) = exp(hi) (1 + lo) of the compensated log pmf with its special cases
// (NaN for a bad p, 0 outside the support), or oracle.norm_pdf(y, n, probs).
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

// rep_prev / rep_cur: bit k set where column k of day p - 1 / day p is reported
template <int MODEL, int OBS, bool CUM>
__global__ __launch_bounds__(64) void incidence_step_kernel(IncidenceArgs a, int p, int rep_prev, int rep_cur) {
    constexpr int C = Shape<MODEL, 1>::C;
    constexpr int F = incidence_flows(MODEL);
    constexpr int WG = 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    LogTab* tab = reinterpret_cast<LogTab*>(smem);       // the layout of pf_step_kernel (step_lds_bytes)
    double* red = smem + 2 * kLogTabEntries;
    double* seg_start = red + 16;
    double* seg_end = seg_start + s.nseg;
    const BlockPos bp = step_block(s);
    const int chain = bp.chain;
    const int tid = threadIdx.x;
    const int j = bp.b * WG + tid;
    if (s.status[chain] != 0) return;
    const ChainParam cp = s.cp[chain];
    const int prev = (p - 1) & 1, cur = p & 1;
    const size_t wprev = ((size_t)prev * s.max_chains + chain) * s.wstride;
    const size_t wcur = ((size_t)cur * s.max_chains + chain) * s.wstride;
    const size_t bprev = ((size_t)prev * s.max_chains + chain) * s.bstride;
    const size_t bcur = ((size_t)cur * s.max_chains + chain) * s.bstride;

    // likelihood of the reports up to day p - 1: zetas[p] = zetas[p-1] * mean(w), in log space (pf_step_kernel)
    const double total = (s.seg == 1) ? scan_block_sums<WG>(s.bsum + bprev, s.B, seg_start + s.B, seg_start, red)
                                      : scan_segments(s.bsum + bprev, s.B, s.seg, s.nseg, seg_start, seg_end);
    if (!(total > 0.0)) {                                // all weights 0 or NaN: this chain ends here
        if (bp.b == 0 && tid == 0) {
            s.status[chain] = kStatusDegenerate;
            s.log_zeta[(size_t)chain * s.T + p] = -__builtin_inf();
        }
        return;
    }
    if (bp.b == 0 && tid == 0)
        s.log_zeta[(size_t)chain * s.T + p] = s.log_zeta[(size_t)chain * s.T + p - 1] + log(total / (double)s.N);

    // multinomial draw and certified search, exactly the filter's
    double U = 0.0;
    int anc = 0;
    bool certified = true, ambiguous = false;
    if (j < s.N) {
        const Block r = philox(0u, (uint32_t)j, ((uint32_t)p & 0xFFFFFFu) | kDomainResample, cp.f, cp.k0, cp.k1);
        U = u01(r.x, r.y);
        if (s.seg == 1)
            anc = resample_search<WG>(U, seg_start + s.B, seg_start, s.B, total, s.wloc + wprev, s.N, s.cert_k,
                                      certified, 0.0, ambiguous);
        else
            anc = resample_search_seg(U, seg_start, seg_end, s.nseg, s.seg, s.bsum + bprev, s.B, total,
                                      s.wloc + wprev, WG, s.N, s.cert_k, certified, 0.0, ambiguous);
    }
    if (__any(!certified)) {   // wave-uniform: the whole wave resolves its uncertified draws exactly
        const int e = resample_exact_wave(!certified, U, s.wraw + wprev, s.N);
        if (!certified) {
            anc = e;
            atomicAdd(counter_slot(s.counters) + 1, 1ull);
        }
    }
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
    if (__any(!fast_ok)) {
        for (int i = tid; i < kLogTabEntries; i += WG) tab[i] = s.logtab[i];
        __syncthreads();
        if (!fast_ok) nev = exact_propagate<MODEL, 1>(x, cp, (uint32_t)j, ptag, 1.0, tab, iters);
    }
    if (s.count_events) {  // pf_step_kernel's counters
        unsigned long long e = (unsigned long long)nev, li = (unsigned long long)iters;
        int wmax = iters;
        for (int o = 32; o > 0; o >>= 1) {
            e += __shfl_xor(e, o, 64);
            li += __shfl_xor(li, o, 64);
            wmax = max(wmax, __shfl_xor(wmax, o, 64));
        }
        const unsigned long long ex = __ballot(!fast_ok);             // lanes past N hold fast_ok = true
        if (tid == 0) {
            unsigned long long* slot = counter_slot(s.counters);
            atomicAdd(slot, e);
            atomicAdd(slot + 2, li);
            atomicAdd(slot + 3, 64ull * (unsigned long long)wmax);
            atomicAdd(slot + 4, (unsigned long long)__popcll(ex));
            atomicAdd(slot + 5, ex ? 1ull : 0ull);
        }
    }
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
#pragma unroll
            for (int k = 0; k < F; ++k)
                if ((rep_cur >> k) & 1)                                                  // uniform branch
                    w = w * incidence_factor<OBS>(yrow[k], (double)acc[k], cp, s.lf, s.lf_max);
        }
    }
    if (p + 1 < s.T) {
        const double loc = block_inclusive_scan<WG>(w, red);
        s.wraw[wcur + j] = w;                            // lanes past N: 0 and the block's sum, in the weight layout's
        s.wloc[wcur + j] = loc;                          // own padding (B x 64 slots); they touch no particle array
        if (tid == WG - 1) s.bsum[bcur + bp.b] = loc;
    }
}

template <int MODEL, int OBS, bool CUM>
static hipError_t launch_incidence_t(const IncidenceArgs& a, const uint8_t* rep, int n_chains, const FilterStreams& fs) {
    const StepArgs& s0 = a.s;
    const size_t lds = step_lds_bytes(s0.B, 64);
    const int S = std::max(1, std::min(fs.n, n_chains));
    for (int g = 0; g < S; ++g) {
        IncidenceArgs ag = a;
        ag.s.chain0 = (int)((long)n_chains * g / S);
        const int n_g = (int)((long)n_chains * (g + 1) / S) - ag.s.chain0;
        const hipStream_t st = fs.s[g];
        ag.s.xcd_map = s0.xcd_map && (long)s0.B * n_g * 64 < (1L << 31);
        const dim3 grid = ag.s.xcd_map ? dim3(s0.B * n_g) : dim3(s0.B, n_g), block(64);
        hipLaunchKernelGGL((incidence_init_kernel<MODEL>), grid, block, lds, st, ag);
        for (int p = 1; p < s0.T; ++p)
            hipLaunchKernelGGL((incidence_step_kernel<MODEL, OBS, CUM>), grid, block, lds, st, ag, p, (int)rep[p - 1],
                               (int)rep[p]);
        if (g > 0) (void)hipEventRecord(fs.join[g], st);
    }
    for (int g = 1; g < S; ++g) (void)hipStreamWaitEvent(fs.s[0], fs.join[g], 0);
    return hipGetLastError();
}

template <int MODEL>
static hipError_t launch_incidence_m(const IncidenceArgs& a, int obs, bool cumulate, const uint8_t* rep, int n_chains,
                                     const FilterStreams& fs) {
    if (obs == kBinomial)
        return cumulate ? launch_incidence_t<MODEL, kBinomial, true>(a, rep, n_chains, fs)
                        : launch_incidence_t<MODEL, kBinomial, false>(a, rep, n_chains, fs);
    return cumulate ? launch_incidence_t<MODEL, kNormal, true>(a, rep, n_chains, fs)
                    : launch_incidence_t<MODEL, kNormal, false>(a, rep, n_chains, fs);
}

hipError_t launch_incidence(const IncidenceArgs& a, int model, int obs, bool cumulate, const uint8_t* rep, int n_chains,
                            const FilterStreams& fs) {
    if (a.s.wg != 64 || a.s.lanes != 1 || a.s.T < 3 || !a.counts || !rep || (cumulate && !a.acc))
        return hipErrorInvalidValue;
    if (obs != kBinomial && obs != kNormal) return hipErrorInvalidValue;
    if (model == kSIR) return launch_incidence_m<kSIR>(a, obs, cumulate, rep, n_chains, fs);
    if (model == kSEIR) return launch_incidence_m<kSEIR>(a, obs, cumulate, rep, n_chains, fs);
    return hipErrorInvalidValue;
}

}  // namespace epipf
