// epipf_if2_sub.hip -- the iterated-filtering kernels of the subgroup models (G = 2..4) for MI355X (gfx950) and their
// launcher.
//
// if2_sub_init_kernel / if2_sub_step_kernel filter with theta per particle and G groups: one lane per particle, one wave
// per block, on the shared phases of epipf_step.hpp (step_total, step_ancestor, step_count, step_store_weights,
// step_degenerate, step_log_zeta, init_state, init_weights) with IF2's status rule and filter index (epipf_if2.hip).
// theta is
// beta[G][G] row-major then gamma, D = G*G + 1 components per particle: gathered from the ancestor out of the
// component-major swarm, jittered on domain 7 << 24 (component c from block c / 2), stored, and used as the lane's own
// rates (a per-lane ChainParam copy: theta for the exact loop, thetaf for the certified f32 loop).  The loops over the
// components are fully unrolled so that the rates stay in registers (FastSubgroups reads them through a pointer).  No
// wave-cooperative replay: it takes one wave-uniform ChainParam.  The end-of-iteration reduction is if2_finish_kernel.
#include "epipf_if2_sub.hpp"

#include <algorithm>

#include "epipf_step.hpp"

namespace epipf {

// theta[c] + hw[c] (2u - 1), reflected at 0; component c draws from block c / 2 of (., j, tag, f): words (0, 1) for
// even c, (2, 3) for odd c.  No contraction (-ffp-contract=off): the restatement's roundings.
template <int D>
__device__ __forceinline__ void if2_sub_perturb(double* th, const If2SubArgs& a, uint32_t j, uint32_t tag,
                                                const ChainParam& cp) {
#pragma unroll
    for (int b = 0; b < (D + 1) / 2; ++b) {
        const Block r = philox((uint32_t)b, j, tag, cp.f, cp.k0, cp.k1);
        {
            const double u = u01(r.x, r.y);
            const double t = th[2 * b] + a.hw[2 * b] * (2.0 * u - 1.0);
            th[2 * b] = (t < 0.0) ? -t : t;
        }
        if (2 * b + 1 < D) {
            const double u = u01(r.z, r.w);
            const double t = th[2 * b + 1] + a.hw[2 * b + 1] * (2.0 * u - 1.0);
            th[2 * b + 1] = (t < 0.0) ? -t : t;
        }
    }
}

template <int MODEL, int G, int OBS>
__global__ __launch_bounds__(64) void if2_sub_init_kernel(If2SubArgs a) {
    static_assert(MODEL >= kSubgroups && G >= 2 && G <= kMaxLaneG, "the subgroup models with per-lane rates");
    constexpr int C = Shape<MODEL, G>::C;
    constexpr int D = G * G + 1;
    constexpr int WG = 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const BlockPos bp = step_block(s);
    const int chain = bp.chain;
    const int j = bp.b * WG + (int)threadIdx.x;
    ChainParam cp = s.cp[chain];
    cp.f += (uint32_t)a.m;
    // the first iteration starts every search; a search that degenerated in an earlier one stays as it ended
    if (a.m == 0) {
        if (bp.b == 0 && threadIdx.x == 0) s.status[chain] = kStatusOk;
    } else if (s.status[chain] != 0) {
        return;
    }
    double x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    if (j < s.N) {
        init_particle<MODEL, G>(s, cp, j, x);                            // pmcmc.py:156-175
        init_state<C>(s, chain, j, x);
        double th[D];
#pragma unroll
        for (int c = 0; c < D; ++c) th[c] = a.start[((size_t)chain * D + c) * s.N + j];
        if2_sub_perturb<D>(th, a, (uint32_t)j, kDomainIf2, cp);          // step 0
#pragma unroll
        for (int c = 0; c < D; ++c) a.swarm[((size_t)chain * D + c) * s.N + j] = th[c];   // buffer 0
    }
    init_weights<WG>(s, smem, bp, j, j < s.N, true, WG - 1, [&] {
        return particle_weight<MODEL, G, OBS>(x, s.Y, cp, s.cp + chain, s.lf, s.lf_max,
                                              s.hidden + (size_t)chain * s.hist_stride + (size_t)j * C);
    });
}

template <int MODEL, int G, int OBS>
__global__ __launch_bounds__(64) void if2_sub_step_kernel(If2SubArgs a, int p) {
    static_assert(MODEL >= kSubgroups && G >= 2 && G <= kMaxLaneG, "the subgroup models with per-lane rates");
    constexpr int C = Shape<MODEL, G>::C;
    constexpr int K = Shape<MODEL, G>::K;
    constexpr int D = G * G + 1;
    constexpr int WG = 64;
    static_assert(D <= kLaneTheta, "ChainParam::theta holds the lane's rates");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    LogTab* tab = step_logtab(smem);
    const BlockPos bp = step_block(s);
    const int chain = bp.chain;
    const int tid = threadIdx.x;
    const int j = bp.b * WG + tid;
    if (s.status[chain] != 0) return;
    ChainParam cp = s.cp[chain];
    cp.f += (uint32_t)a.m;
    const int prev = (p - 1) & 1, cur = p & 1;            // the swarm's halves, as the weights' (step_half)
    const size_t wprev = step_half(s, chain, p - 1, s.wstride), wcur = step_half(s, chain, p, s.wstride);
    const size_t bprev = step_half(s, chain, p - 1, s.bstride), bcur = step_half(s, chain, p, s.bstride);
    const double total = step_total(s, smem, bprev);
    if (!(total > 0.0)) {
        step_degenerate(s, bp, p);
        return;
    }
    step_log_zeta(s, bp, p, total);
    int anc = step_ancestor<false>(s, smem, cp, p, j, total, wprev, bprev);
    // the ancestor's theta, jittered: this particle's rates.  The lane's own ChainParam copy differs from the chain's
    // in theta and thetaf only.  Lanes past N keep the chain's zeroed theta and run no SSA.
    double x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    const uint32_t ptag = ((uint32_t)p & 0xFFFFFFu) | kDomainSSA;
    ChainParam lcp = cp;
    bool fast_ok = true, eligible = false;
    int nev = 0, iters = 0;
    if (j < s.N) {
        anc = checked_index(anc, s.N);
        s.ancestry[(size_t)chain * s.anc_stride + (size_t)p * s.N + j] = anc;
        double th[D];
#pragma unroll
        for (int c = 0; c < D; ++c) th[c] = a.swarm[(((size_t)prev * s.max_chains + chain) * D + c) * s.N + anc];
        if2_sub_perturb<D>(th, a, (uint32_t)j, ((uint32_t)p & 0xFFFFFFu) | kDomainIf2, cp);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            a.swarm[(((size_t)cur * s.max_chains + chain) * D + c) * s.N + j] = th[c];
            lcp.theta[c] = th[c];
            lcp.thetaf[c] = (float)th[c];
        }
        const int32_t* hp = s.hidden + (size_t)chain * s.hist_stride + ((size_t)(p - 1) * s.N + anc) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (double)hp[c];
        fast_ok = fast_propagate<MODEL, G>(x, lcp, (uint32_t)j, ptag, 1.0, nev, iters, eligible);
    }
    // lanes the f32 loop could not run or could not certify at the step boundary: the exact loop from the untouched
    // parent state, per lane.  Its log table goes to LDS only in waves that need it (one wave per block, so the test
    // is block-uniform and the barrier legal).
    if (__any(!fast_ok)) {
        for (int i = tid; i < kLogTabEntries; i += WG) tab[i] = s.logtab[i];
        __syncthreads();
        if (!fast_ok) nev = exact_propagate<MODEL, G>(x, lcp, (uint32_t)j, ptag, 1.0, tab, iters);
    }
    step_count(s, nev, iters, !fast_ok);                 // lanes past N hold fast_ok = true
    double w = 0.0;
    if (j < s.N) {
        int32_t* hc = s.hidden + (size_t)chain * s.hist_stride + ((size_t)p * s.N + j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) hc[c] = (int32_t)x[c];
        if (p + 1 < s.T) w = particle_weight<MODEL, G, OBS>(x, s.Y + (size_t)p * K, cp, s.cp + chain, s.lf, s.lf_max, hc);
    }
    step_store_weights(s, smem, bp.b, j, p, w, wcur, bcur);
}

template <int MODEL, int G, int OBS>
static hipError_t launch_if2_sub_t(const If2Args& a, int n_searches, const double* half_widths, const FilterStreams& fs) {
    const StepArgs& s0 = a.s;
    const size_t lds = step_lds_bytes(s0.B, 64);
    launch_chain_groups(s0, n_searches, fs, 64, [&](int, const StepArgs& sg, int n_g, dim3 grid, hipStream_t st) {
        If2Args fin = a;                                 // if2_finish_kernel's block: the same layout and buffers
        If2SubArgs ag{};
        ag.s = sg; ag.d = a.d; ag.M = a.M; ag.swarm = a.swarm; ag.start = a.start;
        for (int m = 0; m < a.M; ++m) {
            ag.m = m;
            for (int c = 0; c < a.d; ++c) ag.hw[c] = half_widths[(size_t)m * a.d + c];
            ag.s.log_zeta = s0.log_zeta + (size_t)m * s0.max_chains * s0.T;
            hipLaunchKernelGGL((if2_sub_init_kernel<MODEL, G, OBS>), grid, dim3(64), lds, st, ag);
            for (int p = 1; p < s0.T; ++p)
                hipLaunchKernelGGL((if2_sub_step_kernel<MODEL, G, OBS>), grid, dim3(64), lds, st, ag, p);
            fin.s = ag.s;
            fin.m = m;
            launch_if2_finish(fin, n_g, st);
        }
    });
    return hipGetLastError();
}

template <int MODEL, int G>
static hipError_t launch_if2_sub_o(const If2Args& a, int obs, int n_searches, const double* half_widths,
                                   const FilterStreams& fs) {
    return obs == kBinomial ? launch_if2_sub_t<MODEL, G, kBinomial>(a, n_searches, half_widths, fs)
                            : launch_if2_sub_t<MODEL, G, kNormal>(a, n_searches, half_widths, fs);
}

template <int MODEL>
static hipError_t launch_if2_sub_g(const If2Args& a, int G, int obs, int n_searches, const double* half_widths,
                                   const FilterStreams& fs) {
    switch (G) {
        case 2: return launch_if2_sub_o<MODEL, 2>(a, obs, n_searches, half_widths, fs);
        case 3: return launch_if2_sub_o<MODEL, 3>(a, obs, n_searches, half_widths, fs);
        case 4: return launch_if2_sub_o<MODEL, 4>(a, obs, n_searches, half_widths, fs);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_if2_sub(const If2Args& a, int model, int G, int obs, int n_searches, const double* half_widths,
                          const FilterStreams& fs) {
    if (a.s.wg != 64 || a.s.lanes != 1 || a.M < 1 || a.d != G * G + 1 || a.d > kLaneTheta) return hipErrorInvalidValue;
    if (model == kSubgroups) return launch_if2_sub_g<kSubgroups>(a, G, obs, n_searches, half_widths, fs);
    if (model == kSubgroups2) return launch_if2_sub_g<kSubgroups2>(a, G, obs, n_searches, half_widths, fs);
    return hipErrorInvalidValue;
}

}  // namespace epipf
