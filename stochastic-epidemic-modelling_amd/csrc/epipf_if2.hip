// epipf_if2.hip -- the iterated-filtering kernels for MI355X (gfx950) and their launcher.
//
// if2_init_kernel / if2_step_kernel filter with theta per particle: one lane per particle, one wave per block, on the
// shared phases of epipf_step.hpp -- the grid (step_block), the step total and log_zeta (step_total, step_degenerate,
// step_log_zeta), the ancestor (step_ancestor), the event counters (step_count, which epipf_if2 harvests and clears),
// the weight stores (step_store_weights) and the init kernel's ends (init_state, init_weights) -- and the filter's weight
// (particle_weight).  Their own:
//   - the status rule: the first iteration starts every search, a search that degenerated stays as it ended;
//   - the filter index is the chain's plus the iteration (cp.f + m), so the M passes of a call need no upload between;
//   - after the ancestor is known the lane gathers the ancestor's theta, jitters it (perturb) and stores it, and
//     runs the SSA on its own ChainParam copy with that theta (rates in VGPRs instead of SGPRs);
//   - the SSA is the certified f32 loop (fast_propagate) with the exact loop per lane for what it hands back.  The
//     wave-cooperative replay (coop_replay) takes one wave-uniform ChainParam, which a lane's theta is not.
// if2_finish_kernel closes an iteration of the searches still running: the swarm becomes the next iteration's start
// and its component means are reduced in a fixed order.
#include "epipf_if2.hpp"

#include <algorithm>

#include "epipf_if2_perturb.hpp"
#include "epipf_step.hpp"

namespace epipf {

template <int MODEL, int OBS>
__global__ __launch_bounds__(64) void if2_init_kernel(If2Args a) {
    constexpr int C = Shape<MODEL, 1>::C;
    constexpr int D = (MODEL == kSIR) ? 2 : 3;
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
        init_particle<MODEL, 1>(s, cp, j, x);                            // pmcmc.py:156-175
        init_state<C>(s, chain, j, x);
        double th[D];
#pragma unroll
        for (int c = 0; c < D; ++c) th[c] = a.start[((size_t)chain * D + c) * s.N + j];
        if2_perturb<D>(th, a, (uint32_t)j, kDomainIf2, cp);              // step 0
#pragma unroll
        for (int c = 0; c < D; ++c) a.swarm[((size_t)chain * D + c) * s.N + j] = th[c];   // buffer 0
    }
    init_weights<WG>(s, smem, bp, j, j < s.N, true, WG - 1, [&] {
        return particle_weight<MODEL, 1, OBS>(x, s.Y, cp, s.cp + chain, s.lf, s.lf_max,
                                              s.hidden + (size_t)chain * s.hist_stride + (size_t)j * C);
    });
}

template <int MODEL, int OBS>
__global__ __launch_bounds__(64) void if2_step_kernel(If2Args a, int p) {
    constexpr int C = Shape<MODEL, 1>::C;
    constexpr int K = Shape<MODEL, 1>::K;
    constexpr int D = (MODEL == kSIR) ? 2 : 3;
    constexpr int WG = 64;
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
    // in theta and thetaf only.
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
        if2_perturb<D>(th, a, (uint32_t)j, ((uint32_t)p & 0xFFFFFFu) | kDomainIf2, cp);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            a.swarm[(((size_t)cur * s.max_chains + chain) * D + c) * s.N + j] = th[c];
            lcp.theta[c] = th[c];
            lcp.thetaf[c] = (float)th[c];
        }
        const int32_t* hp = s.hidden + (size_t)chain * s.hist_stride + ((size_t)(p - 1) * s.N + anc) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (double)hp[c];
        fast_ok = fast_propagate<MODEL, 1>(x, lcp, (uint32_t)j, ptag, 1.0, nev, iters, eligible);
    }
    // lanes the f32 loop could not run or could not certify at the step boundary: the exact loop from the untouched
    // parent state, per lane.  Its log table goes to LDS only in waves that need it (one wave per block, so the test
    // is block-uniform and the barrier legal).
    if (__any(!fast_ok)) {
        for (int i = tid; i < kLogTabEntries; i += WG) tab[i] = s.logtab[i];
        __syncthreads();
        if (!fast_ok) nev = exact_propagate<MODEL, 1>(x, lcp, (uint32_t)j, ptag, 1.0, tab, iters);
    }
    step_count(s, nev, iters, !fast_ok);                 // lanes past N hold fast_ok = true
    double w = 0.0;
    if (j < s.N) {
        int32_t* hc = s.hidden + (size_t)chain * s.hist_stride + ((size_t)p * s.N + j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) hc[c] = (int32_t)x[c];
        if (p + 1 < s.T) w = particle_weight<MODEL, 1, OBS>(x, s.Y + (size_t)p * K, cp, s.cp + chain, s.lf, s.lf_max, hc);
    }
    step_store_weights(s, smem, bp.b, j, p, w, wcur, bcur);
}

// End of iteration m for the searches still running: block (c, search) copies component c of the final swarm (buffer
// (T - 1) & 1) to the start copy and reduces its mean: each thread's strided partial sum, then the 256 partials in
// thread order by one thread (a fixed order: the same bits on every run).
__global__ __launch_bounds__(256) void if2_finish_kernel(If2Args a) {
    __shared__ double part[256];
    const StepArgs& s = a.s;
    const int c = blockIdx.x, chain = s.chain0 + (int)blockIdx.y;
    if (s.status[chain] != 0) return;
    const int last = (s.T - 1) & 1;
    const double* src = a.swarm + (((size_t)last * s.max_chains + chain) * a.d + c) * s.N;
    double* dst = a.start + ((size_t)chain * a.d + c) * s.N;
    double acc = 0.0;
    for (int i = threadIdx.x; i < s.N; i += 256) {
        const double v = src[i];
        dst[i] = v;
        acc = acc + v;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < 256; ++i) tot = tot + part[i];
        a.mean[((size_t)chain * a.M + a.m) * a.d + c] = tot / (double)s.N;
        if (c == 0) a.done[chain] = a.m + 1;
    }
}

void launch_if2_finish(const If2Args& a, int n_g, hipStream_t st) {
    hipLaunchKernelGGL(if2_finish_kernel, dim3(a.d, n_g), dim3(256), 0, st, a);
}

template <int MODEL, int OBS>
static hipError_t launch_if2_t(const If2Args& a, int n_searches, const double* half_widths, const FilterStreams& fs) {
    const StepArgs& s0 = a.s;
    const size_t lds = step_lds_bytes(s0.B, 64);
    launch_chain_groups(s0, n_searches, fs, 64, [&](int, const StepArgs& sg, int n_g, dim3 grid, hipStream_t st) {
        If2Args ag = a;
        ag.s = sg;
        for (int m = 0; m < a.M; ++m) {
            ag.m = m;
            for (int c = 0; c < a.d; ++c) ag.hw[c] = half_widths[(size_t)m * a.d + c];
            ag.s.log_zeta = s0.log_zeta + (size_t)m * s0.max_chains * s0.T;
            hipLaunchKernelGGL((if2_init_kernel<MODEL, OBS>), grid, dim3(64), lds, st, ag);
            for (int p = 1; p < s0.T; ++p) hipLaunchKernelGGL((if2_step_kernel<MODEL, OBS>), grid, dim3(64), lds, st, ag, p);
            launch_if2_finish(ag, n_g, st);
        }
    });
    return hipGetLastError();
}

hipError_t launch_if2(const If2Args& a, int model, int obs, int n_searches, const double* half_widths,
                      const FilterStreams& fs) {
    if (a.s.wg != 64 || a.s.lanes != 1 || a.M < 1) return hipErrorInvalidValue;
    if (model == kSIR && a.d == 2)
        return obs == kBinomial ? launch_if2_t<kSIR, kBinomial>(a, n_searches, half_widths, fs)
                                : launch_if2_t<kSIR, kNormal>(a, n_searches, half_widths, fs);
    if (model == kSEIR && a.d == 3)
        return obs == kBinomial ? launch_if2_t<kSEIR, kBinomial>(a, n_searches, half_widths, fs)
                                : launch_if2_t<kSEIR, kNormal>(a, n_searches, half_widths, fs);
    return hipErrorInvalidValue;
}

}  // namespace epipf
