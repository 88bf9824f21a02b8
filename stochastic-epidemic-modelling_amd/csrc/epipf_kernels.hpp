// epipf_kernels.hpp -- the one-lane-per-particle kernel templates (init, filter step, simulate, simulate_path) and
// their launch helpers, shared by the translation units that instantiate them: epipf_kernels.hip (SIR, SEIR and the
// subgroup models up to G = 4) and epipf_kernels_wide.hip (the subgroup models at G = 5..8, split off for compile time).
// pf_init_kernel / pf_step_kernel run the shared phases of epipf_step.hpp; their own are the skip
// status, the blocks of fewer than WG particles (lane-group layouts), the systematic draw and the ambiguity count
// (step_ancestor<true>), the chain's wave-uniform rates and the cooperative replay of the lanes the f32 loop hands back.
// pf_step_kernel keeps one shared phase inline, the block-sum scan (step_total's body).
#pragma once
#include "epipf_step.hpp"
#include <algorithm>

#include <cstdio>

#include "epipf_internal.hpp"

#ifndef EPIPF_STEP_WAVES
#define EPIPF_STEP_WAVES 1   // minimum waves per SIMD asked of the step kernel's register allocation
#endif

namespace epipf {

template <int MODEL, int G, int OBS, int WG>
__global__ __launch_bounds__(WG) void pf_init_kernel(StepArgs a) {
    using Sh = Shape<MODEL, G>;
    constexpr int C = Sh::C;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const BlockPos bp = step_block(a);
    const int chain = bp.chain;
    // a.wg particles per block: WG (one lane each), or fewer for the lane-group runs' smaller blocks (the lanes past
    // a.wg hold no particle and weigh 0 in the scan)
    const bool mine = (int)threadIdx.x < a.wg;
    const int j = bp.b * a.wg + (int)threadIdx.x;
    const ChainParam cp = a.cp[chain];
    // the chain's status for this run: skipped or running (the step kernels read it; a degenerate step sets 1)
    if (bp.b == 0 && threadIdx.x == 0) a.status[chain] = cp.skip ? kStatusSkipped : kStatusOk;
    if (cp.skip) return;
    double x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    if (mine && j < a.N) {
        if constexpr (G > kMaxLaneG)                           // pmcmc.py:156-175
            init_particle_wide<MODEL, G>(a, cp, j, x, wide_param(a.cp, a.max_chains, chain));
        else
            init_particle<MODEL, G>(a, cp, j, x);
        init_state<C>(a, chain, j, x);
    }
    init_weights<WG>(a, smem, bp, j, mine && j < a.N, mine, a.wg - 1, [&] {
        return particle_weight<MODEL, G, OBS>(x, a.Y, cp, a.cp + chain, a.lf, a.lf_max,
                                              a.hidden + (size_t)chain * a.hist_stride + (size_t)j * C);
    });
}

template <int MODEL, int G, int OBS, int WG>
__global__ __launch_bounds__(WG, EPIPF_STEP_WAVES) void pf_step_kernel(StepArgs a, int p) {
    using Sh = Shape<MODEL, G>;
    constexpr int C = Sh::C;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    static_assert(WG == 64, "one wave per block (scan_segments)");
    LogTab* tab = step_logtab(smem);
    double* red = step_red(smem);                        // for the block-sum scan below, step_total's body: it stays
    double* seg_start = step_prefix(smem);               // inline in this kernel, with its pointers taken here, because
    double* seg_end = seg_start + a.nseg;                // as a call every instance's generated code moved
    const BlockPos bp = step_block(a);
    const int chain = bp.chain;
    const int tid = threadIdx.x;
    const int j = bp.b * WG + tid;
    if (a.status[chain] != 0) return;
    const ChainParam cp = a.cp[chain];
    const size_t wprev = step_half(a, chain, p - 1, a.wstride), wcur = step_half(a, chain, p, a.wstride);
    const size_t bprev = step_half(a, chain, p - 1, a.bstride), bcur = step_half(a, chain, p, a.bstride);

    // (b) likelihood: zetas[p] = zetas[p-1] * mean(w)  (pmcmc.py:183), kept in log space
    // S = 1 (B <= kMaxSegments): the block sums and their exclusive prefix stay in LDS; else segment ends only
    const double total = (a.seg == 1) ? scan_block_sums<WG>(a.bsum + bprev, a.B, seg_start + a.B, seg_start, red)
                                      : scan_segments(a.bsum + bprev, a.B, a.seg, a.nseg, seg_start, seg_end);
    if (!(total > 0.0)) {  // all weights 0 or NaN: numpy raises ValueError -> (None, None, None), :187-192
        step_degenerate(a, bp, p);
        return;
    }
    step_log_zeta(a, bp, p, total);

    int nev = 0, iters = 0;
    double w = 0.0;
    // (d) the draw (multinomial or systematic), the certified search, the ambiguity count, pmcmc.py:188-190
    int anc = step_ancestor<true>(a, smem, cp, p, j, total, wprev, bprev);
    // (f) gather the parent state, (g) propagate over [0, 1], :195-220: the certified f32 loop, then the exact path
    // for the lanes it hands back.  The exact path's log table is copied to LDS only by waves that need it (~1% at
    // config 2): one wave per block, so the wave-uniform test is block-uniform and the barriers are legal.
    double x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    const uint32_t ptag = ((uint32_t)p & 0xFFFFFFu) | kDomainSSA;
    bool fast_ok = false, eligible = false;
    const WideParam* wp = nullptr;                       // G = 5..8: the chain's block behind the ChainParam array
    if constexpr (G > kMaxLaneG) wp = wide_param(a.cp, a.max_chains, chain);
    if (j < a.N) {
        anc = checked_index(anc, a.N);
        a.ancestry[(size_t)chain * a.anc_stride + (size_t)p * a.N + j] = anc;   // :193
        const int32_t* hp = a.hidden + (size_t)chain * a.hist_stride + ((size_t)(p - 1) * a.N + anc) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (double)hp[c];
        fast_ok = fast_propagate<MODEL, G>(x, cp, (uint32_t)j, ptag, 1.0, nev, iters, eligible, wp);
    }
    const bool exact = j < a.N && !fast_ok;
    if (__any(exact)) {
        for (int i = tid; i < kLogTabEntries; i += WG) tab[i] = a.logtab[i];
        __syncthreads();
        // lanes the f32 loop could not run (population or rates out of its range): the exact loop, per lane
        if (exact && !eligible) {
            int ex_iters = 0;
            nev = exact_propagate<MODEL, G>(x, cp, (uint32_t)j, ptag, 1.0, tab, ex_iters, wp);
            iters += ex_iters;
        }
        // lanes it stopped at the step boundary: replayed one at a time by the whole wave (coop_replay).  The lanes'
        // states wait in their output rows meanwhile (x is not live across the replay: registers, occupancy).
        unsigned long long pend = __ballot(exact && eligible);
        if (pend) {
            int32_t* hrow = a.hidden + (size_t)chain * a.hist_stride + (size_t)p * a.N * C;
            if (j < a.N) {
#pragma unroll
                for (int c = 0; c < C; ++c) hrow[(size_t)j * C + c] = (int32_t)x[c];   // replayed lanes: the parent
            }
            __syncthreads();                                          // one wave per block: orders the rows
            while (pend) {
                const int L = (int)__builtin_ctzll(pend);
                pend &= pend - 1ull;
                const uint32_t jl = __builtin_amdgcn_readlane((uint32_t)j, L);
                const int n = coop_replay<MODEL, G>(hrow + (size_t)jl * C, cp, jl, ptag, 1.0, tab, wp);
                if (tid == L) nev = n;
            }
            __syncthreads();
            if (j < a.N) {
#pragma unroll
                for (int c = 0; c < C; ++c) x[c] = (double)hrow[(size_t)j * C + c];
            }
        }
    }
    if (j < a.N) {
        int32_t* hc = a.hidden + (size_t)chain * a.hist_stride + ((size_t)p * a.N + j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) hc[c] = (int32_t)x[c];                        // :222-231
        // (a) weights of the new state against Y[p], used by step p+1, :178-181
        if (p + 1 < a.T) w = particle_weight<MODEL, G, OBS>(x, a.Y + (size_t)p * Sh::K, cp, a.cp + chain, a.lf, a.lf_max, hc);
    }
    step_count(a, nev, iters, exact);
    step_store_weights(a, smem, bp.b, j, p, w, wcur, bcur);
}

template <int MODEL, int G>
__global__ __launch_bounds__(256) void simulate_kernel(SimArgs a) {
    constexpr int C = Shape<MODEL, G>::C;
    __shared__ LogTab tab[kLogTabEntries];
    if (threadIdx.x < kLogTabEntries) tab[threadIdx.x] = a.logtab[threadIdx.x];
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    int nev = 0, iters = 0;
    if (j < a.n) {
        double x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (double)a.in[(size_t)j * C + c];
        int exact = 0;
        const WideParam* wp = nullptr;                   // G = 5..8: the block behind the one ChainParam
        if constexpr (G > kMaxLaneG) wp = wide_param(a.cp, 1, 0);
        nev = ssa_propagate<MODEL, G>(x, *a.cp, (uint32_t)j, (a.step & 0xFFFFFFu) | kDomainSSA, a.tmax, tab, iters, exact, wp);
#pragma unroll
        for (int c = 0; c < C; ++c) a.out[(size_t)j * C + c] = (int32_t)x[c];
    }
    unsigned long long e = (unsigned long long)nev;
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(a.events, e);
}

// Full-path SSA (gillespie_algo.py *_simulate with last_values_only=False): the exact event loop -- whose clock is
// the reference's bit for bit (SsaState) -- storing every event's time and state (:68-70).  Same draws and same
// final state as simulate_kernel.  Lanes of a wave step together (the event index is wave-uniform), so event k's
// stores of the wave land in contiguous [k][...][lane] rows.
template <int MODEL, int G>
__global__ __launch_bounds__(256) void simulate_path_kernel(SimPathArgs a) {
    constexpr int C = Shape<MODEL, G>::C;
    __shared__ LogTab tab[kLogTabEntries];
    if (threadIdx.x < kLogTabEntries) tab[threadIdx.x] = a.logtab[threadIdx.x];
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const ChainParam cp = *a.cp;
    const uint32_t ptag = (a.step & 0xFFFFFFu) | kDomainSSA;
    double x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = (double)a.in[(size_t)j * C + c];
    SsaState<MODEL, G> st;
    if constexpr (G > kMaxLaneG) st.bind(wide_param(a.cp, 1, 0));
    st.load(x, cp);
    double t = 0.0;
    uint32_t k = 0;
    int nev = 0;
    bool alive = st.active();
    while (alive) {
        const Block r = philox(__builtin_amdgcn_readfirstlane(k), (uint32_t)j, ptag, cp.f, cp.k0, cp.k1);
        ++k;
        const bool ev = st.event(r, t, a.tmax, cp, tab);
        if (ev) {
            if (nev < a.cap) {
                double xs[C];
                st.save(xs);
                a.times[(size_t)nev * a.n + j] = t;
#pragma unroll
                for (int c = 0; c < C; ++c) a.states[((size_t)nev * C + c) * a.n + j] = (int32_t)xs[c];
            }
            ++nev;
        }
        alive = ev && st.active();
    }
    st.save(x);
#pragma unroll
    for (int c = 0; c < C; ++c) a.final_state[(size_t)j * C + c] = (int32_t)x[c];
    a.nev[j] = nev;
}

template <int MODEL, int G, int OBS, int WG>
static hipError_t launch_filter_t(const StepArgs& a, int n_chains, const FilterStreams& fs) {
    constexpr int C = Shape<MODEL, G>::C;
    const size_t lds = step_lds_bytes(a.B, WG);
    // W lanes per particle (runs too small to fill the chip): the lane-group step kernel, epipf_group.hip
    const GroupStepFn group = a.lanes > 1 ? group_step_launcher(MODEL, G, OBS, a.lanes, a.lane_events) : nullptr;
    if (a.lanes > 1 && !group) return hipErrorInvalidValue;
    const size_t glds = group ? group_lds_bytes(a.B, a.seg, C, a.lanes, a.lane_events, a.wg) : 0;
    // the grid-size test leaves room for the lane-group blocks
    launch_chain_groups(a, n_chains, fs, WG * std::max(1, a.lanes),
                        [&](int g, const StepArgs& ag, int, dim3 grid, hipStream_t s) {
        if (g == 0 && fs.ev_init) (void)hipEventRecord(fs.ev_init, s);
        hipLaunchKernelGGL((pf_init_kernel<MODEL, G, OBS, WG>), grid, dim3(WG), lds, s, ag);
        if (g == 0 && fs.ev_step0) (void)hipEventRecord(fs.ev_step0, s);
        if (fs.g_begin[g]) (void)hipEventRecord(fs.g_begin[g], s);
        for (int p = 1; p < a.T; ++p) {
#ifdef EPIPF_ROCTX
            char msg[48];
            snprintf(msg, sizeof msg, "filter step %d group %d", p, g);
            EPIPF_RANGE_PUSH(msg);
#endif
            if (group) group(ag, p, grid, glds, s);
            else hipLaunchKernelGGL((pf_step_kernel<MODEL, G, OBS, WG>), grid, dim3(WG), lds, s, ag, p);
            EPIPF_RANGE_POP();
        }
        if (fs.g_end[g]) (void)hipEventRecord(fs.g_end[g], s);
    });
    if (fs.ev_end) (void)hipEventRecord(fs.ev_end, fs.s[0]);
    return hipGetLastError();
}

template <int MODEL, int G, int WG>
static hipError_t launch_obs(const StepArgs& a, int obs, int n_chains, const FilterStreams& fs) {
    return obs == kBinomial ? launch_filter_t<MODEL, G, kBinomial, WG>(a, n_chains, fs)
                            : launch_filter_t<MODEL, G, kNormal, WG>(a, n_chains, fs);
}

template <int MODEL, int G>
static void sim_t(const SimArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((simulate_kernel<MODEL, G>), dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

template <int MODEL, int G>
static void sim_path_t(const SimPathArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((simulate_path_kernel<MODEL, G>), dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace epipf
