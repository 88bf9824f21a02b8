// epipf_step.hpp -- what the filter kernels share: the grid mapping (step_block), the initial state (init_particle),
// the block-sum prefix scans, also used by the lane-group step kernel (epipf_group.hip), and the phases of a
// one-lane-per-particle step and init kernel (step_half .. init_weights), which the plain filter
// (epipf_kernels.hpp), IF2 (epipf_if2.hip, epipf_if2_sub.hip), the random-walk filter (epipf_walk.hip) and the
// incidence filter (epipf_incidence.hip) call around their own middle.
#pragma once
#include "epipf_device.hpp"
#include "epipf_internal.hpp"

namespace epipf {

// (chain, particle block) of this workgroup.  2-D grid: (blockIdx.y, blockIdx.x).  XCD-aware 1-D grid of B x chains
// (a.xcd_map): the dispatcher deals workgroups round-robin over the 8 XCDs (MI355X_MICROARCH.md, observed; which XCD
// gets block 0 is not fixed), so the blocks p = l (mod 8) share one XCD and its L2.  Label l takes a contiguous range
// of the chain-major block order -- whole chains when B x chains is a multiple of 8 chains' blocks -- so a chain's
// blocks fetch its block sums, in-block prefixes and parent states (the previous step's) into one L2 instead of
// eight, and find them already there when consecutive launches deal the label to the same XCD.  A bijection for any
// grid size (label l holds q + [l < r] blocks), so placement only changes speed.
struct BlockPos {
    int chain, b;
};
__device__ __forceinline__ BlockPos step_block(const StepArgs& a) {
    if (!a.xcd_map) return {a.chain0 + (int)blockIdx.y, (int)blockIdx.x};
    const int total = (int)gridDim.x, p = (int)blockIdx.x;
    const int q = total >> 3, r = total & 7, l = p & 7;
    const int L = l * q + min(l, r) + (p >> 3);
    const int c = L / a.B;
    return {a.chain0 + c, L - c * a.B};
}

// Initial state of particle j (pmcmc.py:156-175): per group an initial infected count Poisson(mu) by CDF inversion on
// the keyed stream (counter (g, j, 2 << 24, f)), S = population - I, the rest 0.  pf_init_kernel and the one-workgroup
// filter (epipf_fused.hpp) draw it with this code.
template <int MODEL, int G>
__device__ __forceinline__ void init_particle(const StepArgs& a, const ChainParam& cp, int j, double* x) {
    constexpr int C = Shape<MODEL, G>::C;
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
#pragma unroll
    for (int g = 0; g < ((MODEL >= kSubgroups) ? G : 1); ++g) {
        const Block r = philox((uint32_t)g, (uint32_t)j, kDomainInit, cp.f, cp.k0, cp.k1);
        const double U = u01(r.x, r.y);
        const double mu = a.mu[g];
        double pk = a.emu[g], F = pk;
        int k = 0;
        while (U >= F && k < a.kmax[g]) { k += 1; pk = pk * mu / (double)k; F = F + pk; }
        const double S0 = a.npop[g] - (double)k;
        if constexpr (MODEL == kSIR) { x[0] = S0; x[1] = (double)k; }
        else if constexpr (MODEL == kSEIR) { x[0] = S0; x[2] = (double)k; }
        else { x[3 * g] = S0; x[3 * g + 1] = (double)k; }
    }
}

// The same draw for the subgroup models at G > kMaxLaneG: groups 0..3 from the kernel arguments, groups 4..7 from the
// chain's WideParam block (a function of its own, so that the one above stays the narrower kernels' code as it was).
template <int MODEL, int G>
__device__ __forceinline__ void init_particle_wide(const StepArgs& a, const ChainParam& cp, int j, double* x,
                                                   const WideParam* wp) {
    static_assert(MODEL >= kSubgroups && G > kMaxLaneG && G <= kMaxG, "the wide subgroup models");
#pragma unroll
    for (int c = 0; c < 3 * G; ++c) x[c] = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const Block r = philox((uint32_t)g, (uint32_t)j, kDomainInit, cp.f, cp.k0, cp.k1);
        const double U = u01(r.x, r.y);
        const bool lo = g < kMaxLaneG;
        const int h = lo ? 0 : g - kMaxLaneG, gl = lo ? g : 0;
        const double mu = lo ? a.mu[gl] : wp->mu_hi[h];
        double pk = lo ? a.emu[gl] : wp->emu_hi[h], F = pk;
        const int kmax = lo ? a.kmax[gl] : wp->kmax_hi[h];
        int k = 0;
        while (U >= F && k < kmax) { k += 1; pk = pk * mu / (double)k; F = F + pk; }
        x[3 * g] = (lo ? a.npop[gl] : wp->npop_hi[h]) - (double)k;
        x[3 * g + 1] = (double)k;
    }
}

// LDS ordering between the lanes that run a helper: the whole block (__syncthreads), or only the calling wave
// (WAVE = true: the lane-group kernel runs these on its first wave while the other waves wait at a block barrier).
template <bool WAVE>
__device__ __forceinline__ void lds_sync() {
    if constexpr (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// exclusive prefix of the B block sums into LDS (bpex), deterministic order; returns the total.
template <int WG, bool WAVE = false>
__device__ __forceinline__ double scan_block_sums(const double* __restrict__ bsum_g, int B, double* bpex,
                                                  double* bsum, double* red) {
    const int tid = threadIdx.x;
    const int per = (B + WG - 1) / WG;
    const int beg = min(tid * per, B), end = min(beg + per, B);
    double s = 0.0;
    for (int i = beg; i < end; ++i) {
        const double v = bsum_g[i];
        bsum[i] = v;
        s = s + v;
    }
    const double incl = block_inclusive_scan<WG>(s, red);
    // exclusive offset of this thread's chunk = inclusive result of the previous thread
    double* incl_lds = bpex + B;  // scratch after bpex (allocated B + WG)
    incl_lds[tid] = incl;
    lds_sync<WAVE>();
    double e = (tid == 0) ? 0.0 : incl_lds[tid - 1];
    for (int i = beg; i < end; ++i) {
        bpex[i] = e;
        e = e + bsum[i];
    }
    lds_sync<WAVE>();
    return bpex[B - 1] + bsum[B - 1];
}

// Segmented prefix of the B block sums (64-thread block): lane l sums the blocks of segments [l*q, (l+1)*q)
// sequentially, a wave scan gives each lane its offset, and the lane writes seg_start[k] / seg_end[k] (the running
// sum before / after segment k's S blocks) to LDS.  With S = 1 this is scan_block_sums<64> exactly (seg_start =
// bpex, seg_end = bpex + bsum).  LDS holds 2 * nseg <= 400 doubles whatever N is, so one-wave blocks keep 7 waves
// per SIMD at every size (before, past ~16k particles the 2B-double table capped occupancy and 256-thread blocks
// were needed, whose four waves retire together).
template <bool WAVE = false>
__device__ __forceinline__ double scan_segments(const double* __restrict__ bsum_g, int B, int S, int nseg,
                                                double* seg_start, double* seg_end) {
    const int lane = threadIdx.x;
    const int q = (nseg + 63) / 64;
    const int k0 = min(lane * q, nseg), k1 = min(k0 + q, nseg);
    const int b0 = min(k0 * S, B), b1 = min(k1 * S, B);
    double s = 0.0;
    for (int i = b0; i < b1; ++i) s = s + bsum_g[i];
    const double inc = block_inclusive_scan<64>(s, nullptr);
    const double up = __shfl_up(inc, 1, 64);
    double e = (lane == 0) ? 0.0 : up;
    for (int k = k0; k < k1; ++k) {
        seg_start[k] = e;
        const int ie = min((k + 1) * S, B);
        for (int i = k * S; i < ie; ++i) e = e + bsum_g[i];
        seg_end[k] = e;
    }
    lds_sync<WAVE>();
    return seg_end[nseg - 1];
}

// The block-sum prefix of a run on 16-particle blocks (lane-group runs, kGroupBlock), with the step's TOTAL summed in
// the 64-particle layout's order, so that a filter's log-likelihood does not depend on which layout its launch used
// (the layout follows the number of chains sharing the launch, pick_block).  The 64-layout total is
//   c_m = the in-block scan's last lane over 64-block m = (s_4m + s_4m+1) + (s_4m+2 + s_4m+3)
// exactly: block_inclusive_scan's Hillis-Steele window at lane 63 is the balanced tree of its four aligned 16-lane
// windows, each the 16-particle block's own scan result s (lane 15, the lanes past the block adding nothing), and
// IEEE addition commutes; then lane l adds the c_m of its P consecutive 64-blocks in order (P = a.canon_per: the
// 64-layout's per-lane share, scan_block_sums / scan_segments), a wave scan gives each lane its offset, and the total is
// the last lane's running sum.  Blocks past N hold weights 0 in both layouts (sums exact).
// Outputs for the 16-particle search: flat (S16 = 1) every block's exclusive prefix and sum (bpex, bsum); segmented
// (S16 = 4 S64, whole 64-blocks per segment) seg_start / seg_end.  Inside a 64-block the 16-block prefixes are
// e, e + s0, e + (s0 + s1), e + ((s0 + s1) + s2): other roundings of the same prefixes, within the resampling
// certificate's depth bound (cert_k is taken on the 16-block layout's larger D), so the search stays certified.
// The total goes through LDS (*tot, written by the lane holding the last 64-block).
template <bool WAVE>
__device__ __forceinline__ double scan_block_sums16(const double* __restrict__ bsum_g, int B16, int P, int S16,
                                                    double* bpex, double* bsum, double* seg_start, double* seg_end,
                                                    double* tot) {
    const int lane = threadIdx.x & 63;
    const int B64 = (B16 + 3) >> 2;
    const int m0 = min(lane * P, B64), m1 = min(m0 + P, B64);
    auto sub = [&](int i) __attribute__((always_inline)) { return i < B16 ? bsum_g[i] : 0.0; };
    double s = 0.0;
    for (int m = m0; m < m1; ++m) {
        const double s0 = sub(4 * m), s1 = sub(4 * m + 1), s2 = sub(4 * m + 2), s3 = sub(4 * m + 3);
        s = s + ((s0 + s1) + (s2 + s3));
    }
    const double inc = block_inclusive_scan<64>(s, nullptr);
    const double up = __shfl_up(inc, 1, 64);
    double e = (lane == 0) ? 0.0 : up;
    for (int m = m0; m < m1; ++m) {
        const int i = 4 * m;
        const double s0 = sub(i), s1 = sub(i + 1), s2 = sub(i + 2), s3 = sub(i + 3);
        const double s01 = s0 + s1;
        if (S16 == 1) {
            bpex[i] = e;
            bsum[i] = s0;
            if (i + 1 < B16) { bpex[i + 1] = e + s0; bsum[i + 1] = s1; }
            if (i + 2 < B16) { bpex[i + 2] = e + s01; bsum[i + 2] = s2; }
            if (i + 3 < B16) { bpex[i + 3] = e + (s01 + s2); bsum[i + 3] = s3; }
        } else if (i % S16 == 0) {
            seg_start[i / S16] = e;
        }
        e = e + (s01 + (s2 + s3));
        if (S16 > 1 && ((i + 4) % S16 == 0 || m == B64 - 1)) seg_end[i / S16] = e;
        if (m == B64 - 1) *tot = e;
    }
    lds_sync<WAVE>();
    return *tot;
}

// ------------------------------------------------------------------ the phases of a one-lane-per-particle step
// One lane per particle, one wave per block (64 threads), the weight layout of 64-particle blocks: the plain filter
// (pf_step_kernel), IF2 (epipf_if2.hip, epipf_if2_sub.hip), the random-walk filter (epipf_walk.hip) and the incidence
// filter (epipf_incidence.hip) run these phases around their own middle.  Every helper takes the
// kernel's dynamic LDS (step_lds_bytes) and carves it up itself,
//   LogTab tab[kLogTabEntries] | double red[16] | S = 1: bsum [B], bpex [B + 64]; else seg_start [nseg], seg_end [nseg]
// because pointers handed on in a struct lose the LDS address space (generic loads in place of ds_read).
__device__ __forceinline__ LogTab* step_logtab(double* smem) { return reinterpret_cast<LogTab*>(smem); }
__device__ __forceinline__ double* step_red(double* smem) { return smem + 2 * kLogTabEntries; }
__device__ __forceinline__ double* step_prefix(double* smem) { return smem + 2 * kLogTabEntries + 16; }

// Offset of a chain's slice in the half of step q of a double buffer with `stride` elements per chain: step p reads
// what step p - 1 wrote (q = p - 1: wraw, wloc and bsum) and writes the half of q = p.  A function of scalars, not a
// struct of the four offsets: the struct costs step kernel instances scalar spills.
__device__ __forceinline__ size_t step_half(const StepArgs& a, int chain, int q, size_t stride) {
    return ((size_t)(q & 1) * a.max_chains + chain) * stride;
}

// (b) likelihood: zetas[p] = zetas[p-1] * mean(w) (pmcmc.py:183), kept in log space.  step_total: the prefix of the
// previous step's block sums into LDS -- S = 1 (B <= kMaxSegments): the block sums and their exclusive prefix; else the
// segment ends only -- and their total.  A kernel then branches on the total itself,
//     if (!(total > 0.0)) { step_degenerate(a, bp, p); return; }
//     step_log_zeta(a, bp, p, total);
// all weights 0 or NaN (numpy raises ValueError -> (None, None, None), :187-192): the chain ends here, degenerate, and
// the block returns; else log_zeta[p].  The branch stays in the kernel and the helpers take and return values only
// (an exit inside a helper, or an output reference, costs the kernels scalar spills).
// pf_step_kernel (epipf_kernels.hpp) carries a copy of this body inline: a change to the segment layout goes in both.
__device__ __forceinline__ double step_total(const StepArgs& a, double* smem, size_t bprev) {
    double* red = step_red(smem);
    double* seg_start = step_prefix(smem);
    double* seg_end = seg_start + a.nseg;
    const double total = (a.seg == 1) ? scan_block_sums<64>(a.bsum + bprev, a.B, seg_start + a.B, seg_start, red)
                                      : scan_segments(a.bsum + bprev, a.B, a.seg, a.nseg, seg_start, seg_end);
    return total;
}
__device__ __forceinline__ void step_degenerate(const StepArgs& a, const BlockPos& bp, int p) {
    if (bp.b == 0 && threadIdx.x == 0) {
        a.status[bp.chain] = kStatusDegenerate;
        a.log_zeta[(size_t)bp.chain * a.T + p] = -__builtin_inf();
    }
}
__device__ __forceinline__ void step_log_zeta(const StepArgs& a, const BlockPos& bp, int p, double total) {
    if (bp.b == 0 && threadIdx.x == 0)
        a.log_zeta[(size_t)bp.chain * a.T + p] = a.log_zeta[(size_t)bp.chain * a.T + p - 1] + log(total / (double)a.N);
}

// (d) particle j's ancestor: the multinomial draw on (0, j, p | resample, f), the certified two-level search of the
// prefix step_total left in LDS, and for the draws it could not certify the exact search by the whole wave, counted in
// slot 1 (pmcmc.py:188-190).  The caller clamps the result (checked_index).  REF, the plain filter alone: the
// systematic draw (a.resample_mode), and with a.ref_k > 0 the reference-ambiguous draws counted in slot 6 (rare: ~1e-8
// of draws at config 2; every uncertified one included).  Without REF neither costs a branch or a register.
template <bool REF>
__device__ __forceinline__ int step_ancestor(const StepArgs& a, double* smem, const ChainParam& cp, int p, int j,
                                             double total, size_t wprev, size_t bprev) {
    double* seg_start = step_prefix(smem);
    double U = 0.0;
    int anc = 0;
    bool certified = true, ambiguous = false;
    if (j < a.N) {
        const uint32_t rtag = ((uint32_t)p & 0xFFFFFFu) | kDomainResample;
        if (!REF || a.resample_mode == 0) {
            const Block r = philox(0u, (uint32_t)j, rtag, cp.f, cp.k0, cp.k1);
            U = u01(r.x, r.y);
        } else {
            const Block r = philox(0u, 0u, rtag, cp.f, cp.k0, cp.k1);
            U = ((double)j + u01(r.x, r.y)) / (double)a.N;
        }
        const double ref_k = REF ? a.ref_k : 0.0;
        if (a.seg == 1)
            anc = resample_search<64>(U, seg_start + a.B, seg_start, a.B, total, a.wloc + wprev, a.N, a.cert_k,
                                      certified, ref_k, ambiguous);
        else
            anc = resample_search_seg(U, seg_start, seg_start + a.nseg, a.nseg, a.seg, a.bsum + bprev, a.B, total,
                                      a.wloc + wprev, 64, a.N, a.cert_k, certified, ref_k, ambiguous);
    }
    if constexpr (REF) {
        if (ambiguous) atomicAdd(counter_slot(a.counters) + 6, 1ull);
    }
    if (__any(!certified)) {   // wave-uniform: the whole wave resolves its uncertified draws exactly
        const int e = resample_exact_wave(!certified, U, a.wraw + wprev, a.N);
        if (!certified) {
            anc = e;
            atomicAdd(counter_slot(a.counters) + 1, 1ull);
        }
    }
    return anc;
}

// The event counters of a wave (a.count_events: EPIPF_PROFILE_COUNTERS): accepted events, lane-iterations,
// wave-iterations x 64 (lane utilisation), and from `exact` -- the lane left the certified f32 loop for the exact SSA
// loop; false in lanes past N -- the particle-steps on the exact loop and the waves with at least one.
__device__ __forceinline__ void step_count(const StepArgs& a, int nev, int iters, bool exact) {
    if (!a.count_events) return;
    unsigned long long e = (unsigned long long)nev, li = (unsigned long long)iters;
    int wmax = iters;
    for (int o = 32; o > 0; o >>= 1) {
        e += __shfl_xor(e, o, 64);
        li += __shfl_xor(li, o, 64);
        wmax = max(wmax, __shfl_xor(wmax, o, 64));
    }
    const unsigned long long ex = __ballot(exact);
    if (threadIdx.x == 0) {
        unsigned long long* slot = counter_slot(a.counters);
        atomicAdd(slot, e);
        atomicAdd(slot + 2, li);
        atomicAdd(slot + 3, 64ull * (unsigned long long)wmax);
        atomicAdd(slot + 4, (unsigned long long)__popcll(ex));
        atomicAdd(slot + 5, ex ? 1ull : 0ull);
    }
}

// The weights step p + 1 reads: w (0 in lanes past N), the block's inclusive prefix and its sum, in the weight
// layout's own padding (B x 64 slots), so every lane stores.  The last step is followed by none and stores nothing.
__device__ __forceinline__ void step_store_weights(const StepArgs& a, double* smem, int b, int j, int p, double w,
                                                   size_t wcur, size_t bcur) {
    if (p + 1 >= a.T) return;
    const double loc = block_inclusive_scan<64>(w, step_red(smem));
    a.wraw[wcur + j] = w;
    a.wloc[wcur + j] = loc;
    if (threadIdx.x == 63) a.bsum[bcur + b] = loc;
}

// The two shared ends of an init kernel.  init_state: particle j's state x into row 0 of the history and its ancestor
// 0.  init_weights: log_zeta[0] = 0, and with a step to follow (T > 1; the incidence filter's T >= 3 always) the weights
// of row 0 into half 0 of the weight buffers with the block's scan.  weight() is the kernel's own, called in the lanes
// that hold a particle (`live`; the others weigh 0) after the state is stored: the binomial weight's tie path reads the
// row back.  smem: the kernel's dynamic LDS, as in the step helpers; an init kernel scans in its first doubles.
// `mine`: the lane holds a slot of the weight layout, `last`: the lane of the block's last slot (blocks of fewer than
// WG particles in the lane-group runs' layout: the lanes past a.wg store nothing).
template <int C>
__device__ __forceinline__ void init_state(const StepArgs& a, int chain, int j, const double* x) {
    int32_t* h = a.hidden + (size_t)chain * a.hist_stride + (size_t)j * C;
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = (int32_t)x[c];
    a.ancestry[(size_t)chain * a.anc_stride + j] = 0;
}
template <int WG, class Weight>
__device__ __forceinline__ void init_weights(const StepArgs& a, double* smem, const BlockPos& bp, int j, bool live,
                                             bool mine, int last, Weight weight) {
    if (bp.b == 0 && threadIdx.x == 0) a.log_zeta[(size_t)bp.chain * a.T] = 0.0;
    if (a.T > 1) {
        double w = 0.0;
        if (live) w = weight();
        const size_t wbase = (size_t)bp.chain * a.wstride;            // buffer 0
        const double loc = block_inclusive_scan<WG>(w, smem);
        if (mine) {
            a.wraw[wbase + j] = w;
            a.wloc[wbase + j] = loc;
        }
        if ((int)threadIdx.x == last) a.bsum[(size_t)bp.chain * a.bstride + bp.b] = loc;
    }
}

}  // namespace epipf
