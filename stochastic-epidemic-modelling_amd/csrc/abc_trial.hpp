// abc_trial.hpp -- one ABC trial on one lane (abc_algo.py:33-88), shared by the rejection sampler's
// abc_trials_kernel (abc_kernels.hip) and the ABC-SMC trial kernel (abc_smc_kernels.hip).
//
// The day table needs no event history: day d holds the state after every event with time <= d (ceil(time)
// groups events into day rows, missing days repeat the previous row), so a lane writes day rows as its clock
// passes integer days.  An event past day T-1 only changes row T, which :88 truncates away: the walk stops.
#pragma once
#include "abc_device.hpp"
#include "epipf_group.hpp"
#include "epipf_internal.hpp"

namespace epipf {

__device__ __forceinline__ void write_day(int32_t* col, size_t n, int d, double S, double I, double R) {
    int32_t* p = col + (size_t)d * 3 * n;
    p[0] = (int32_t)S;
    p[n] = (int32_t)I;
    p[2 * n] = (int32_t)R;
}

// Trial t's initial counts (abc_algo.py:38-39) in x
__device__ __forceinline__ void abc_trial_counts(const AbcArgs& a, uint32_t t, double* x) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                               // :38-39
        const Block r = philox((uint32_t)c, t, kDomainAbcInit, a.f, a.k0, a.k1);
        x[c] = (double)poisson_mode_inversion(a.lam[c], u01(r.x, r.y), a.pm[c]);
    }
}

// Trial t's prior (abc_algo.py:35-36) and initial counts (:38-39): theta in cp, counts in x
__device__ __forceinline__ void abc_trial_start(const AbcArgs& a, uint32_t t, ChainParam& cp, double* x) {
    const Block rp = philox(0u, t, kDomainAbcPrior, a.f, a.k0, a.k1);
    cp.theta[0] = a.prior_lo[0] + a.prior_rng[0] * u01(rp.x, rp.y);             // abc_algo.py:35
    cp.theta[1] = a.prior_lo[1] + a.prior_rng[1] * u01(rp.z, rp.w);             // :36
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                               // :38-39
        const Block r = philox((uint32_t)c, t, kDomainAbcInit, a.f, a.k0, a.k1);
        x[c] = (double)poisson_mode_inversion(a.lam[c], u01(r.x, r.y), a.pm[c]);
    }
}

// The trial's SIR path from x over [0, T-1] (gillespie_algo.py:10-75 with the reference-exact clock), writing each
// day row as the clock passes it: day d holds the state after every event with time <= d.  `write`: this lane
// stores the rows (the lane-group kernel runs it on every lane of a group, one of which writes).  Returns the events;
// x holds the final state, day the first row not yet written, iters the loop iterations.
// Early rejection: `acc` sums |I_d - Y_I,d| + |R_d - Y_R,d| over the rows passed (the distance's terms,
// abc_algo.py:12); once it exceeds `reject_sum` the distance of the full table is provably above the threshold
// (epipf_abc's bound) and the walk stops with `rejected` set -- the rest of the path cannot change the
// trial's fate, and a rejected trial's table is never read.  reject_sum = INFINITY: never.
__device__ __forceinline__ int abc_exact_path(double* x, const ChainParam& cp, uint32_t t, const AbcArgs& a,
                                              const LogTab* __restrict__ tab, int32_t* col, bool write, int& day,
                                              double& next_day, int& iters, double reject_sum, bool& rejected) {
    const size_t n = (size_t)a.n;
    SsaState<kSIR, 1> st;
    st.load(x, cp);
    const double R0 = x[2];
    const double last_day = a.last_day;
    double clock = 0.0;
    uint32_t k = 0;
    int nev = 0;
    bool alive = st.active();
    double acc = 0.0;
    rejected = false;
    Block rn{0u, 0u, 0u, 0u};
    if (alive) rn = philox(0u, t, kDomainAbcSsa, a.f, a.k0, a.k1);
    while (alive) {                          // every lane enters at k = 0: k stays wave-uniform
        const Block r = rn;
        ++k;
        rn = philox(__builtin_amdgcn_readfirstlane(k), t, kDomainAbcSsa, a.f, a.k0, a.k1);
        const double S0 = st.S, I0 = st.I;
        const int rec0 = st.nrec;
        const bool ev = st.template event<true>(r, clock, last_day, cp, tab);   // false: the event lands after day T-1
        if (ev) {
            ++nev;
            while (next_day < clock) {                                   // days the event does not reach
                const double R = R0 + (double)rec0;
                if (write) write_day(col, n, day, S0, I0, R);
                acc += fabs(I0 - a.Y[3 * day + 1]) + fabs(R - a.Y[3 * day + 2]);
                ++day;
                next_day += 1.0;
            }
            rejected = acc > reject_sum;
        }
        alive = ev && st.active() && !rejected;
    }
    st.save(x);
    iters = (int)k;
    return nev;
}

// One lane of the one-lane trial kernels: sorted position g0 + global thread index runs trial perm[g] (or g).
// SMC = false, the rejection sampler: theta from the prior counter, written to the batch's theta columns.
// SMC = true, an ABC-SMC generation: theta was written by abc_smc_propose_kernel, which also marked the proposals
// outside the prior box in row 0's S (the early-rejection marker abc_distance_kernel turns into +inf); a marked
// trial runs nothing.  Everything after the start is the same code.
// (The arguments by value, as the kernel receives them: by reference the rejection sampler's kernel takes one more
// VGPR than its 65.)
template <bool SMC>
__device__ __forceinline__ void abc_trial_lane(const AbcArgs a, const LogTab* tab) {
    const int g = a.g0 + (int)(blockIdx.x * 256 + threadIdx.x);    // sorted position (from g0: the lane groups)
    int nev = 0, iters = 0;
    if (g < a.n) {
        const int i = a.perm ? a.perm[g] : g;
        const uint32_t t = a.t0 + (uint32_t)i;
        const size_t n = (size_t)a.n;
        ChainParam cp;
        double x[3];
        bool run = true;
        if constexpr (SMC) {
            run = a.days[i] >= 0;
            cp.theta[0] = a.theta[i];
            cp.theta[1] = a.theta[n + i];
            if (run) abc_trial_counts(a, t, x);
        } else {
            abc_trial_start(a, t, cp, x);
        }
        if (run) {
            int32_t* col = a.days + i;
            int day = 0;
            double next_day = 0.0;
            bool rejected;
            nev = abc_exact_path(x, cp, t, a, tab, col, true, day, next_day, iters, a.reject_sum, rejected);
            if (rejected) col[0] = -1;                                   // row 0's S: abc_distance_kernel's marker
            else for (; day < a.T; ++day) write_day(col, n, day, x[0], x[1], x[2]);
            if constexpr (!SMC) {
                a.theta[i] = cp.theta[0];
                a.theta[n + i] = cp.theta[1];
            }
        }
    }
    if (a.count) {
        unsigned long long e = (unsigned long long)nev, li = (unsigned long long)iters;
        int wmax = iters;
        for (int o = 32; o > 0; o >>= 1) {
            e += __shfl_xor(e, o, 64);
            li += __shfl_xor(li, o, 64);
            wmax = max(wmax, __shfl_xor(wmax, o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* slot = counter_slot(a.counters);
            atomicAdd(slot, e);
            atomicAdd(slot + 2, li);
            atomicAdd(slot + 3, 64ull * (unsigned long long)wmax);
        }
    }
}

// Predicted event count of a trial with this theta (the length-ordering key): a forward-Euler
// integration of the deterministic SIR from the mean initial counts, dt = 1/4 day, up to day T-1.
__device__ __forceinline__ uint32_t abc_predicted_length(const AbcArgs& a, float beta, float gamma) {
    float S = (float)a.lam[0], I = (float)a.lam[1];
    const float N = (float)(a.lam[0] + a.lam[1] + a.lam[2]);
    const float bN = N > 0.f ? 0.25f * beta / N : 0.f, g4 = 0.25f * gamma;
    float events = 0.f;
    for (int s = 0; s < 4 * (a.T - 1) && I >= 0.5f; ++s) {
        const float inf = fminf(bN * S * I, S), rec = g4 * I;
        S -= inf;
        I += inf - rec;
        events += inf + rec;
    }
    return (uint32_t)fminf(events * 0.25f, 65535.f);
}

}  // namespace epipf
