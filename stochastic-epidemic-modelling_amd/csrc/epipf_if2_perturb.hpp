// epipf_if2_perturb.hpp -- the parameter jitter of iterated filtering, shared by the IF2 kernels
// (epipf_if2.hip) and the random-walk filter's (epipf_walk.hip, §18).  Device code only.
#pragma once
#include "epipf_if2.hpp"
#include "epipf_step.hpp"

namespace epipf {

// theta[c] + hw[c] (2u - 1), reflected at 0; component c draws from block c / 2 of (., j, tag, f): words (0, 1) for
// even c, (2, 3) for odd c.  No contraction (-ffp-contract=off): the restatement's roundings.
template <int D>
__device__ __forceinline__ void if2_perturb_hw(double* th, const double* hw, uint32_t j, uint32_t tag, const ChainParam& cp) {
#pragma unroll
    for (int b = 0; b < (D + 1) / 2; ++b) {
        const Block r = philox((uint32_t)b, j, tag, cp.f, cp.k0, cp.k1);
        {
            const double u = u01(r.x, r.y);
            const double t = th[2 * b] + hw[2 * b] * (2.0 * u - 1.0);
            th[2 * b] = (t < 0.0) ? -t : t;
        }
        if (2 * b + 1 < D) {
            const double u = u01(r.z, r.w);
            const double t = th[2 * b + 1] + hw[2 * b + 1] * (2.0 * u - 1.0);
            th[2 * b + 1] = (t < 0.0) ? -t : t;
        }
    }
}

// The IF2 kernels' form: the half-widths of the running iteration, from the argument block.
template <int D>
__device__ __forceinline__ void if2_perturb(double* th, const If2Args& a, uint32_t j, uint32_t tag, const ChainParam& cp) {
    if2_perturb_hw<D>(th, a.hw, j, tag, cp);
}

}  // namespace epipf
