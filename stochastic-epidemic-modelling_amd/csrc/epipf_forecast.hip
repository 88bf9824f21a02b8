// epipf_forecast.hip -- forecast_kernel (epipf_forecast.hpp) for SIR, SEIR and the subgroup models up to G = 4, and
// the dispatch over model and G (as launch_simulate_path).
#include "epipf_forecast.hpp"

namespace epipf {

// dynamic LDS the launch may take for the block sums (the log table is static LDS beside it)
constexpr size_t kForecastLdsSums = 32 * 1024;

bool forecast_lds_sums(int H, int C) { return sizeof(unsigned long long) * (size_t)H * C <= kForecastLdsSums; }

// The kernel's lane-minor rows [HC][n] -> the caller's layout [n][HC] (HC = H C cells per trajectory), 64 x 64 tiles
// through LDS so that both the loads and the stores of a wave are contiguous.
__global__ __launch_bounds__(256) void forecast_transpose_kernel(const int32_t* __restrict__ in,
                                                                 int32_t* __restrict__ out, int n, int HC) {
    __shared__ int32_t tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const size_t j0 = (size_t)blockIdx.x * 64, c0 = (size_t)blockIdx.y * 64;   // 64-bit: n may be close to 2^31
    for (int i = ty; i < 64; i += 4)
        if (c0 + i < (size_t)HC && j0 + tx < (size_t)n) tile[i][tx] = in[(c0 + i) * n + (j0 + tx)];
    __syncthreads();
    for (int i = ty; i < 64; i += 4)
        if (j0 + i < (size_t)n && c0 + tx < (size_t)HC) out[(j0 + i) * HC + (c0 + tx)] = tile[tx][i];
}

hipError_t launch_forecast_transpose(const int32_t* in, int32_t* out, int n, int HC, hipStream_t s) {
    // grid extents: y, and 256 x blocks in 32 bits along x
    if ((HC + 63) / 64 > 65535 || (size_t)n >= ((size_t)1 << 30)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((size_t)n + 63) / 64), (unsigned)((HC + 63) / 64));
    hipLaunchKernelGGL(forecast_transpose_kernel, grid, dim3(256), 0, s, in, out, n, HC);
    return hipGetLastError();
}

// the SSA of both subgroup models is the same (they differ in what is observed)
hipError_t launch_forecast(const ForecastArgs& a, int model, int G, hipStream_t s) {
    switch (model) {
        case kSIR: forecast_t<kSIR, 1>(a, s); break;
        case kSEIR: forecast_t<kSEIR, 1>(a, s); break;
        default:
            switch (G) {
                case 1: forecast_t<kSubgroups, 1>(a, s); break;
                case 2: forecast_t<kSubgroups, 2>(a, s); break;
                case 3: forecast_t<kSubgroups, 3>(a, s); break;
                case 4: forecast_t<kSubgroups, 4>(a, s); break;
                default: return launch_forecast_wide(a, G, s);
            }
    }
    return hipGetLastError();
}

}  // namespace epipf
