// isa_forms.hip -- issue cost of the instruction forms the one-lane SIR event loop's rewrite rests on,
// in SIMD-cycles per wave64 instruction, beside profiles/r1_isa_throughput.txt (whose probe timed none of them):
//   v_cmp_lt_f32 into an SGPR pair, v_cndmask_b32 on an SGPR-pair mask, v_bfi_b32, v_pk_add_f32, v_fma_f32 with an
//   SGPR operand; and as yardsticks the r1 table's own v_xor_b32, v_fma_f32 (VGPR operands) and v_mad_u64_u32.
// Each kernel issues 32 instructions of one form per loop iteration (8 independent chains, four times), 8 waves per
// SIMD (2,048 blocks of 256 threads), so the figure is the form's issue cost, not its latency.  The shader clock is read in
// the kernel: clock64() (core clock) over wall_clock64() (100 MHz) across the loop of one wave.
// One line per form: us/launch, clock, cycles per wave instruction per SIMD.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o scripts/bin/isa_forms scripts/isa_forms.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

typedef float float2v __attribute__((ext_vector_type(2)));

enum Form { kXor, kFma, kMad64, kCmpF32, kCndmask, kBfi, kPkAdd, kFmaSgpr, kForms };
static const char* kNames[kForms] = {"k_xor", "k_fma_f32", "k_mad_u64", "k_cmp_f32_sgpr", "k_cndmask_sgpr", "k_bfi",
                                     "k_pk_add_f32", "k_fma_f32_sgpr"};

// 8 independent instructions of form F on the accumulators v[0..7]
template <int F>
__device__ __forceinline__ void eight(uint32_t (&v)[8], float (&f)[8], float2v (&p)[8], unsigned long long (&m)[8],
                                      unsigned long long (&w)[8], uint32_t a, float fa, float sa, float2v pa,
                                      unsigned long long mask) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if constexpr (F == kXor) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(v[i]) : "v"(a));
        else if constexpr (F == kFma) asm volatile("v_fma_f32 %0, %0, %1, %0" : "+v"(f[i]) : "v"(fa));
        else if constexpr (F == kMad64) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(w[i]) : "v"(a), "v"(v[i]) : "vcc");
        else if constexpr (F == kCmpF32) asm volatile("v_cmp_lt_f32_e64 %0, %1, %2" : "+s"(m[i]) : "v"(f[i]), "v"(fa));
        else if constexpr (F == kCndmask) asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(v[i]) : "v"(a), "s"(mask));
        else if constexpr (F == kBfi) asm volatile("v_bfi_b32 %0, %1, %0, %0" : "+v"(v[i]) : "v"(a));
        else if constexpr (F == kPkAdd) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(p[i]) : "v"(pa));
        else if constexpr (F == kFmaSgpr) asm volatile("v_fma_f32 %0, %0, %1, %0" : "+v"(f[i]) : "s"(sa));
    }
}

template <int F>
__global__ __launch_bounds__(256) void form_kernel(int iters, uint32_t a, float fa, float sa, unsigned long long mask,
                                                   uint32_t* out, unsigned long long* clocks) {
    uint32_t v[8];
    float f[8];
    float2v p[8];
    unsigned long long m[8], w[8];
    for (int i = 0; i < 8; ++i) {
        v[i] = threadIdx.x + i;
        f[i] = 0.5f + 0.001f * (float)(threadIdx.x + i);
        p[i] = float2v{f[i], f[i]};
        m[i] = 0;
        w[i] = threadIdx.x * 3u + i;
    }
    const float2v pa{fa, sa};
    const unsigned long long c0 = clock64(), w0 = wall_clock64();
    for (int k = 0; k < iters; ++k) {
        eight<F>(v, f, p, m, w, a, fa, sa, pa, mask);
        eight<F>(v, f, p, m, w, a, fa, sa, pa, mask);
        eight<F>(v, f, p, m, w, a, fa, sa, pa, mask);
        eight<F>(v, f, p, m, w, a, fa, sa, pa, mask);
    }
    const unsigned long long c1 = clock64(), w1 = wall_clock64();
    uint32_t acc = 0;
    for (int i = 0; i < 8; ++i)
        acc ^= v[i] ^ __float_as_uint(f[i]) ^ __float_as_uint(p[i].x) ^ __float_as_uint(p[i].y) ^ (uint32_t)m[i] ^
               (uint32_t)(m[i] >> 32) ^ (uint32_t)w[i] ^ (uint32_t)(w[i] >> 32);
    out[blockIdx.x * 256u + threadIdx.x] = acc;
    if (blockIdx.x == 0 && threadIdx.x == 0) { clocks[0] = c1 - c0; clocks[1] = w1 - w0; }
}

template <int F>
static void run(int blocks, int iters, uint32_t* d_out, unsigned long long* d_clk) {
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    form_kernel<F><<<blocks, 256>>>(iters, 0x9E3779B9u, 0.999f, 1.001f, 0x5555555555555555ull, d_out, d_clk);   // warm-up
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    unsigned long long clk[2] = {0, 1};
    for (int r = 0; r < 3; ++r) {
        CHECK(hipEventRecord(a));
        form_kernel<F><<<blocks, 256>>>(iters, 0x9E3779B9u, 0.999f, 1.001f, 0x5555555555555555ull, d_out, d_clk);
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (ms < best) {
            best = ms;
            CHECK(hipMemcpy(clk, d_clk, sizeof(clk), hipMemcpyDeviceToHost));
        }
    }
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const double simds = 4.0 * prop.multiProcessorCount;
    const double ghz = (double)clk[0] / ((double)clk[1] / 0.1);                   // wall_clock64: 100 MHz
    const double wave_insts = (double)blocks * 4.0 * (double)iters * 32.0;        // 4 waves per block
    const double cyc = (double)best * 1e-3 * ghz * 1e9 * simds / wave_insts;
    const double wave0 = (double)clk[0] / ((double)iters * 32.0);                 // one wave's own cycles per instruction
    printf("%-16s ILP=8 blocks=%5d %10.3f us/launch  clk %.2f GHz  %6.2f cyc/wave-inst/SIMD  (wave0: %6.2f cyc/inst)\n",
           kNames[F], blocks, best * 1e3, ghz, cyc, wave0);
    fflush(stdout);
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
}

int main(int argc, char** argv) {
    const int blocks = argc > 1 ? atoi(argv[1]) : 2048;
    const int iters = argc > 2 ? atoi(argv[2]) : 1024;
    if (blocks < 1 || blocks > 65536 || iters < 1 || iters > (1 << 20)) { fprintf(stderr, "bad arguments\n"); return 2; }
    uint32_t* d_out;
    unsigned long long* d_clk;
    CHECK(hipMalloc(&d_out, (size_t)blocks * 256 * sizeof(uint32_t)));
    CHECK(hipMalloc(&d_clk, 2 * sizeof(unsigned long long)));
    run<kXor>(blocks, iters, d_out, d_clk);
    run<kFma>(blocks, iters, d_out, d_clk);
    run<kMad64>(blocks, iters, d_out, d_clk);
    run<kCmpF32>(blocks, iters, d_out, d_clk);
    run<kCndmask>(blocks, iters, d_out, d_clk);
    run<kBfi>(blocks, iters, d_out, d_clk);
    run<kPkAdd>(blocks, iters, d_out, d_clk);
    run<kFmaSgpr>(blocks, iters, d_out, d_clk);
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_clk));
    return 0;
}
