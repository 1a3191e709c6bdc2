// tools/pair_arith.hip — what one packed f32 pair operation costs on this chip, against its two plain f32 operations.
//
// The streams are the f2 helpers of mtr_core.h themselves (fma2, mul2, add2, rsub2; PK = packed, !PK = plain), unrolled by the compiler:
// no hand-written assembly.  Per helper: `independent` = 8 accumulators updated in turn (nothing waits for the previous instruction),
// `dependent` = one accumulator (each instruction waits for the one before).  One workgroup on one CU, of 4, 8 or 16 waves = 1, 2 or 4
// waves on each of its four SIMDs; every wave stamps its own clock (s_memtime, shader cycles) around the loop.
//
// build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize tools/pair_arith.hip -o tools/pair_arith
//         (-fno-slp-vectorize: otherwise the compiler packs the plain twin again)
// run:    timeout -k 10 120 tools/pair_arith        one short launch per case; prints the table this round's profile file quotes
//
// Columns: cyc/pair = cycles of a wave per pair operation (median over the waves of the workgroup); cyc/instr = the same per VALU
// instruction of the stream (1 per pair when packed, 2 when plain); simd cyc/pair = cycles of one SIMD per pair operation = cyc/pair
// divided by the waves that share it — the price that matters to a kernel bound by VALU issue.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mitransient_amd/csrc/mtr_core.h"

using namespace mtr;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int kMaxThreads = 1024, kUnroll = 8, kIters = 256;
enum Op { FMA_PPP = 0, FMA_PSP, FMA_PSS, MUL_PP, ADD_PP, RSUB_SP, N_OPS };
static const char *kOpName[N_OPS] = { "fma2(f2, f2, f2)", "fma2(f2, float, f2)", "fma2(f2, float, float)", "mul2(f2, f2)", "add2(f2, f2)", "rsub2(float, f2)" };

template <int OP, bool PK>
__device__ __forceinline__ f2 step(f2 a, f2 b, f2 c, float s, float t)
{
    if (OP == FMA_PPP) return fma2<PK>(a, b, c);
    if (OP == FMA_PSP) return fma2<PK>(a, s, c);
    if (OP == FMA_PSS) return fma2<PK>(a, s, t);
    if (OP == MUL_PP) return mul2<PK>(a, b);
    if (OP == ADD_PP) return add2<PK>(a, c);
    return rsub2<PK>(s, a);
}

// in: 8 floats per thread (opaque to the compiler: nothing folds); out: one float per thread; cyc: one stamp difference per wave
template <int OP, bool PK, int CHAINS>
__global__ __launch_bounds__(kMaxThreads) void k_stream(const float *in, float *out, unsigned long long *cyc, int iters)
{
    const float *p = in + 8 * threadIdx.x;
    const f2 b{ p[0], p[1] }, c{ p[2], p[3] };
    const float s = p[4], t = p[5];
    f2 acc[CHAINS];
#pragma unroll
    for (int k = 0; k < CHAINS; ++k) acc[k] = f2{ p[6] + (float)k, p[7] - (float)k };
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
            for (int k = 0; k < CHAINS; ++k) acc[k] = step<OP, PK>(acc[k], b, c, s, t);
        }
    }
    // the stamp after the loop must not be taken before the last result exists: make it depend on the accumulators
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < CHAINS; ++k) sum += acc[k].x + acc[k].y;
    asm volatile("" : "+v"(sum));
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[threadIdx.x] = sum;
    if ((threadIdx.x & 63u) == 0u) cyc[threadIdx.x >> 6] = t1 - t0;
}

struct Bufs { float *in, *out; unsigned long long *cyc; };

template <int OP, bool PK, int CHAINS>
static double run(const Bufs &b, int waves_per_simd)
{
    const int threads = 256 * waves_per_simd, waves = threads / 64;
    CHECK(hipMemset(b.cyc, 0, sizeof(unsigned long long) * (kMaxThreads / 64)));
    hipLaunchKernelGGL((k_stream<OP, PK, CHAINS>), dim3(1), dim3(threads), 0, 0, b.in, b.out, b.cyc, kIters);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned long long> c(waves);
    CHECK(hipMemcpy(c.data(), b.cyc, sizeof(unsigned long long) * waves, hipMemcpyDeviceToHost));
    std::sort(c.begin(), c.end());
    return (double)c[waves / 2] / ((double)kIters * kUnroll * CHAINS);       // cycles of a wave per pair operation
}

template <int OP>
static void report(const Bufs &b)
{
    for (int dep = 0; dep < 2; ++dep)
        for (int w = 1; w <= 4; w *= 2) {
            const double pk = dep ? run<OP, true, 1>(b, w) : run<OP, true, 8>(b, w);
            const double sc = dep ? run<OP, false, 1>(b, w) : run<OP, false, 8>(b, w);
            printf("%-24s %-11s %d  | packed %7.2f %7.2f %7.2f | plain %7.2f %7.2f %7.2f | packed / plain pair %5.2f   one v_pk = %4.2f plain instr\n",
                   kOpName[OP], dep ? "dependent" : "independent", w, pk, pk, pk / w, sc, sc / 2.0, sc / w, pk / sc, pk / (sc / 2.0));
        }
}

int main()
{
    Bufs b;
    std::vector<float> h(8 * kMaxThreads);
    for (int i = 0; i < kMaxThreads; ++i) {
        float *p = &h[8 * i];
        p[0] = 1.0f; p[1] = -1.0f; p[2] = 0.0f; p[3] = 0.0f; p[4] = 1.0f; p[5] = 0.0f; p[6] = 1.0f + 1e-3f * (float)i; p[7] = 2.0f;
    }
    CHECK(hipMalloc(&b.in, sizeof(float) * h.size()));
    CHECK(hipMalloc(&b.out, sizeof(float) * kMaxThreads));
    CHECK(hipMalloc(&b.cyc, sizeof(unsigned long long) * (kMaxThreads / 64)));
    CHECK(hipMemcpy(b.in, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
    for (int i = 0; i < 20; ++i) run<FMA_PPP, false, 8>(b, 4);       // clocks up, code loaded
    printf("cycles per pair operation: %d iterations x %d unrolled x chains (8 independent, 1 dependent); one workgroup, waves per SIMD in column 3\n", kIters, kUnroll);
    printf("%-24s %-11s w  | packed cyc/pair cyc/instr simd cyc/pair | plain cyc/pair cyc/instr simd cyc/pair |\n", "helper", "stream");
    report<FMA_PPP>(b); report<FMA_PSP>(b); report<FMA_PSS>(b); report<MUL_PP>(b); report<ADD_PP>(b); report<RSUB_SP>(b);
    CHECK(hipFree(b.in)); CHECK(hipFree(b.out)); CHECK(hipFree(b.cyc));
    return 0;
}
