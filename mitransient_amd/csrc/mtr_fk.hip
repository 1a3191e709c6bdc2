// mtr_fk.hip — the three passes of f-k migration around the caller's two FFTs (additive, ABI 24).  A translation unit of its
// own: the kernels of every other file keep their instructions.  The arithmetic is mtr_fk.h's.
//
//   k_fk_prepare   one thread per 16 bytes of P (2H, 2W, 2T'), taken as one flat array (2T' need not be a multiple of 4: a
//                  thread's four elements may end one depth row and begin the next).  Every element is stored, the zeros of the
//                  padding included: no memset pass.  A thread inside the padded half of a row stores zeros without looking at
//                  the capture; one inside the low corner adds its q bins per element in increasing order.
//   k_fk_stolt     a workgroup owns one row (iy, ix) of the spectrum.  A row of at most kFkStage elements is copied to LDS first
//                  (coalesced float2 loads), a longer one is read where it lies: the taps of consecutive outputs are at most one
//                  element apart, so either way they are near-sequential.  A thread stores two outputs as one float4; the zero
//                  half of G's row (kz <= 0) is stored without arithmetic.
//   k_fk_finish    a workgroup owns a 64 x 64 (depth, scan column) tile of one scan row: |g|^2 is read depth-fastest (a wave reads
//                  512 contiguous bytes), goes through an LDS tile with a pitch of 65 words, and is stored x-fastest.
//
// No thread adds to what another wrote: the same call gives the same bits.  All element indices are 64-bit.
#include "mtr_fk.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

__global__ void __launch_bounds__(kFkBlock) k_fk_prepare(const FkArgs a, const float *__restrict__ capture, const int32_t *__restrict__ shift,
                                                         float4 *__restrict__ padded, uint64_t n4)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFkBlock + threadIdx.x;
    if (i >= n4) return;
    const uint32_t L = 2u * a.Tp;
    const uint64_t e = 4u * i;
    uint32_t r = (uint32_t)(e / L), k = (uint32_t)(e - (uint64_t)r * L);             // (r < 2H 2W < 2^32: fk_check)
    float v[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (!(k >= a.Tp && k + 3u < L)) {                                                // (otherwise: four elements of one row's padding)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = fk_prepare_at(a, capture, shift, r, k);
            if (++k == L) { k = 0u; ++r; }                                          // (the last thread's r may reach 2H 2W: not used again)
        }
    }
    padded[i] = make_float4(v[0], v[1], v[2], v[3]);
}

template <bool STAGED>
__global__ void __launch_bounds__(kFkBlock) k_fk_stolt(const FkArgs a, const float2 *__restrict__ spectrum, float4 *__restrict__ resampled)
{
    __shared__ float2 staged[STAGED ? kFkStage : 1u];
    const uint32_t ix = blockIdx.x, iy = blockIdx.y, tid = threadIdx.x;             // (ix < 2W, iy < 2H: the grid)
    const uint64_t row = (uint64_t)iy * (2u * a.W) + ix;
    const float2 *__restrict__ src = spectrum + row * ((uint64_t)a.Tp + 1u);
    if (STAGED) {
        for (uint32_t i = tid; i <= a.Tp; i += kFkBlock) staged[i] = src[i];         // (Tp + 1 <= kFkStage: launch_fk_stolt)
        __syncthreads();
    }
    const float lateral = fk_lateral(a, iy, ix);
    float4 *__restrict__ dst = resampled + row * (uint64_t)a.Tp;                    // (2 Tp complex = Tp float4)
    for (uint32_t j = tid; j < a.Tp; j += kFkBlock) {
        float o[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (uint32_t c = 0u; c < 2u; ++c) {
            uint32_t i0; float w, jac;
            if (fk_tap(a.Tp, lateral, 2u * j + c, i0, w, jac)) {                    // (true: i0 + 1 <= Tp, inside the row)
                const float2 f0 = STAGED ? staged[i0] : src[i0], f1 = STAGED ? staged[i0 + 1u] : src[i0 + 1u];
                o[2u * c] = fk_mix(f0.x, f1.x, w, jac);
                o[2u * c + 1u] = fk_mix(f0.y, f1.y, w, jac);
            }
        }
        dst[j] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

__global__ void __launch_bounds__(kFkBlock) k_fk_finish(const FkArgs a, const float2 *__restrict__ field, float *__restrict__ volume, uint32_t n_xt)
{
    __shared__ float tile[kFkTile][kFkTile + 1u];
    const uint32_t zt = blockIdx.x / n_xt, xt = blockIdx.x - zt * n_xt, iy = blockIdx.y;        // (iy < H: the grid)
    const uint32_t zb = zt * kFkTile, xb = xt * kFkTile;
    const uint32_t lane = threadIdx.x % kFkTile, first = threadIdx.x / kFkTile;
    constexpr uint32_t kStep = kFkBlock / kFkTile;
    const uint64_t depth = 2ull * a.Tp;
    for (uint32_t tx = first; tx < kFkTile; tx += kStep) {
        const uint32_t x = xb + tx, z = zb + lane;
        if (x < a.W && z < a.nz) {                                                  // (z0 + z < Tp: fk_check)
            const float2 g = field[((uint64_t)iy * (2u * a.W) + x) * depth + a.z0 + z];
            tile[tx][lane] = fk_power(g.x, g.y);
        }
    }
    __syncthreads();
    for (uint32_t tz = first; tz < kFkTile; tz += kStep) {
        const uint32_t x = xb + lane, z = zb + tz;
        if (x < a.W && z < a.nz) volume[((uint64_t)z * a.H + iy) * a.W + x] = tile[lane][tz];
    }
}

} // namespace

hipError_t launch_fk_prepare(const FkArgs &a, const float *capture, const int32_t *shift, float *padded, hipStream_t stream)
{
    const uint64_t n4 = 2ull * a.H * a.W * a.Tp;                                     // (2H 2W 2T' floats, four to a thread)
    const uint64_t blocks = (n4 + kFkBlock - 1u) / kFkBlock;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fk_prepare, dim3((uint32_t)blocks), dim3(kFkBlock), 0, stream, a, capture, shift, (float4 *)padded, n4);
    return hipGetLastError();
}

hipError_t launch_fk_stolt(const FkArgs &a, const float *spectrum, float *resampled, hipStream_t stream)
{
    const dim3 grid(2u * a.W, 2u * a.H);                                            // (2H <= 65534: fk_check)
    if (a.Tp + 1u <= kFkStage) hipLaunchKernelGGL((k_fk_stolt<true>), grid, dim3(kFkBlock), 0, stream, a, (const float2 *)spectrum, (float4 *)resampled);
    else hipLaunchKernelGGL((k_fk_stolt<false>), grid, dim3(kFkBlock), 0, stream, a, (const float2 *)spectrum, (float4 *)resampled);
    return hipGetLastError();
}

hipError_t launch_fk_finish(const FkArgs &a, const float *field, float *volume, hipStream_t stream)
{
    const uint32_t n_xt = (a.W + kFkTile - 1u) / kFkTile, n_zt = (a.nz + kFkTile - 1u) / kFkTile;
    if ((uint64_t)n_xt * n_zt > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fk_finish, dim3(n_xt * n_zt, a.H), dim3(kFkBlock), 0, stream, a, (const float2 *)field, volume, n_xt);
    return hipGetLastError();
}

} // namespace mtr
