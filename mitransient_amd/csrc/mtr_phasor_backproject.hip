// mtr_phasor_backproject.hip — mtr_phasor_backproject (additive, ABI 24): the phasors of a NLOS capture propagated back into a
// complex voxel volume.  A translation unit of its own: the kernels of every other file keep their instructions.  The arithmetic
// is mtr_phasor_backproject.h's (pb_voxel).
//
//   k_pb_weight            weights given: w_k P[p, k] of every row, two f32 products per element, into the workspace — the path
//                          kernel then reads rows that are weighted already (a product of two wave-uniform values per term would
//                          be vector work of every wave: there is no scalar f32 multiply on gfx950).
//   k_phasor_backproject   k_backproject's tiling: a workgroup is 8 x 8 x 4 neighbouring voxels, a thread one voxel.  The thread
//                          walks the pairs of its slab in ascending order.  Nothing is gathered: the scan-point record, the
//                          frequency table and the row P[p, .] have wave-uniform addresses and are read with scalar loads (a whole
//                          anchor block of 16 frequencies is 32 consecutive floats, a ragged one is read four frequencies at a
//                          time), and enter the f32 vector instructions of the inner loop as scalar operands.  One slab: the sum is stored to the volume.  More: to plane `slab`.
//   k_pb_reduce            one thread per voxel: the complex planes added in slab order and stored.  No float atomics anywhere.
#include "mtr_phasor_backproject.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

constexpr uint32_t kPbBlock = kBpTileX * kBpTileY * kBpTileZ;
static_assert(kPbBlock == 256u, "a tile is one voxel per thread of a 256-thread workgroup");

__global__ void __launch_bounds__(kPbBlock) k_pb_weight(const float2 *__restrict__ phasors, const float *__restrict__ weights,
                                                        float2 *__restrict__ out, size_t n, uint32_t F)
{
    const size_t i = (size_t)blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n) return;
    const float w = weights[i % F];
    const float2 p = phasors[i];
    out[i] = make_float2(w * p.x, w * p.y);
}

template <uint32_t CAPTURE, bool UNIFORM>
__global__ void __launch_bounds__(kPbBlock) k_phasor_backproject(const PbArgs a, const BpPlan pl, float2 *__restrict__ out)
{
    const uint32_t tile = blockIdx.x, slab = blockIdx.y;
    const uint32_t tz = tile / (pl.tx * pl.ty), r = tile - tz * (pl.tx * pl.ty), ty = r / pl.tx, tx = r - ty * pl.tx;
    const uint32_t tid = threadIdx.x;
    const uint32_t ix = tx * kBpTileX + (tid & (kBpTileX - 1u));
    const uint32_t iy = ty * kBpTileY + ((tid / kBpTileX) & (kBpTileY - 1u));
    const uint32_t iz = tz * kBpTileZ + tid / (kBpTileX * kBpTileY);
    if (!((ix < a.nx) & (iy < a.ny) & (iz < a.nz))) return;                     // (no barrier below)
    const uint64_t p0 = (uint64_t)slab * pl.slab_len;
    if (p0 >= a.n_pairs) return;
    const uint64_t p1 = (a.n_pairs - p0 < pl.slab_len) ? a.n_pairs : p0 + pl.slab_len;      // ragged last slab
    float re, im;
    pb_voxel<CAPTURE, UNIFORM, false>(a, ix, iy, iz, p0, p1, re, im);           // (weights given: the rows are k_pb_weight's)
    const size_t n_vox = (size_t)a.nx * a.ny * a.nz;
    out[(size_t)slab * n_vox + ((size_t)iz * a.ny + iy) * a.nx + ix] = make_float2(re, im);
}

__global__ void __launch_bounds__(kPbBlock) k_pb_reduce(const float2 *__restrict__ partial, float2 *__restrict__ volume,
                                                        size_t n_vox, uint32_t n_slabs)
{
    const size_t i = (size_t)blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n_vox) return;
    float re = 0.0f, im = 0.0f;
    for (uint32_t sl = 0; sl < n_slabs; ++sl) { const float2 v = partial[(size_t)sl * n_vox + i]; re += v.x; im += v.y; }
    volume[i] = make_float2(re, im);
}

template <uint32_t CAPTURE>
void launch_paths(const PbArgs &a, const BpPlan &pl, float2 *out, hipStream_t stream)
{
    const dim3 grid((uint32_t)pl.n_tiles, pl.n_slabs);
    if (a.uniform) hipLaunchKernelGGL((k_phasor_backproject<CAPTURE, true>), grid, dim3(kPbBlock), 0, stream, a, pl, out);
    else hipLaunchKernelGGL((k_phasor_backproject<CAPTURE, false>), grid, dim3(kPbBlock), 0, stream, a, pl, out);
}

} // namespace

hipError_t launch_phasor_backproject(const PbArgs &args, const BpPlan &pl, float *work, float *volume, hipStream_t stream)
{
    PbArgs a = args;
    const size_t n_weighted = pb_weighted_floats(a);
    if (n_weighted) {
        const size_t n = n_weighted / 2u;
        hipLaunchKernelGGL(k_pb_weight, dim3((uint32_t)((n + kPbBlock - 1u) / kPbBlock)), dim3(kPbBlock), 0, stream,
                           (const float2 *)a.phasors, a.weights, (float2 *)work, n, a.F);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        a.phasors = work; a.weights = nullptr;
    }
    float2 *planes = (float2 *)(work + n_weighted);
    float2 *out = pl.n_slabs > 1u ? planes : (float2 *)volume;
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) launch_paths<MTR_CAPTURE_CONFOCAL>(a, pl, out, stream);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) launch_paths<MTR_CAPTURE_SINGLE>(a, pl, out, stream);
    else launch_paths<MTR_CAPTURE_EXHAUSTIVE>(a, pl, out, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || pl.n_slabs <= 1u) return e;
    const size_t n_vox = (size_t)a.nx * a.ny * a.nz;
    hipLaunchKernelGGL(k_pb_reduce, dim3((uint32_t)((n_vox + kPbBlock - 1u) / kPbBlock)), dim3(kPbBlock), 0, stream,
                       (const float2 *)planes, (float2 *)volume, n_vox, pl.n_slabs);
    return hipGetLastError();
}

} // namespace mtr
