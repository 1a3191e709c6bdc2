// mtr_backproject.hip — mtr_backproject (additive, ABI 24): a NLOS capture summed back into a voxel volume.  A translation unit
// of its own: the kernels of every other file keep their instructions.  The arithmetic is mtr_backproject.h's (bp_voxel).
//
//   k_backproject         a workgroup is a tile of 8 x 8 x 4 neighbouring voxels, a thread one voxel, a wave one 8 x 8 slice of
//                         constant z.  The thread walks the pairs of its slab in ascending order: the scan-point record
//                         (P_s, so, P_l, lo) has a wave-uniform address and is read with scalar loads, the capture row is
//                         gathered from HBM / L2 — neighbouring voxels read neighbouring bins — and every tap is checked
//                         against [0, T) first.  One slab: the sum is stored to the volume.  More: to plane `slab` of `partial`.
//   k_backproject_reduce  one thread per voxel: the planes added in slab order and stored.  No float atomics anywhere.
#include "mtr_backproject.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

constexpr uint32_t kBpBlock = kBpTileX * kBpTileY * kBpTileZ;
static_assert(kBpBlock == 256u, "a tile is one voxel per thread of a 256-thread workgroup");

template <uint32_t CAPTURE, bool LINEAR>
__global__ void __launch_bounds__(kBpBlock) k_backproject(const BpArgs a, const BpPlan pl, float *__restrict__ out)
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
    const float v = bp_voxel<CAPTURE, LINEAR>(a, ix, iy, iz, p0, p1);
    const size_t n_vox = (size_t)a.nx * a.ny * a.nz;
    out[(size_t)slab * n_vox + ((size_t)iz * a.ny + iy) * a.nx + ix] = v;
}

__global__ void __launch_bounds__(kBpBlock) k_backproject_reduce(const float *__restrict__ partial, float *__restrict__ volume,
                                                                 size_t n_vox, uint32_t n_slabs)
{
    const size_t i = (size_t)blockIdx.x * kBpBlock + threadIdx.x;
    if (i >= n_vox) return;
    float acc = 0.0f;
    for (uint32_t sl = 0; sl < n_slabs; ++sl) acc += partial[(size_t)sl * n_vox + i];
    volume[i] = acc;
}

template <uint32_t CAPTURE>
void launch_paths(const BpArgs &a, const BpPlan &pl, float *out, hipStream_t stream)
{
    const dim3 grid((uint32_t)pl.n_tiles, pl.n_slabs);
    if (a.linear) hipLaunchKernelGGL((k_backproject<CAPTURE, true>), grid, dim3(kBpBlock), 0, stream, a, pl, out);
    else hipLaunchKernelGGL((k_backproject<CAPTURE, false>), grid, dim3(kBpBlock), 0, stream, a, pl, out);
}

} // namespace

hipError_t launch_backproject(const BpArgs &a, const BpPlan &pl, float *partial, float *volume, hipStream_t stream)
{
    float *out = pl.n_slabs > 1u ? partial : volume;
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) launch_paths<MTR_CAPTURE_CONFOCAL>(a, pl, out, stream);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) launch_paths<MTR_CAPTURE_SINGLE>(a, pl, out, stream);
    else launch_paths<MTR_CAPTURE_EXHAUSTIVE>(a, pl, out, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || pl.n_slabs <= 1u) return e;
    const size_t n_vox = (size_t)a.nx * a.ny * a.nz;
    hipLaunchKernelGGL(k_backproject_reduce, dim3((uint32_t)((n_vox + kBpBlock - 1u) / kBpBlock)), dim3(kBpBlock), 0, stream,
                       (const float *)partial, volume, n_vox, pl.n_slabs);
    return hipGetLastError();
}

} // namespace mtr

// test hook of the library, outside the C ABI of include/mitransient_amd.h: bp_plan without a device;
// out = { n_tiles, n_slabs, slab_len (low word), slab_len (high word) }; returns 0 when there is no plan
extern "C" int mtr_test_backproject_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, int n_cu, uint32_t *out)
{
    mtr::BpPlan pl;
    if (!mtr::bp_plan(nx, ny, nz, n_pairs, n_cu, pl)) return 0;
    out[0] = (uint32_t)pl.n_tiles; out[1] = pl.n_slabs; out[2] = (uint32_t)pl.slab_len; out[3] = (uint32_t)(pl.slab_len >> 32);
    return 1;
}
