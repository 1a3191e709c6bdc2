// mtr_phasor_forward_project.hip — mtr_phasor_forward_project (additive, ABI 24): a complex voxel volume turned into the phasors
// of a NLOS capture, the conjugate transpose of mtr_phasor_backproject.  A translation unit of its own: the kernels of every
// other file keep their instructions.  The arithmetic is mtr_phasor_forward_project.h's (pf_voxel over pb_anchor / pb_rotate).
//
//   k_phasor_forward_project  a workgroup owns one row p, one block of kPbAnchor = 16 frequencies and one slab of voxels.  The
//                             scan-point record of the row and the block's frequencies have wave-uniform addresses and are read
//                             with scalar loads before the walk.  The threads stride over the slab's voxels in linear index
//                             order (ix fastest: U is read as coalesced float2, the next voxel's value while this one is worked
//                             on); a thread keeps the block's 16 complex sums in registers.  Then the 64 lanes of a wave are
//                             added with a butterfly (every lane ends with the same sum), the four waves through LDS in wave
//                             order, and thread k of the first 16 stores (p, k0 + k).  One slab: times w_k, to the phasors.
//                             More: unweighted, to plane `slab`.
//   k_pf_reduce               one thread per (p, k): the planes added in slab order, times w_k, stored.
//
// Every thread's voxels, the tree and the slab order are fixed: the same call gives the same bits.  No float atomics anywhere.
#include "mtr_phasor_forward_project.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

constexpr uint32_t kPfWaves = kPfBlock / 64u;
static_assert(kPfBlock % 64u == 0u && kPbAnchor * 2u <= 64u, "the first wave stores a block's 2 x 16 sums");

template <uint32_t CAPTURE, bool UNIFORM, bool FULL>
__device__ __forceinline__ void pf_walk(const PbArgs &a, const PfRow &r, const float *fk, uint32_t nk, const float2 *__restrict__ u,
                                        uint32_t e0, uint32_t e1, float *qr, float *qi)
{
    // index e of the slab counts (ix fastest, iy, iz); a step of kPfBlock is (dx, dy, dz) with at most one carry per axis
    const uint32_t dx = kPfBlock % a.nx, dy = (kPfBlock / a.nx) % a.ny, dz = (kPfBlock / a.nx) / a.ny;
    uint32_t e = e0 + threadIdx.x;                                                  // (e1 <= n_vox < 2^31: no wrap)
    if (e >= e1) return;
    uint32_t ix = e % a.nx, t = e / a.nx, iy = t % a.ny, iz = t / a.ny;
    float2 uv = u[e];                                                               // (e < e1 <= n_vox whenever U is read)
    for (; e < e1; e += kPfBlock) {
        const float vx = bp_centre(a.vmin[0], a.step[0], ix), vy = bp_centre(a.vmin[1], a.step[1], iy), vz = bp_centre(a.vmin[2], a.step[2], iz);
        ix += dx; if (ix >= a.nx) { ix -= a.nx; ++iy; }
        iy += dy; if (iy >= a.ny) { iy -= a.ny; ++iz; }
        iz += dz;
        const float2 un = e + kPfBlock < e1 ? u[e + kPfBlock] : make_float2(0.0f, 0.0f);
        pf_voxel<CAPTURE, UNIFORM, FULL>(r, a.start_opl, a.freq_step, a.tau_min, a.tau_max, fk, nk, vx, vy, vz, uv.x, uv.y, qr, qi);
        uv = un;
    }
}

template <uint32_t CAPTURE, bool UNIFORM>
__global__ void __launch_bounds__(kPfBlock) k_phasor_forward_project(const PbArgs a, const PfPlan pl, const float2 *__restrict__ u,
                                                                     float2 *__restrict__ out, uint32_t weighted)
{
    __shared__ float part[kPfWaves][2u * kPbAnchor];
    const uint32_t tid = threadIdx.x, slab = blockIdx.y;
    const uint32_t p = blockIdx.x / pl.n_blocks, k0 = (blockIdx.x - p * pl.n_blocks) * kPbAnchor;      // (p < n_pairs, k0 < F: the grid)
    const uint32_t nk = a.F - k0 < kPbAnchor ? a.F - k0 : kPbAnchor;
    const PfRow r = pf_row<CAPTURE>(a, p);
    float fk[kPbAnchor];
#pragma unroll
    for (uint32_t j = 0u; j < kPbAnchor; ++j) fk[j] = a.frequencies[k0 + (j < nk ? j : nk - 1u)];       // (inside the table)
    float qr[kPbAnchor], qi[kPbAnchor];
#pragma unroll
    for (uint32_t j = 0u; j < kPbAnchor; ++j) { qr[j] = 0.0f; qi[j] = 0.0f; }

    const uint32_t n_vox = a.nx * a.ny * a.nz;
    const uint64_t e0 = (uint64_t)slab * pl.slab_len;                               // (< n_vox: n_slabs = ceil(n_vox / slab_len))
    const uint32_t e1 = e0 + pl.slab_len < n_vox ? (uint32_t)(e0 + pl.slab_len) : n_vox;      // ragged last slab
    if (nk == kPbAnchor) pf_walk<CAPTURE, UNIFORM, true>(a, r, fk, nk, u, (uint32_t)e0, e1, qr, qi);
    else pf_walk<CAPTURE, UNIFORM, false>(a, r, fk, nk, u, (uint32_t)e0, e1, qr, qi);

    // the lanes of a wave, a butterfly: every lane ends with the wave's sum, the same tree whatever the lane
#pragma unroll
    for (uint32_t j = 0u; j < kPbAnchor; ++j) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { qr[j] += __shfl_xor(qr[j], m, 64); qi[j] += __shfl_xor(qi[j], m, 64); }
    }
    const uint32_t wave = tid / 64u, lane = tid & 63u;
    if (lane == 0u) {
#pragma unroll
        for (uint32_t j = 0u; j < kPbAnchor; ++j) { part[wave][2u * j] = qr[j]; part[wave][2u * j + 1u] = qi[j]; }
    }
    __syncthreads();
    if (tid < nk) {                                                                 // the waves in wave order
        float sr = part[0][2u * tid], si = part[0][2u * tid + 1u];
#pragma unroll
        for (uint32_t w = 1u; w < kPfWaves; ++w) { sr += part[w][2u * tid]; si += part[w][2u * tid + 1u]; }
        const uint32_t k = k0 + tid;
        if (weighted) { const float wk = a.weights[k]; sr = wk * sr; si = wk * si; }
        out[((size_t)slab * a.n_pairs + p) * a.F + k] = make_float2(sr, si);         // (slab 0 of one: the phasors themselves)
    }
}

__global__ void __launch_bounds__(kPfBlock) k_pf_reduce(const float2 *__restrict__ planes, const float *__restrict__ weights,
                                                        float2 *__restrict__ phasors, size_t n, uint32_t F, uint32_t n_slabs)
{
    const size_t i = (size_t)blockIdx.x * kPfBlock + threadIdx.x;
    if (i >= n) return;
    float re = 0.0f, im = 0.0f;
    for (uint32_t sl = 0; sl < n_slabs; ++sl) { const float2 v = planes[(size_t)sl * n + i]; re += v.x; im += v.y; }
    if (weights) { const float w = weights[i % F]; re = w * re; im = w * im; }
    phasors[i] = make_float2(re, im);
}

template <uint32_t CAPTURE>
void launch_rows(const PbArgs &a, const PfPlan &pl, const float2 *u, float2 *out, uint32_t weighted, hipStream_t stream)
{
    const dim3 grid((uint32_t)pl.n_groups, pl.n_slabs);
    if (a.uniform) hipLaunchKernelGGL((k_phasor_forward_project<CAPTURE, true>), grid, dim3(kPfBlock), 0, stream, a, pl, u, out, weighted);
    else hipLaunchKernelGGL((k_phasor_forward_project<CAPTURE, false>), grid, dim3(kPfBlock), 0, stream, a, pl, u, out, weighted);
}

} // namespace

hipError_t launch_phasor_forward_project(const PbArgs &a, const PfPlan &pl, const float *volume, float *planes, float *phasors, hipStream_t stream)
{
    const bool one = pl.n_slabs <= 1u;
    float2 *out = one ? (float2 *)phasors : (float2 *)planes;
    const uint32_t weighted = one && a.weights ? 1u : 0u;                            // (more slabs: k_pf_reduce weights the sum)
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) launch_rows<MTR_CAPTURE_CONFOCAL>(a, pl, (const float2 *)volume, out, weighted, stream);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) launch_rows<MTR_CAPTURE_SINGLE>(a, pl, (const float2 *)volume, out, weighted, stream);
    else launch_rows<MTR_CAPTURE_EXHAUSTIVE>(a, pl, (const float2 *)volume, out, weighted, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || one) return e;
    const size_t n = (size_t)a.n_pairs * a.F;
    hipLaunchKernelGGL(k_pf_reduce, dim3((uint32_t)((n + kPfBlock - 1u) / kPfBlock)), dim3(kPfBlock), 0, stream,
                       (const float2 *)planes, a.weights, (float2 *)phasors, n, a.F, pl.n_slabs);
    return hipGetLastError();
}

} // namespace mtr

// test hook of the library, outside the C ABI of include/mitransient_amd.h: pf_plan without a device;
// out = { n_blocks, n_slabs, slab_len (low word), slab_len (high word), kPbAnchor }; returns 0 when there is no plan
extern "C" int mtr_test_phasor_forward_project_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, uint32_t F, int n_cu, uint32_t *out)
{
    mtr::PfPlan pl;
    if (!mtr::pf_plan(nx, ny, nz, n_pairs, F, n_cu, pl)) return 0;
    out[0] = pl.n_blocks; out[1] = pl.n_slabs; out[2] = (uint32_t)pl.slab_len; out[3] = (uint32_t)(pl.slab_len >> 32); out[4] = mtr::kPbAnchor;
    return 1;
}
