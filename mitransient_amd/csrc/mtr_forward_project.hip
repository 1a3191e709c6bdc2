// mtr_forward_project.hip — mtr_forward_project (additive, ABI 24): a voxel volume scattered into a NLOS capture, the transpose
// of mtr_backproject.  A translation unit of its own: the kernels of every other file keep their instructions.  The arithmetic
// is mtr_forward_project.h's (fp_taps over bp_path and the lookups of mtr_backproject.h).
//
//   k_forward_project         a workgroup owns one capture row p, one window of at most kFpWindow bins of it and one slab of
//                             voxels.  The window lives in LDS, zeroed first.  The scan-point record of the row has a
//                             wave-uniform address and is read with scalar loads.  The threads stride over
//                             the slab's voxels in linear index order (ix fastest: the volume is read coalesced, the next
//                             voxel's value while this one is worked on), skip the voxels that are exactly 0 (volumes are
//                             sparse; a NaN is not 0), and add their taps into the window with LDS float atomics
//                             (ds_add_f32, no compare-and-swap loop: -munsafe-fp-atomics).  After a barrier the window is
//                             stored, coalesced: every cell of the output is written.  One slab: to the capture.  More: to
//                             plane `slab` of `partial`.
//   k_forward_project_reduce  one thread per cell: the planes added in slab order and stored.  No global float atomics anywhere.
//
// The order of the LDS adds inside a workgroup is not fixed: the same call gives the same capture to rounding, not to bits.
#include "mtr_forward_project.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

template <uint32_t CAPTURE, bool LINEAR>
__global__ void __launch_bounds__(kFpBlock) k_forward_project(const BpArgs a, const FpPlan pl, const float *__restrict__ x,
                                                              float *__restrict__ out)
{
    extern __shared__ float win[];                                                 // [window_len]
    const uint32_t tid = threadIdx.x, slab = blockIdx.y;
    const uint32_t p = blockIdx.x / pl.n_windows, w0 = (blockIdx.x - p * pl.n_windows) * kFpWindow;      // (p < n_pairs: the grid)
    const uint32_t wn = a.T - w0 < kFpWindow ? a.T - w0 : kFpWindow;               // (w0 < T: n_windows = ceil(T / kFpWindow))
    for (uint32_t i = tid; i < wn; i += kFpBlock) win[i] = 0.0f;                   // (wn <= window_len floats of LDS)
    __syncthreads();

    const FpRow r = fp_row<CAPTURE>(a, p);
    // the walk: index e of the slab counts (ix fastest, iy, iz); a step of kFpBlock is (dx, dy, dz) with at most one carry per axis
    const uint32_t n_vox = a.nx * a.ny * a.nz;
    const uint64_t e0 = (uint64_t)slab * pl.slab_len;
    const uint32_t e1 = e0 + pl.slab_len < n_vox ? (uint32_t)(e0 + pl.slab_len) : n_vox;      // ragged last slab
    const uint32_t dx = kFpBlock % a.nx, dy = (kFpBlock / a.nx) % a.ny, dz = (kFpBlock / a.nx) / a.ny;
    uint64_t e = e0 + tid;
    uint32_t ix = 0u, iy = 0u, iz = 0u;
    if (e < e1) { ix = (uint32_t)e % a.nx; const uint32_t t = (uint32_t)e / a.nx; iy = t % a.ny; iz = t / a.ny; }
    float xv = e < e1 ? x[e] : 0.0f;                                                // (e < e1 <= n_vox whenever the volume is read)
    for (; e < e1; e += kFpBlock) {
        const float vx = bp_centre(a.vmin[0], a.step[0], ix), vy = bp_centre(a.vmin[1], a.step[1], iy), vz = bp_centre(a.vmin[2], a.step[2], iz);
        ix += dx; if (ix >= a.nx) { ix -= a.nx; ++iy; }
        iy += dy; if (iy >= a.ny) { iy -= a.ny; ++iz; }
        iz += dz;
        const float xn = e + kFpBlock < e1 ? x[e + kFpBlock] : 0.0f;                // the next voxel's value is on its way meanwhile
        if (xv != 0.0f)                                                             // (a NaN is not skipped)
            fp_taps<CAPTURE, LINEAR>(a, r, vx, vy, vz, xv, [&](uint32_t b, float val) {
                const uint32_t i = b - w0;                                          // (b < w0 wraps above wn)
                if (i < wn) atomicAdd(&win[i], val);
            });
        xv = xn;
    }
    __syncthreads();
    float *dst = out + ((size_t)slab * a.n_pairs + p) * a.T + w0;
    for (uint32_t i = tid; i < wn; i += kFpBlock) dst[i] = win[i];
}

__global__ void __launch_bounds__(kFpBlock) k_forward_project_reduce(const float *__restrict__ partial, float *__restrict__ capture,
                                                                     size_t n_cells, uint32_t n_slabs)
{
    const size_t i = (size_t)blockIdx.x * kFpBlock + threadIdx.x;
    if (i >= n_cells) return;
    float acc = 0.0f;
    for (uint32_t sl = 0; sl < n_slabs; ++sl) acc += partial[(size_t)sl * n_cells + i];
    capture[i] = acc;
}

template <uint32_t CAPTURE>
void launch_capture(const BpArgs &a, const FpPlan &pl, const float *x, float *out, hipStream_t stream)
{
    const dim3 grid((uint32_t)pl.n_groups, pl.n_slabs);
    const size_t lds = (size_t)pl.window_len * sizeof(float);
    if (a.linear) hipLaunchKernelGGL((k_forward_project<CAPTURE, true>), grid, dim3(kFpBlock), lds, stream, a, pl, x, out);
    else hipLaunchKernelGGL((k_forward_project<CAPTURE, false>), grid, dim3(kFpBlock), lds, stream, a, pl, x, out);
}

} // namespace

hipError_t launch_forward_project(const BpArgs &a, const FpPlan &pl, const float *volume, float *partial, float *capture, hipStream_t stream)
{
    float *out = pl.n_slabs > 1u ? partial : capture;
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) launch_capture<MTR_CAPTURE_CONFOCAL>(a, pl, volume, out, stream);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) launch_capture<MTR_CAPTURE_SINGLE>(a, pl, volume, out, stream);
    else launch_capture<MTR_CAPTURE_EXHAUSTIVE>(a, pl, volume, out, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || pl.n_slabs <= 1u) return e;
    const size_t n_cells = (size_t)a.n_pairs * a.T;
    hipLaunchKernelGGL(k_forward_project_reduce, dim3((uint32_t)((n_cells + kFpBlock - 1u) / kFpBlock)), dim3(kFpBlock), 0, stream,
                       (const float *)partial, capture, n_cells, pl.n_slabs);
    return hipGetLastError();
}

} // namespace mtr

// test hook of the library, outside the C ABI of include/mitransient_amd.h: fp_plan without a device;
// out = { n_windows, n_slabs, slab_len (low word), slab_len (high word), kFpWindow }; returns 0 when there is no plan
extern "C" int mtr_test_forward_project_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, uint32_t T, int n_cu, uint32_t *out)
{
    mtr::FpPlan pl;
    if (!mtr::fp_plan(nx, ny, nz, n_pairs, T, n_cu, pl)) return 0;
    out[0] = pl.n_windows; out[1] = pl.n_slabs; out[2] = (uint32_t)pl.slab_len; out[3] = (uint32_t)(pl.slab_len >> 32); out[4] = mtr::kFpWindow;
    return 1;
}
