// mtr_forward_project.h — the arithmetic of mtr_forward_project (additive, ABI 24): the transpose of mtr_backproject, a voxel
// volume (nz, ny, nx) scattered into a NLOS capture (rows, T) — the three-bounce forward model of a hidden volume, and the
// gradient of a backprojection.  MTR_HD: the kernels of mtr_forward_project.hip and the host build of
// tests/host_forward_project.cpp compile this one text.
//
//   weights   backprojection is the linear map  volume[v] = sum over rows p, bins b of  W(v, p, b) capture[p, b]; this is
//             capture[p, b] = sum over voxels v of  W(v, p, b) volume[v]  with the same W: the path length d of (v, p) is
//             bp_path's (mtr_backproject.h — bp_voxel's expression, the same bits), the bin and the in-window decision are
//             bp_bin_nearest's / bp_bins_linear's.  nearest adds x[v] to bin floor(u); linear adds (1 - w) x[v] to b0 and
//             w x[v] to b0 + 1, each only where it lies in [0, T).  The pair is an exact transpose up to the order of the f32 sums.
//   order     the host build adds the voxels of a cell in ascending linear order (ix fastest).  The kernel adds them in LDS with
//             float atomics, whose order inside a workgroup is not fixed: the result is reproducible to rounding, NOT to
//             bits (a bit-deterministic mode is not offered).  Every cell of the capture is written; a cell nothing lands in is 0.
#ifndef MTR_FORWARD_PROJECT_H
#define MTR_FORWARD_PROJECT_H

#include "mtr_backproject.h"

namespace mtr {

// the scan-point record of capture row p: what bp_path needs beside the voxel
struct FpRow { float ps[3], pl[3], so, lo; };

template <uint32_t CAPTURE>
MTR_HD FpRow fp_row(const BpArgs &a, uint64_t p)
{
    const uint64_t s = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? p / a.L : p;
    const uint64_t l = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? p - s * a.L : (CAPTURE == MTR_CAPTURE_CONFOCAL ? s : 0u);
    FpRow r;
    for (int k = 0; k < 3; ++k) { r.ps[k] = a.sensor_points[(size_t)s * 3u + k]; r.pl[k] = a.laser_points[(size_t)l * 3u + k]; }
    r.so = a.sensor_offset[(size_t)s]; r.lo = a.laser_offset[(size_t)l];
    return r;
}

// The taps of voxel value x at (vx, vy, vz) in row r: add(bin, value) is called for each tap inside [0, T), lower tap first.
template <uint32_t CAPTURE, bool LINEAR, class Add>
MTR_HD void fp_taps(const BpArgs &a, const FpRow &r, float vx, float vy, float vz, float x, Add add)
{
    const float d = bp_path<CAPTURE>(r.ps, r.pl, r.so, r.lo, vx, vy, vz);
    if (LINEAR) {
        int64_t b0; float w;
        if (!bp_bins_linear(a.T, a.start_opl, a.bin_width, d, b0, w)) return;
        const int64_t b1 = b0 + 1;
        if (b0 >= 0 && b0 < (int64_t)a.T) add((uint32_t)b0, (1.0f - w) * x);
        if (b1 >= 0 && b1 < (int64_t)a.T) add((uint32_t)b1, w * x);
    } else {
        uint32_t b;
        if (bp_bin_nearest(a.T, a.start_opl, a.bin_width, d, b)) add(b, x);
    }
}

// The split of a call over workgroups: one workgroup per (capture row, window of at most kFpWindow bins, slab of voxels).  The
// window is the workgroup's LDS accumulator (kFpWindow floats = 64 KiB at most; a row of 4096 bins takes 16 KiB and leaves
// several workgroups per compute unit).  Rows x windows normally fill the device; only when they cannot (a Single capture of a
// few scan points into 128^3) the voxels are cut into n_slabs contiguous ranges of slab_len (linear index order), each summed
// into its own (rows, T) plane of `partial` and the planes added in slab order — no global float atomics.  The planes never
// take more than kFpPartialCap bytes: fewer slabs are used instead.
constexpr uint32_t kFpBlock = 256u;
constexpr uint32_t kFpWindow = 16384u;                                 // bins of one workgroup's LDS window
constexpr uint32_t kFpMinSlab = 4096u;                                 // voxels: a slab no shorter than this
constexpr uint32_t kFpPerCU = 4u;                                      // workgroups wanted per compute unit
constexpr uint64_t kFpPartialCap = 256ull << 20;                       // bytes of n_slabs * rows * T * 4
struct FpPlan { uint32_t n_windows, window_len, n_slabs; uint64_t slab_len, n_groups; };

inline bool fp_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, uint32_t T, int n_cu, FpPlan &pl)
{
    pl = FpPlan{};
    if (!nx || !ny || !nz || !n_pairs || !T || n_cu <= 0) return false;
    const uint64_t n_vox = (uint64_t)nx * ny * nz;
    if (n_vox > 0x7fffffffull || n_pairs > 0x7fffffffull) return false;     // (the kernel's voxel index is 32-bit; grid.x)
    pl.n_windows = (T + kFpWindow - 1u) / kFpWindow;
    pl.window_len = T < kFpWindow ? T : kFpWindow;
    pl.n_groups = n_pairs * pl.n_windows;
    if (pl.n_groups > 0x7fffffffull) return false;                     // (grid.x)
    const uint64_t cap = (uint64_t)n_cu * kFpPerCU;
    uint64_t want = pl.n_groups >= cap ? 1u : (cap + pl.n_groups - 1u) / pl.n_groups;
    const uint64_t most = (n_vox + kFpMinSlab - 1u) / kFpMinSlab;
    if (want > most) want = most;
    const uint64_t plane = n_pairs * T * sizeof(float);
    const uint64_t fit = kFpPartialCap / plane;                        // planes the cap has room for (0: none, one slab)
    if (want > fit) want = fit;
    if (want > 65535u) want = 65535u;
    if (want < 1u) want = 1u;
    pl.slab_len = (n_vox + want - 1u) / want;
    pl.n_slabs = (uint32_t)((n_vox + pl.slab_len - 1u) / pl.slab_len);
    return true;
}

#if defined(__HIPCC__)
// k_forward_project over the plan's rows, windows and slabs, then — more than one slab — k_forward_project_reduce
// (partial: n_slabs * rows * T floats of device memory, unused with one slab)
hipError_t launch_forward_project(const BpArgs &a, const FpPlan &pl, const float *volume, float *partial, float *capture, hipStream_t stream);
#endif

} // namespace mtr
#endif
