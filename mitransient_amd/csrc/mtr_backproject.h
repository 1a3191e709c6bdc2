// mtr_backproject.h — the arithmetic of mtr_backproject (additive, ABI 24): unfiltered backprojection of a NLOS capture
// (H, W, T) into a voxel volume.  MTR_HD, like mtr_polar.h / mtr_nlos.h: the kernels of mtr_backproject.hip and the host build of
// tests/host_backproject.cpp compile this one text.
//
//   capture   S sensor points P_s (relay-wall points in film order [y][x]), L laser points P_l, T bins of bin_width from start_opl.
//             Confocal (L = S): pairs {(s, s)}, rows (S, T).  Single (L = 1): pairs {(s, 0)}, rows (S, T).  Exhaustive: every
//             (s, l), rows (S, L, T) — the film's own order [y][x][laser_x][laser_y][t], l = laser_x * Ly + laser_y.
//   path      d = ((|P_s - v| + |v - P_l|) + so[s]) + lo[l] for the voxel centre v; so / lo are the sensor -> wall and
//             laser -> wall legs of a capture rendered with account_first_and_last_bounces, zeros otherwise.  Every norm is
//             sqrtf((dx*dx + dy*dy) + dz*dz), no fma (the Makefile's -ffp-contract=off), the sums in the order written.
//   lookup    u = (d - start_opl) / bin_width.  nearest: bin floor(u), film_bin's expression (mtr_core.h) — a rendered
//             three-bounce contribution is read from the bin it was splatted into.  linear: u' = u - 0.5, b0 = floor(u'),
//             w = u' - b0, (1 - w) H[b0] + w H[b0 + 1].  A tap outside [0, T) contributes 0 and is never read.
//   volume    box [vmin, vmax], (nx, ny, nz) voxels, centres vmin + (i + 0.5) * ((vmax - vmin) / n); a voxel's value is the
//             sum over its pairs in ascending (s, l) order.
#ifndef MTR_BACKPROJECT_H
#define MTR_BACKPROJECT_H

#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include "../../include/mitransient_amd.h"

#ifndef MTR_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MTR_HD __host__ __device__ __forceinline__
#else
#define MTR_HD inline __attribute__((always_inline))
#endif
#endif

namespace mtr {

// mtr_backproject_desc, checked (bp_check) and with the pair count worked out
struct BpArgs {
    uint32_t capture_type, linear;
    uint32_t S, L, T;
    float start_opl, bin_width;
    float vmin[3], step[3];             // step = (vmax - vmin) / n
    uint32_t nx, ny, nz;
    uint64_t n_pairs;                   // S (Confocal, Single) or S * L (Exhaustive): the rows of the capture
    const float *sensor_points, *laser_points, *sensor_offset, *laser_offset;
    const float *capture;
};

MTR_HD float bp_norm(float dx, float dy, float dz) { return sqrtf((dx * dx + dy * dy) + dz * dz); }

MTR_HD float bp_centre(float vmin, float step, uint32_t i) { return vmin + ((float)i + 0.5f) * step; }

// the value of one capture row (T bins) at path length d; every tap is checked against [0, T) before it is read
MTR_HD float bp_tap_nearest(const float *row, uint32_t T, float start_opl, float bin_width, float d)
{
    const float u = (d - start_opl) / bin_width;
    if (!(u >= 0.0f && u < (float)T)) return 0.0f;
    const uint32_t b = (uint32_t)floorf(u);
    return b < T ? row[b] : 0.0f;       // ((float)T rounds up above 2^24 bins: the integer test decides)
}

MTR_HD float bp_tap_linear(const float *row, uint32_t T, float start_opl, float bin_width, float d)
{
    const float u = (d - start_opl) / bin_width - 0.5f;
    if (!(u >= -1.0f && u < (float)T)) return 0.0f;      // both taps outside (or a NaN)
    const float b0f = floorf(u);
    const float w = u - b0f;
    const int64_t b0 = (int64_t)b0f, b1 = b0 + 1;
    const float h0 = (b0 >= 0 && b0 < (int64_t)T) ? row[b0] : 0.0f;
    const float h1 = (b1 >= 0 && b1 < (int64_t)T) ? row[b1] : 0.0f;
    return (1.0f - w) * h0 + w * h1;
}

// The same lookups and the same path length for the transpose (mtr_forward_project.h), which adds where bp_tap_* read: the
// operations of bp_tap_nearest / bp_tap_linear / bp_voxel in their order, restated rather than shared so that k_backproject
// keeps its instructions.  nearest: the bin, or false outside the window.  linear: the lower tap b0 (b0 + 1 is the other;
// either may lie outside [0, T)) and the weight w of the upper one, or false when both lie outside.
MTR_HD bool bp_bin_nearest(uint32_t T, float start_opl, float bin_width, float d, uint32_t &b)
{
    const float u = (d - start_opl) / bin_width;
    if (!(u >= 0.0f && u < (float)T)) return false;
    b = (uint32_t)floorf(u);
    return b < T;
}

MTR_HD bool bp_bins_linear(uint32_t T, float start_opl, float bin_width, float d, int64_t &b0, float &w)
{
    const float u = (d - start_opl) / bin_width - 0.5f;
    if (!(u >= -1.0f && u < (float)T)) return false;
    const float b0f = floorf(u);
    w = u - b0f;
    b0 = (int64_t)b0f;
    return true;
}

// the path length of voxel centre (vx, vy, vz) for one pair (P_s, so), (P_l, lo); Confocal never reads pl
template <uint32_t CAPTURE>
MTR_HD float bp_path(const float *ps, const float *pl, float so, float lo, float vx, float vy, float vz)
{
    const float r1 = bp_norm(ps[0] - vx, ps[1] - vy, ps[2] - vz);
    float r2 = r1;                                          // Confocal: P_l = P_s, and (-x)^2 = x^2 — the same bits
    if (CAPTURE != MTR_CAPTURE_CONFOCAL) r2 = bp_norm(vx - pl[0], vy - pl[1], vz - pl[2]);
    return ((r1 + r2) + so) + lo;
}

// the sum of voxel (ix, iy, iz) over the pairs [p0, p1) of the capture's rows, ascending
template <uint32_t CAPTURE, bool LINEAR>
MTR_HD float bp_voxel(const BpArgs &a, uint32_t ix, uint32_t iy, uint32_t iz, uint64_t p0, uint64_t p1)
{
    const float vx = bp_centre(a.vmin[0], a.step[0], ix), vy = bp_centre(a.vmin[1], a.step[1], iy), vz = bp_centre(a.vmin[2], a.step[2], iz);
    uint64_t s = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? p0 / a.L : p0;
    uint32_t l = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? (uint32_t)(p0 - s * a.L) : 0u;
    float acc = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4                        // (four gathers in flight per thread; the additions keep their order)
#endif
    for (uint64_t p = p0; p < p1; ++p) {
        const float *ps = a.sensor_points + (size_t)s * 3u;
        const float r1 = bp_norm(ps[0] - vx, ps[1] - vy, ps[2] - vz);
        float r2 = r1, lo;                                  // Confocal: P_l = P_s, and (-x)^2 = x^2 — the same bits
        if (CAPTURE == MTR_CAPTURE_CONFOCAL) lo = a.laser_offset[(size_t)s];
        else {
            const float *pl = a.laser_points + (size_t)l * 3u;
            r2 = bp_norm(vx - pl[0], vy - pl[1], vz - pl[2]);
            lo = a.laser_offset[(size_t)l];
        }
        const float d = ((r1 + r2) + a.sensor_offset[(size_t)s]) + lo;      // (bp_path restates this for the transpose)
        const float *row = a.capture + (size_t)p * a.T;
        acc += LINEAR ? bp_tap_linear(row, a.T, a.start_opl, a.bin_width, d) : bp_tap_nearest(row, a.T, a.start_opl, a.bin_width, d);
        if (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) { if (++l == a.L) { l = 0u; ++s; } }
        else ++s;
    }
    return acc;
}

// MTR_ERR_INVALID's cases of mtr_backproject: the message, or NULL for a description that can run
inline const char *bp_check(const mtr_backproject_desc *d, const float *capture, const float *volume)
{
    if (!d || !capture || !volume) return "NULL argument";
    if (!d->sensor_points || !d->laser_points || !d->sensor_offset || !d->laser_offset) return "NULL point or offset array";
    if (d->capture_type != MTR_CAPTURE_SINGLE && d->capture_type != MTR_CAPTURE_CONFOCAL && d->capture_type != MTR_CAPTURE_EXHAUSTIVE)
        return "unknown capture type";
    if (d->interpolation != MTR_BACKPROJECT_NEAREST && d->interpolation != MTR_BACKPROJECT_LINEAR) return "unknown interpolation";
    if (d->n_sensor == 0u || d->n_laser == 0u || d->temporal_bins == 0u) return "a capture of zero size";
    if (d->nx == 0u || d->ny == 0u || d->nz == 0u) return "a volume of zero size";
    if (d->capture_type == MTR_CAPTURE_CONFOCAL && d->n_laser != d->n_sensor) return "a Confocal capture has one laser point per sensor point";
    if (d->capture_type == MTR_CAPTURE_SINGLE && d->n_laser != 1u) return "a Single capture has one laser point";
    if (!(d->bin_width_opl > 0.0f) || !(fabsf(d->bin_width_opl) <= 3.402823466e+38f)) return "bin_width_opl must be positive";
    if (!(fabsf(d->start_opl) <= 3.402823466e+38f)) return "start_opl must be finite";
    for (int k = 0; k < 3; ++k)
        if (!(d->volume_max[k] > d->volume_min[k]) || !(fabsf(d->volume_max[k] - d->volume_min[k]) <= 3.402823466e+38f)) return "an empty volume box";
    return nullptr;
}

inline BpArgs bp_args(const mtr_backproject_desc &d, const float *capture)
{
    BpArgs a{};
    a.capture_type = d.capture_type; a.linear = d.interpolation == MTR_BACKPROJECT_LINEAR ? 1u : 0u;
    a.S = d.n_sensor; a.L = d.n_laser; a.T = d.temporal_bins;
    a.start_opl = d.start_opl; a.bin_width = d.bin_width_opl;
    const uint32_t n[3] = { d.nx, d.ny, d.nz };
    for (int k = 0; k < 3; ++k) { a.vmin[k] = d.volume_min[k]; a.step[k] = (d.volume_max[k] - d.volume_min[k]) / (float)n[k]; }
    a.nx = d.nx; a.ny = d.ny; a.nz = d.nz;
    a.n_pairs = d.capture_type == MTR_CAPTURE_EXHAUSTIVE ? (uint64_t)d.n_sensor * d.n_laser : (uint64_t)d.n_sensor;
    a.sensor_points = d.sensor_points; a.laser_points = d.laser_points; a.sensor_offset = d.sensor_offset; a.laser_offset = d.laser_offset;
    a.capture = capture;
    return a;
}

// The split of a call over workgroups: tiles of kBpTileX x kBpTileY x kBpTileZ voxels (one voxel per thread), and — few voxels,
// many pairs — the pairs cut into n_slabs contiguous ranges of slab_len, each summed into its own (voxels) plane of `partial`
// and the planes added in slab order (k_samples_paths / k_samples_reduce's scheme: the order stays fixed, no float atomics).
constexpr uint32_t kBpTileX = 8u, kBpTileY = 8u, kBpTileZ = 4u;       // 256 threads; a wave is one 8 x 8 slice of constant z
constexpr uint32_t kBpMinSlab = 64u;                                   // pairs: a slab no shorter than this
constexpr uint32_t kBpPerCU = 8u;                                      // workgroups a compute unit keeps resident
struct BpPlan { uint32_t tx, ty, tz; uint64_t n_tiles; uint32_t n_slabs; uint64_t slab_len; };

inline bool bp_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, int n_cu, BpPlan &pl)
{
    pl = BpPlan{};
    if (!nx || !ny || !nz || !n_pairs || n_cu <= 0) return false;
    pl.tx = (nx + kBpTileX - 1u) / kBpTileX; pl.ty = (ny + kBpTileY - 1u) / kBpTileY; pl.tz = (nz + kBpTileZ - 1u) / kBpTileZ;
    pl.n_tiles = (uint64_t)pl.tx * pl.ty * pl.tz;
    if (pl.n_tiles > 0x7fffffffull) return false;
    const uint64_t cap = (uint64_t)n_cu * kBpPerCU;
    uint64_t want = pl.n_tiles >= cap ? 1u : (cap + pl.n_tiles - 1u) / pl.n_tiles;
    const uint64_t most = (n_pairs + kBpMinSlab - 1u) / kBpMinSlab;
    if (want > most) want = most;
    if (want > 65535u) want = 65535u;
    pl.slab_len = (n_pairs + want - 1u) / want;
    pl.n_slabs = (uint32_t)((n_pairs + pl.slab_len - 1u) / pl.slab_len);
    return true;
}

#if defined(__HIPCC__)
// k_backproject over the plan's tiles and slabs, then — more than one slab — k_backproject_reduce
// (partial: n_slabs * nx * ny * nz floats of device memory, unused with one slab)
hipError_t launch_backproject(const BpArgs &a, const BpPlan &pl, float *partial, float *volume, hipStream_t stream);
#endif

} // namespace mtr
#endif
