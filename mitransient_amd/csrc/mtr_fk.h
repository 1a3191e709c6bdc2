// mtr_fk.h — the arithmetic of f-k migration (additive, ABI 24): a confocal capture of a planar wall migrated into a volume in
// N^3 log N (Lindell, Wetzstein, O'Toole 2019).  The two FFTs are the caller's; the three passes around them are declared here.
// MTR_HD: the kernels of mtr_fk.hip and the host build of tests/host_fk.cpp compile this one text, and under the numerics contract
// (f32 throughout, -ffp-contract=off, correctly rounded sqrtf and division, no fmaf) both give the same bits.
//
//   prepare   capture (H, W, T), shift (H, W) int32  ->  P (2H, 2W, 2T') f32, every element written.  In the low corner
//             P[y, x, k] = sqrt(max(S, 0)) ((k + 1/2) / T') with S[y, x, k] = sum over j = kq .. kq + q - 1 of Y[y, x, j - shift[y, x]],
//             the terms inside [0, T) only, added in increasing j; zero elsewhere.
//   stolt     F (2H, 2W, T' + 1) complex64, the non-negative temporal frequencies of P's transform  ->  G (2H, 2W, 2T') complex64,
//             every element written.  With signed indices my, mx, mz and ky = my / H, kx = mx / W, kz = mz / T': for kz > 0
//             k' = sqrt((ax kx)^2 + (ay ky)^2 + kz^2), p = k' T', i0 = floor(p), w = p - i0 and
//             G = ((1 - w) F[i0] + w F[i0 + 1]) (kz / k') when i0 + 1 <= T'; zero otherwise and for kz <= 0.
//   finish    g (2H, 2W, 2T') complex64, G's inverse transform  ->  V (nz, H, W) f32, V[iz, iy, ix] = |g[iy, ix, z_begin + iz]|^2.
//
// All three keep the film's layout, depth fastest, up to the last store.  Nothing is summed across threads: the same call gives
// the same bits.
#ifndef MTR_FK_H
#define MTR_FK_H

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

struct FkArgs {
    uint32_t H, W, T, Tp, q, z0, nz;
    float ax, ay;
};

inline FkArgs fk_args(const mtr_fk_desc &d)
{
    return FkArgs{ d.height, d.width, d.temporal_bins, d.depth_bins, d.bin_factor, d.z_begin, d.nz, d.ax, d.ay };
}

// ---- prepare
// S[k] of one scan point: `row` is its T bins
MTR_HD float fk_bin_sum(const float *row, uint32_t T, int32_t shift, uint32_t q, uint32_t k)
{
    float s = 0.0f;
    const int64_t b0 = (int64_t)k * q - shift;                          // the source bin of j = kq
    for (uint32_t i = 0u; i < q; ++i) {
        const int64_t b = b0 + i;
        if (b >= 0 && b < (int64_t)T) s += row[b];
    }
    return s;
}

MTR_HD float fk_psi(float s, uint32_t k, uint32_t Tp)
{
    return sqrtf(s > 0.0f ? s : 0.0f) * (((float)k + 0.5f) / (float)Tp);
}

// element (row r of 2H x 2W, depth k of 2T') of P
MTR_HD float fk_prepare_at(const FkArgs &a, const float *capture, const int32_t *shift, uint32_t r, uint32_t k)
{
    const uint32_t y = r / (2u * a.W), x = r - y * (2u * a.W);                        // (2H 2W < 2^32: fk_check)
    if (y >= a.H || x >= a.W || k >= a.Tp) return 0.0f;
    const uint64_t s = (uint64_t)y * a.W + x;
    return fk_psi(fk_bin_sum(capture + s * a.T, a.T, shift[s], a.q, k), k, a.Tp);
}

// ---- stolt
// signed FFT index of position i on an axis of 2n points, over n: the axis' frequency in cycles per sample pair
MTR_HD float fk_kappa(uint32_t i, uint32_t n)
{
    const float m = i < n ? (float)i : -(float)(2u * n - i);
    return m / (float)n;
}

// (ax kx)^2 + (ay ky)^2 of a row (iy, ix) of the spectrum
MTR_HD float fk_lateral(const FkArgs &a, uint32_t iy, uint32_t ix)
{
    const float u = a.ax * fk_kappa(ix, a.W), v = a.ay * fk_kappa(iy, a.H);
    return u * u + v * v;
}

// Where output depth index oz of a row reads: false when G is zero there (kz <= 0, or the tap pair leaves the half spectrum)
MTR_HD bool fk_tap(uint32_t Tp, float lateral, uint32_t oz, uint32_t &i0, float &w, float &jac)
{
    if (oz == 0u || oz >= Tp) return false;                             // kz <= 0
    const float kz = (float)oz / (float)Tp;
    const float kp = sqrtf(lateral + kz * kz);
    const float p = kp * (float)Tp;
    const float f = floorf(p);
    if (!(f + 1.0f <= (float)Tp)) return false;                         // (also a NaN)
    i0 = (uint32_t)f; w = p - f; jac = kz / kp;
    return true;
}

MTR_HD float fk_mix(float f0, float f1, float w, float jac) { return ((1.0f - w) * f0 + w * f1) * jac; }

// ---- finish
MTR_HD float fk_power(float re, float im) { return re * re + im * im; }

// MTR_ERR_INVALID's cases, shared by the three entry points
inline const char *fk_check(const mtr_fk_desc *d, const void *src, const void *dst)
{
    if (!d || !src || !dst) return "NULL argument";
    if (d->height < 2u || d->width < 2u || d->temporal_bins == 0u || d->depth_bins == 0u || d->nz == 0u) return "a capture or a volume of zero size";
    if (d->bin_factor == 0u) return "bin_factor must be at least 1";
    if (d->height > 0x7fffu || d->width > 0x7fffu || d->depth_bins > 0x3fffffffu) return "the scan or the depth grid is too large for one call";
    if ((uint64_t)d->z_begin + d->nz > d->depth_bins) return "the depth rows leave the depth grid";
    if (!(d->ax > 0.0f) || !(d->ay > 0.0f) || !(d->ax <= 3.402823466e+38f) || !(d->ay <= 3.402823466e+38f)) return "ax and ay must be positive and finite";
    if (((uintptr_t)src | (uintptr_t)dst) & 15u) return "the tensors must be 16-byte aligned";
    return nullptr;
}

constexpr uint32_t kFkBlock = 256u;
constexpr uint32_t kFkStage = 4096u;          // complex elements of a spectrum row k_fk_stolt keeps in LDS (32 KiB); longer rows are read in place
constexpr uint32_t kFkTile = 64u;             // k_fk_finish: depth x scan-column tile

#if defined(__HIPCC__)
hipError_t launch_fk_prepare(const FkArgs &a, const float *capture, const int32_t *shift, float *padded, hipStream_t stream);
hipError_t launch_fk_stolt(const FkArgs &a, const float *spectrum, float *resampled, hipStream_t stream);
hipError_t launch_fk_finish(const FkArgs &a, const float *field, float *volume, hipStream_t stream);
#endif

} // namespace mtr
#endif
