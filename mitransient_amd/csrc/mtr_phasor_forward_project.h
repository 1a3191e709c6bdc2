// mtr_phasor_forward_project.h — the arithmetic of mtr_phasor_forward_project (additive, ABI 24): the conjugate transpose of
// mtr_phasor_backproject, a complex voxel volume (nz, ny, nx, 2) turned into the phasors (n_pairs, F, 2) it would produce — the
// forward model of a phasor-field reconstruction and the gradient of one.  MTR_HD over mtr_phasor_backproject.h: the kernels of
// mtr_phasor_forward_project.hip and the host build of tests/host_phasor_forward_project.cpp compile this one text.
//
//   factors   mtr_phasor_backproject is V(v) = sum over p of M(v, p) sum over k of (w_k P[p, k]) z(v, p, k); this is
//             Q[p, k] = w_k sum over v of M(v, p) U(v) conj(z(v, p, k)) with the same tau (pb_voxel's expression through pf_tau),
//             the same window test and the same z: pb_anchor at freq[k] (table form), or pb_anchor at every k % kPbAnchor == 0 and
//             pb_rotate by pb_anchor(freq_step, tau) in between (uniform form).  No second way of computing exp: with one
//             description the two calls are exact conjugate transposes up to the order of their f32 sums.
//   blocks    the frequencies are walked in blocks of kPbAnchor = 16, so a block starts at an anchor by construction; a block's
//             sums are 16 complex f32 accumulators, every term added with the four fmaf of pf_add.
//   order     the host build adds the voxels in ascending linear order (ix fastest).  The kernel gives every thread a fixed
//             ascending subset, adds the threads with a fixed tree and the slabs in slab order: the same call gives the same bits
//             (no float atomics), which differ from the host build's by the order of the f32 sums only.
//   weights   NULL means ones; otherwise w_k multiplies the finished sum of (p, k) where it is stored, two f32 products.
#ifndef MTR_PHASOR_FORWARD_PROJECT_H
#define MTR_PHASOR_FORWARD_PROJECT_H

#include "mtr_phasor_backproject.h"

namespace mtr {

// q += u conj(z)
MTR_HD void pf_add(float &qr, float &qi, float ur, float ui, float zr, float zi)
{
    qr = fmaf(ur, zr, qr); qr = fmaf(ui, zi, qr);
    qi = fmaf(ui, zr, qi); qi = fmaf(-ur, zi, qi);
}

// the scan-point record of row p: what tau needs beside the voxel
struct PfRow { float ps[3], pl[3], so, lo; };

template <uint32_t CAPTURE>
MTR_HD PfRow pf_row(const PbArgs &a, uint64_t p)
{
    const uint64_t s = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? p / a.L : p;
    const uint64_t l = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? p - s * a.L : (CAPTURE == MTR_CAPTURE_CONFOCAL ? s : 0u);
    PfRow r;
    for (int k = 0; k < 3; ++k) { r.ps[k] = a.sensor_points[(size_t)s * 3u + k]; r.pl[k] = a.laser_points[(size_t)l * 3u + k]; }
    r.so = a.sensor_offset[(size_t)s]; r.lo = a.laser_offset[(size_t)l];
    return r;
}

// tau of (voxel centre, row): pb_voxel's expression, the same bits (Confocal: r2 = r1, laser_offset[s])
template <uint32_t CAPTURE>
MTR_HD float pf_tau(const PfRow &r, float start_opl, float vx, float vy, float vz)
{
    const float r1 = bp_norm(r.ps[0] - vx, r.ps[1] - vy, r.ps[2] - vz);
    float r2 = r1;
    if (CAPTURE != MTR_CAPTURE_CONFOCAL) r2 = bp_norm(vx - r.pl[0], vy - r.pl[1], vz - r.pl[2]);
    const float d = ((r1 + r2) + r.so) + r.lo;
    return d - start_opl;
}

// One voxel's terms of one frequency block: q[j] += u conj(z(v, p, k0 + j)) for j < nk, where the window holds.  fk: the block's
// frequencies (table form reads fk[0 .. nk), uniform form fk[0] alone).  FULL promises nk == kPbAnchor (the loops unroll, the
// accumulators are registers on the device).
template <uint32_t CAPTURE, bool UNIFORM, bool FULL>
MTR_HD void pf_voxel(const PfRow &r, float start_opl, float freq_step, float tau_min, float tau_max, const float *fk, uint32_t nk,
                     float vx, float vy, float vz, float ur, float ui, float *qr, float *qi)
{
    const float tau = pf_tau<CAPTURE>(r, start_opl, vx, vy, vz);
    if (!(tau >= tau_min && tau <= tau_max)) return;            // (false for a NaN; an infinite tau is outside every finite bound)
    float zr, zi;
    if (UNIFORM) {
        float rr, ri;
        pb_anchor(freq_step, tau, rr, ri);
        pb_anchor(fk[0], tau, zr, zi);
        pf_add(qr[0], qi[0], ur, ui, zr, zi);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 1u; j < kPbAnchor; ++j) {
            if (FULL || j < nk) {                                 // (a guard, not a break: the loop unrolls whole either way)
                pb_rotate(zr, zi, rr, ri);
                pf_add(qr[j], qi[j], ur, ui, zr, zi);
            }
        }
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 0u; j < kPbAnchor; ++j) {
            if (FULL || j < nk) {
                pb_anchor(fk[j], tau, zr, zi);
                pf_add(qr[j], qi[j], ur, ui, zr, zi);
            }
        }
    }
}

// the finished sum of (p, k) as it is stored
MTR_HD void pf_store(float *dst, float qr, float qi, const float *weights, uint32_t k)
{
    if (weights) { const float w = weights[k]; qr = w * qr; qi = w * qi; }
    dst[0] = qr; dst[1] = qi;
}

// MTR_ERR_INVALID's cases of mtr_phasor_forward_project: pb_check's with the roles of the two tensors swapped (both 8-byte aligned)
inline const char *pf_check(const mtr_phasor_backproject_desc *d, const float *volume, const float *phasors)
{
    return pb_check(d, phasors, volume);
}

// The split of a call over workgroups: one workgroup per (row, block of kPbAnchor frequencies, slab of voxels).  Rows x blocks
// normally fill the device; only when they cannot (a few scan points against many voxels) the voxels are cut into n_slabs contiguous
// ranges of slab_len (linear index order), each summed into its own (rows, F, 2) plane of the workspace and the planes added in
// slab order.  The planes never take more than kPfPlaneCap bytes: fewer slabs are used instead.
constexpr uint32_t kPfBlock = 256u;
constexpr uint32_t kPfMinSlab = 2048u;                                 // voxels: a slab no shorter than this (8 per thread)
constexpr uint32_t kPfPerCU = 4u;                                      // workgroups wanted per compute unit
constexpr uint64_t kPfPlaneCap = 256ull << 20;                         // bytes of n_slabs * rows * F * 8
struct PfPlan { uint32_t n_blocks, n_slabs; uint64_t slab_len, n_groups; };

inline bool pf_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, uint32_t F, int n_cu, PfPlan &pl)
{
    pl = PfPlan{};
    if (!nx || !ny || !nz || !n_pairs || !F || n_cu <= 0) return false;
    const uint64_t n_vox = (uint64_t)nx * ny * nz;
    if (n_vox > 0x7fffffffull || n_pairs > 0x7fffffffull) return false;     // (the kernel's voxel index is 32-bit; grid.x)
    pl.n_blocks = (F - 1u) / kPbAnchor + 1u;
    pl.n_groups = n_pairs * pl.n_blocks;
    if (pl.n_groups > 0x7fffffffull) return false;                     // (grid.x)
    const uint64_t cap = (uint64_t)n_cu * kPfPerCU;
    uint64_t want = pl.n_groups >= cap ? 1u : (cap + pl.n_groups - 1u) / pl.n_groups;
    const uint64_t most = (n_vox + kPfMinSlab - 1u) / kPfMinSlab;
    if (want > most) want = most;
    const uint64_t plane = n_pairs * F * 2u * sizeof(float);
    const uint64_t fit = kPfPlaneCap / plane;                          // planes the cap has room for (0: none, one slab)
    if (want > fit) want = fit;
    if (want > 65535u) want = 65535u;                                  // (grid.y)
    if (want < 1u) want = 1u;
    pl.slab_len = (n_vox + want - 1u) / want;
    pl.n_slabs = (uint32_t)((n_vox + pl.slab_len - 1u) / pl.slab_len);
    return true;
}

// floats of device workspace a call needs: the slabs' planes (more than one slab)
inline size_t pf_plane_floats(const PbArgs &a, const PfPlan &pl) { return pl.n_slabs > 1u ? (size_t)pl.n_slabs * a.n_pairs * a.F * 2u : 0u; }

#if defined(__HIPCC__)
// k_phasor_forward_project over the plan's rows, blocks and slabs, then — more than one slab — k_pf_reduce
// (planes: pf_plane_floats floats of device memory, unused with one slab)
hipError_t launch_phasor_forward_project(const PbArgs &a, const PfPlan &pl, const float *volume, float *planes, float *phasors, hipStream_t stream);
#endif

} // namespace mtr
#endif
