// mtr_phasor_backproject.h — the arithmetic of mtr_phasor_backproject (additive, ABI 24): the phasors of a NLOS capture
// (n_pairs, F, 2) — what a phasor_hdr_film on transient_nlos_path develops — propagated back into a complex voxel volume
// (a phasor-field reconstruction).  MTR_HD, like mtr_backproject.h: the kernels of mtr_phasor_backproject.hip and the host build
// of tests/host_phasor_backproject.cpp compile this one text.
//
//   capture   mtr_backproject.h's: S sensor points, L laser points, the two offset arrays, pairs in ascending (s, l) order for
//             Confocal, Single and Exhaustive, voxel centres by bp_centre, norms by bp_norm, d = ((r1 + r2) + so[s]) + lo[l].
//   phasors   P[p, k] = sum of value * exp(-i 2 pi f_k (opl - start_opl)), the film's convention (phasor_term, mtr_core.h).
//   value     tau = d - start_opl;  V(v) = sum over p of [tau_min <= tau <= tau_max] sum over k of (w_k P[p, k]) z[p, k],
//             z[p, k] = exp(+i 2 pi f_k tau).  Pairs ascend and k ascends inside a pair; one complex f32 accumulator per voxel,
//             every term added with the four fmaf of pb_add.  A NaN or infinite tau fails the window test.
//   z         table form: the conjugate of phasor_term(freq[k], tau) — the reduction and polynomials the film accumulated P with.
//             uniform form (freq_step > 0, the caller's promise that freq[k] = freq[0] + k freq_step): the table form at every
//             k % kPbAnchor == 0, between those z <- z r (pb_rotate) with r the conjugate of phasor_term(freq_step, tau).
//   weights   NULL means ones; otherwise w_k P is formed first, two f32 products.
#ifndef MTR_PHASOR_BACKPROJECT_H
#define MTR_PHASOR_BACKPROJECT_H

#include "mtr_core.h"
#include "mtr_backproject.h"

namespace mtr {

constexpr uint32_t kPbAnchor = 16u;         // uniform form: frequencies between two evaluations of phasor_term

// mtr_phasor_backproject_desc, checked (pb_check) and with the pair count worked out
struct PbArgs {
    uint32_t capture_type, uniform;
    uint32_t S, L, F;
    float start_opl, freq_step, tau_min, tau_max;
    float vmin[3], step[3];             // step = (vmax - vmin) / n
    uint32_t nx, ny, nz;
    uint64_t n_pairs;                   // S (Confocal, Single) or S * L (Exhaustive): the rows of `phasors`
    const float *sensor_points, *laser_points, *sensor_offset, *laser_offset;
    const float *frequencies, *weights; // weights: NULL for ones (and for rows that are weighted already)
    const float *phasors;               // (n_pairs, F, 2)
};

// z = exp(+i 2 pi f tau): the conjugate of the film's term
MTR_HD void pb_anchor(float freq, float tau, float &zr, float &zi)
{
    float c, s;
    phasor_term(freq, tau, c, s);
    zr = c; zi = -s;
}

// z <- z r
MTR_HD void pb_rotate(float &zr, float &zi, float rr, float ri)
{
    const float nr = fmaf(zr, rr, -(zi * ri)), ni = fmaf(zr, ri, zi * rr);
    zr = nr; zi = ni;
}

// acc += (a + i b) z
MTR_HD void pb_add(float &re, float &im, float a, float b, float zr, float zi)
{
    re = fmaf(a, zr, re); re = fmaf(-b, zi, re);
    im = fmaf(a, zi, im); im = fmaf(b, zr, im);
}

// (w_k P[p, k]) of one row; WEIGHTED false: the row as it is (weights NULL, or rows that are weighted already)
template <bool WEIGHTED>
MTR_HD void pb_value(const float *row, const float *weights, uint32_t k, float &a, float &b)
{
    a = row[2u * k]; b = row[2u * k + 1u];
    if (WEIGHTED) { const float w = weights[k]; a = w * a; b = w * b; }
}

// one frequency of the uniform form between two anchors: z <- z r, acc += (w_k P[p, k]) z
template <bool WEIGHTED>
MTR_HD void pb_step(const float *row, const float *weights, uint32_t k, float &zr, float &zi, float rr, float ri, float &re, float &im)
{
    float va, vb;
    pb_rotate(zr, zi, rr, ri);
    pb_value<WEIGHTED>(row, weights, k, va, vb);
    pb_add(re, im, va, vb, zr, zi);
}

// the F terms of one pair at tau added to (re, im), k ascending
template <bool UNIFORM, bool WEIGHTED>
MTR_HD void pb_pair(const PbArgs &a, const float *row, float tau, float &re, float &im)
{
    float va, vb, zr, zi;
    if (!UNIFORM) {
        for (uint32_t k = 0; k < a.F; ++k) {
            pb_anchor(a.frequencies[k], tau, zr, zi);
            pb_value<WEIGHTED>(row, a.weights, k, va, vb);
            pb_add(re, im, va, vb, zr, zi);
        }
        return;
    }
    float rr, ri;
    pb_anchor(a.freq_step, tau, rr, ri);
    for (uint32_t k0 = 0; k0 < a.F; k0 += kPbAnchor) {
        pb_anchor(a.frequencies[k0], tau, zr, zi);
        pb_value<WEIGHTED>(row, a.weights, k0, va, vb);
        pb_add(re, im, va, vb, zr, zi);
        if (a.F - k0 >= kPbAnchor) {                        // a whole block: fifteen rotations, unrolled on the device
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (uint32_t j = 1u; j < kPbAnchor; ++j) pb_step<WEIGHTED>(row, a.weights, k0 + j, zr, zi, rr, ri, re, im);
        } else {                                            // the ragged last block: four at a time (one read of the row), then singly
            uint32_t k = k0 + 1u;
            for (; k + 4u <= a.F; k += 4u) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (uint32_t j = 0u; j < 4u; ++j) pb_step<WEIGHTED>(row, a.weights, k + j, zr, zi, rr, ri, re, im);
            }
            for (; k < a.F; ++k) pb_step<WEIGHTED>(row, a.weights, k, zr, zi, rr, ri, re, im);
        }
    }
}

// the sum of voxel (ix, iy, iz) over the pairs [p0, p1) of the capture's rows, ascending
template <uint32_t CAPTURE, bool UNIFORM, bool WEIGHTED>
MTR_HD void pb_voxel(const PbArgs &a, uint32_t ix, uint32_t iy, uint32_t iz, uint64_t p0, uint64_t p1, float &re, float &im)
{
    const float vx = bp_centre(a.vmin[0], a.step[0], ix), vy = bp_centre(a.vmin[1], a.step[1], iy), vz = bp_centre(a.vmin[2], a.step[2], iz);
    uint64_t s = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? p0 / a.L : p0;
    uint32_t l = (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) ? (uint32_t)(p0 - s * a.L) : 0u;
    re = 0.0f; im = 0.0f;
    for (uint64_t p = p0; p < p1; ++p) {
        const float *ps = a.sensor_points + (size_t)s * 3u;
        const float r1 = bp_norm(ps[0] - vx, ps[1] - vy, ps[2] - vz);
        float r2 = r1, lo;                                  // Confocal: P_l = P_s (mtr_backproject.h, bp_voxel)
        if (CAPTURE == MTR_CAPTURE_CONFOCAL) lo = a.laser_offset[(size_t)s];
        else {
            const float *pl = a.laser_points + (size_t)l * 3u;
            r2 = bp_norm(vx - pl[0], vy - pl[1], vz - pl[2]);
            lo = a.laser_offset[(size_t)l];
        }
        const float d = ((r1 + r2) + a.sensor_offset[(size_t)s]) + lo;
        const float tau = d - a.start_opl;
        if (tau >= a.tau_min && tau <= a.tau_max)           // (false for a NaN; an infinite tau is outside every finite bound)
            pb_pair<UNIFORM, WEIGHTED>(a, a.phasors + (size_t)p * a.F * 2u, tau, re, im);
        if (CAPTURE == MTR_CAPTURE_EXHAUSTIVE) { if (++l == a.L) { l = 0u; ++s; } }
        else ++s;
    }
}

// MTR_ERR_INVALID's cases of mtr_phasor_backproject: the message, or NULL for a description that can run
inline const char *pb_check(const mtr_phasor_backproject_desc *d, const float *phasors, const float *volume)
{
    if (!d || !phasors || !volume) return "NULL argument";
    if ((((uintptr_t)phasors) | ((uintptr_t)volume)) & 7u) return "phasors and volume are (Re, Im) pairs, 8-byte aligned";
    if (!d->sensor_points || !d->laser_points || !d->sensor_offset || !d->laser_offset) return "NULL point or offset array";
    if (!d->frequencies) return "NULL frequency table";
    if (d->capture_type != MTR_CAPTURE_SINGLE && d->capture_type != MTR_CAPTURE_CONFOCAL && d->capture_type != MTR_CAPTURE_EXHAUSTIVE)
        return "unknown capture type";
    if (d->n_sensor == 0u || d->n_laser == 0u || d->n_freq == 0u) return "a capture of zero size";
    if (d->nx == 0u || d->ny == 0u || d->nz == 0u) return "a volume of zero size";
    if (d->capture_type == MTR_CAPTURE_CONFOCAL && d->n_laser != d->n_sensor) return "a Confocal capture has one laser point per sensor point";
    if (d->capture_type == MTR_CAPTURE_SINGLE && d->n_laser != 1u) return "a Single capture has one laser point";
    if (!(fabsf(d->start_opl) <= 3.402823466e+38f)) return "start_opl must be finite";
    if (!(d->tau_min <= d->tau_max)) return "tau_min <= tau_max is required (neither a NaN)";
    if (!(d->freq_step >= 0.0f)) return "freq_step must be 0 (a table) or positive (a uniform table)";
    for (int k = 0; k < 3; ++k)
        if (!(d->volume_max[k] > d->volume_min[k]) || !(fabsf(d->volume_max[k] - d->volume_min[k]) <= 3.402823466e+38f)) return "an empty volume box";
    return nullptr;
}

inline PbArgs pb_args(const mtr_phasor_backproject_desc &d, const float *phasors)
{
    PbArgs a{};
    a.capture_type = d.capture_type; a.uniform = d.freq_step > 0.0f ? 1u : 0u;
    a.S = d.n_sensor; a.L = d.n_laser; a.F = d.n_freq;
    a.start_opl = d.start_opl; a.freq_step = d.freq_step; a.tau_min = d.tau_min; a.tau_max = d.tau_max;
    const uint32_t n[3] = { d.nx, d.ny, d.nz };
    for (int k = 0; k < 3; ++k) { a.vmin[k] = d.volume_min[k]; a.step[k] = (d.volume_max[k] - d.volume_min[k]) / (float)n[k]; }
    a.nx = d.nx; a.ny = d.ny; a.nz = d.nz;
    a.n_pairs = d.capture_type == MTR_CAPTURE_EXHAUSTIVE ? (uint64_t)d.n_sensor * d.n_laser : (uint64_t)d.n_sensor;
    a.sensor_points = d.sensor_points; a.laser_points = d.laser_points; a.sensor_offset = d.sensor_offset; a.laser_offset = d.laser_offset;
    a.frequencies = d.frequencies; a.weights = d.weights;
    a.phasors = phasors;
    return a;
}

// floats of device workspace a call needs: the weighted rows (weights given) and the slabs' complex planes (more than one slab)
inline size_t pb_weighted_floats(const PbArgs &a) { return a.weights ? (size_t)a.n_pairs * a.F * 2u : 0u; }
inline size_t pb_plane_floats(const PbArgs &a, const BpPlan &pl) { return pl.n_slabs > 1u ? (size_t)pl.n_slabs * a.nx * a.ny * a.nz * 2u : 0u; }

#if defined(__HIPCC__)
// weights given: k_pb_weight writes w_k P into `work`; k_phasor_backproject over the plan's tiles and slabs; then — more than one
// slab — k_pb_reduce.  work: pb_weighted_floats + pb_plane_floats floats of device memory, in that order.
hipError_t launch_phasor_backproject(const PbArgs &a, const BpPlan &pl, float *work, float *volume, hipStream_t stream);
#endif

} // namespace mtr
#endif
