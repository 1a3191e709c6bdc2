// mtr_kat.h — known-answer harness of mtr_core.h (TEST HOOK of the library, outside the C ABI of include/mitransient_amd.h).
//
// One element of one family: reads element i of flat input planes, calls ONE mtr_core.h function, stores the raw result words to
// element i of the output planes.  The same text is compiled for the device (mtr_kat.hip: one kernel per family, built with both of
// the library's flag sets) and for the host (tests/host_harness.cpp: a plain loop), so that tests/test_gpu_kat.py compares nothing
// but how each side compiles the header: every output word, bit for bit.
//
// Layout (all families below): plane k of `in` / `out` is words [k * n, (k + 1) * n); floats travel as their bit patterns.
#pragma once
#include "mtr_core.h"

namespace mtr {
namespace kat {

MTR_HD float ldf(const uint32_t *in, uint64_t n, uint32_t k, uint64_t i) { return bitsf(in[k * n + i]); }
MTR_HD void stf(uint32_t *out, uint64_t n, uint32_t k, uint64_t i, float v) { out[k * n + i] = fbits(v); }
MTR_HD void st3(uint32_t *out, uint64_t n, uint32_t k, uint64_t i, f3 v) { stf(out, n, k, i, v.x); stf(out, n, k + 1, i, v.y); stf(out, n, k + 2, i, v.z); }
MTR_HD f3 ld3p(const uint32_t *in, uint64_t n, uint32_t k, uint64_t i) { return mk(ldf(in, n, k, i), ldf(in, n, k + 1, i), ldf(in, n, k + 2, i)); }

// which: 0 sincos_quarter x -> (s, c); 1 sincos_2pi u -> (s, c); 2 asin_half x -> y; 3 acos_f32 x -> y; 4 phasor_term (freq, opl) -> (c, s)
MTR_HD void trig(int which, uint64_t n, uint64_t i, const uint32_t *in, uint32_t *out)
{
    const float x = ldf(in, n, 0, i);
    float a = 0.0f, b = 0.0f;
    if (which == 0) { sincos_quarter(x, a, b); stf(out, n, 0, i, a); stf(out, n, 1, i, b); }
    else if (which == 1) { sincos_2pi(x, a, b); stf(out, n, 0, i, a); stf(out, n, 1, i, b); }
    else if (which == 2) stf(out, n, 0, i, asin_half(x));
    else if (which == 3) stf(out, n, 0, i, acos_f32(x));
    else { phasor_term(x, ldf(in, n, 1, i), a, b); stf(out, n, 0, i, a); stf(out, n, 1, i, b); }
}

// which: 0 concentric_disk (u1, u2) -> (px, py); 1 cosine_hemisphere (u1, u2) -> d; 2 coordinate_system n -> (s, t);
// 3 to_local_about (n, v) -> l; 4 sphere_dir_encode n -> (u, v); 5 sphere_dir_decode (u, v) -> n; 6 unit_z l -> z;
// 7 safe_rcp x -> r; 8 mis_weight (a, b) -> w
MTR_HD void warps(int which, uint64_t n, uint64_t i, const uint32_t *in, uint32_t *out)
{
    if (which == 0) { float px, py; concentric_disk(ldf(in, n, 0, i), ldf(in, n, 1, i), px, py); stf(out, n, 0, i, px); stf(out, n, 1, i, py); }
    else if (which == 1) st3(out, n, 0, i, cosine_hemisphere(ldf(in, n, 0, i), ldf(in, n, 1, i)));
    else if (which == 2) { f3 s, t; coordinate_system(ld3p(in, n, 0, i), s, t); st3(out, n, 0, i, s); st3(out, n, 3, i, t); }
    else if (which == 3) st3(out, n, 0, i, to_local_about(ld3p(in, n, 0, i), ld3p(in, n, 3, i)));
    else if (which == 4) { float u, v; sphere_dir_encode(ld3p(in, n, 0, i), u, v); stf(out, n, 0, i, u); stf(out, n, 1, i, v); }
    else if (which == 5) st3(out, n, 0, i, sphere_dir_decode(ldf(in, n, 0, i), ldf(in, n, 1, i)));
    else if (which == 6) stf(out, n, 0, i, unit_z(ld3p(in, n, 0, i)));
    else if (which == 7) stf(out, n, 0, i, safe_rcp(ldf(in, n, 0, i)));
    else stf(out, n, 0, i, mis_weight(ldf(in, n, 0, i), ldf(in, n, 1, i)));
}

// which: 0 fresnel_conductor (ci, eta, k) -> r; 1 fresnel_dielectric (ci, eta) -> (r, cos_t, eta_it, eta_ti)
MTR_HD void fresnel(int which, uint64_t n, uint64_t i, const uint32_t *in, uint32_t *out)
{
    if (which == 0) stf(out, n, 0, i, fresnel_conductor(ldf(in, n, 0, i), ldf(in, n, 1, i), ldf(in, n, 2, i)));
    else {
        float r, ct, eit, eti;
        fresnel_dielectric(ldf(in, n, 0, i), ldf(in, n, 1, i), r, ct, eit, eti);
        stf(out, n, 0, i, r); stf(out, n, 1, i, ct); stf(out, n, 2, i, eit); stf(out, n, 3, i, eti);
    }
}

// (seed, lane, flags) -> 8 x rng_u32, then 8 x rng_f32 of the same stream [0..16), tea4(seed, lane) [16, 17], rng_inc_of [18, 19],
// rng_seed's (state, inc) before the first draw [20..24); 64-bit values as (low, high)
constexpr uint32_t kRngOut = 24;
MTR_HD void rng(uint64_t n, uint64_t i, const uint32_t *in, uint32_t *out)
{
    const uint32_t seed = in[i], lane = in[n + i], flags = in[2 * n + i];
    Rng r = rng_seed(seed, lane, flags);
    out[20 * n + i] = (uint32_t)r.state; out[21 * n + i] = (uint32_t)(r.state >> 32);
    out[22 * n + i] = (uint32_t)r.inc; out[23 * n + i] = (uint32_t)(r.inc >> 32);
    for (uint32_t k = 0; k < 8; ++k) out[k * n + i] = rng_u32(r);
    for (uint32_t k = 8; k < 16; ++k) stf(out, n, k, i, rng_f32(r));
    uint32_t v0 = seed, v1 = lane;
    tea4(v0, v1);
    out[16 * n + i] = v0; out[17 * n + i] = v1;
    const uint64_t inc = rng_inc_of(seed, lane, flags);
    out[18 * n + i] = (uint32_t)inc; out[19 * n + i] = (uint32_t)(inc >> 32);
}

// (opl, laser) -> (film_bin, film_row_bin) of a film with the given constants (film_bin reads n_freq as a flag alone)
MTR_HD Film film_of(float start_opl, float bin_width, uint32_t tbins, uint32_t lasers, uint32_t n_freq)
{
    Film f{};
    f.start_opl = start_opl; f.bin_width = bin_width; f.tbins = tbins; f.lasers = lasers; f.n_freq = n_freq;
    f.bins = tbins * lasers; f.freq = nullptr;
    return f;
}
MTR_HD void film(const Film &f, uint64_t n, uint64_t i, const uint32_t *in, uint32_t *out)
{
    const float opl = ldf(in, n, 0, i);
    out[i] = (uint32_t)film_bin(f, opl);
    out[n + i] = (uint32_t)film_row_bin(f, opl, in[n + i]);
}

// pairs a, b, c (planes a.x a.y b.x b.y c.x c.y) -> mul2, sub2, add2, fma2 as <true> [0..8) and as <false> [8..16), each (x, y).
// On the host both are the plain form.
constexpr uint32_t kPairsOut = 16;
template <bool PK> MTR_HD void pairs_form(uint64_t n, uint64_t i, f2 a, f2 b, f2 c, uint32_t k, uint32_t *out)
{
    const f2 m = mul2<PK>(a, b), s = sub2<PK>(a, b), d = add2<PK>(a, b), f = fma2<PK>(a, b, c);
    stf(out, n, k, i, m.x); stf(out, n, k + 1, i, m.y); stf(out, n, k + 2, i, s.x); stf(out, n, k + 3, i, s.y);
    stf(out, n, k + 4, i, d.x); stf(out, n, k + 5, i, d.y); stf(out, n, k + 6, i, f.x); stf(out, n, k + 7, i, f.y);
}
MTR_HD void pairs(uint64_t n, uint64_t i, const uint32_t *in, uint32_t *out)
{
    const f2 a{ ldf(in, n, 0, i), ldf(in, n, 1, i) }, b{ ldf(in, n, 2, i), ldf(in, n, 3, i) }, c{ ldf(in, n, 4, i), ldf(in, n, 5, i) };
    pairs_form<true>(n, i, a, b, c, 0, out);
    pairs_form<false>(n, i, a, b, c, 8, out);
}

// the entries tests/host_harness.cpp already had, one element each, in ITS layout (arrays of structures)
MTR_HD float special(int which, float x) { return which == 0 ? mtr_expf(x) : which == 1 ? mtr_logf(x) : which == 2 ? mtr_erff(x) : mtr_erfinvf(x); }
MTR_HD void bsdf_eval_pdf(const mtr_material &m, uint64_t i, const float *wi3, const float *wo3, float *val3, float *pdf)
{
    f3 wi = mk(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), wo = mk(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);
    f3 v = mk(0, 0, 0); float p = 0.0f;
    if ((m.flags & MTR_MAT_TWOSIDED) && wi.z < 0.0f) { wi.z = -wi.z; wo.z = -wo.z; }
    if (bsdf_is_rough(m.type)) rough_eval_pdf(m, mk(m.a[0], m.a[1], m.a[2]), wi, wo, v, p);
    else if (m.type == MTR_BSDF_DIFFUSE && wi.z > 0.0f && wo.z > 0.0f) {
        p = kInvPi * wo.z; v = mk((m.a[0] * kInvPi) * wo.z, (m.a[1] * kInvPi) * wo.z, (m.a[2] * kInvPi) * wo.z);
    }
    val3[3 * i] = v.x; val3[3 * i + 1] = v.y; val3[3 * i + 2] = v.z; pdf[i] = p;
}
MTR_HD void bsdf_sample_one(const mtr_material &m, uint64_t i, const float *wi3, const float *u1, const float *ua, const float *ub,
                            float *wo3, float *pdf, float *w3)
{
    const BsdfSample bs = bsdf_sample<true>(m, mk(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), u1[i], ua[i], ub[i], mk(m.a[0], m.a[1], m.a[2]));
    wo3[3 * i] = bs.wo.x; wo3[3 * i + 1] = bs.wo.y; wo3[3 * i + 2] = bs.wo.z; pdf[i] = bs.pdf;
    w3[3 * i] = bs.w.x; w3[3 * i + 1] = bs.w.y; w3[3 * i + 2] = bs.w.z;
}

}   // namespace kat
}   // namespace mtr
