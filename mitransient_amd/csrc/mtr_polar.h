// mtr_polar.h — the per-path arithmetic of the *_mono_polarized variants: a 4x4 Mueller matrix as the path throughput,
// a Stokes vector (S0, S1, S2, S3) as the radiance.  MTR_HD: the host test build and the device compile the same code.
//
// What is restated (Mitsuba 3, the polarized branches; DESIGN.md "Polarization"):
//   mueller.h            depolarizer, rotator, stokes_basis, rotate_stokes_basis, rotate_mueller_basis,
//                        specular_reflection, specular_transmission
//   fresnel.h            fresnel_polarized (complex eta for conductors; real eta with total internal reflection)
//   SurfaceInteraction   to_world_mueller
//   conductor.cpp / roughconductor.cpp / dielectric.cpp   the `is_polarized_v<Spectrum>` branches of sample / eval
//   diffuse.cpp, area.cpp   depolarizers
//   mitransient utils.py:9-21 (beta_init), transientpath.py:140-318 (the loop; Mueller products at :207-233)
// Every in-scope emitter is a depolarizer, so a contribution is column 0 of (beta * ...) times a scalar radiance, and the path
// radiance needs 4 floats.  The path consumes the sampler exactly as path_bounce does (mtr_core.h): lane i draws the same
// directions, and on a scene of diffuse surfaces M00 of every product is the unpolarized value to the bit (every other term
// of its sums is an exact zero).
#pragma once
#include "mtr_core.h"

namespace mtr {

// ---------------------------------------------------------------- Mueller algebra
struct M44 { float m[16]; };     // row-major: m[4 * row + col]

MTR_HD M44 m44_zero() { M44 r; for (int i = 0; i < 16; ++i) r.m[i] = 0.0f; return r; }
// [mueller.h: depolarizer]
MTR_HD M44 depolarizer(float v) { M44 r = m44_zero(); r.m[0] = v; return r; }
MTR_HD M44 m44_identity() { M44 r = m44_zero(); r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.0f; return r; }
// a * b, every sum in index order ((x0 + x1) + x2) + x3 (no fma: the numerics contract)
MTR_HD M44 m44_mul(const M44 &a, const M44 &b)
{
    M44 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            r.m[4 * i + j] = ((a.m[4 * i] * b.m[j] + a.m[4 * i + 1] * b.m[4 + j]) + a.m[4 * i + 2] * b.m[8 + j]) + a.m[4 * i + 3] * b.m[12 + j];
    return r;
}
MTR_HD M44 m44_scale(M44 a, float s) { for (int i = 0; i < 16; ++i) a.m[i] = a.m[i] * s; return a; }

// [mueller.h: rotator(theta)] by (cos 2 theta, sin 2 theta): rows / columns 1 and 2 of the identity rotated
//   ( 1  0  0  0 )
//   ( 0  c  s  0 )
//   ( 0 -s  c  0 )
//   ( 0  0  0  1 )
MTR_HD M44 rotator_cs(float c2, float s2)
{
    M44 r = m44_identity();
    r.m[5] = c2; r.m[6] = s2; r.m[9] = -s2; r.m[10] = c2;
    return r;
}

// [vector.h: coordinate_system(n).first] (Duff et al. 2017) — [mueller.h: stokes_basis(w)]
MTR_HD f3 stokes_basis(f3 n)
{
    const float sign = n.z >= 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + n.z), b = (n.x * n.y) * a;
    return mk(1.0f + sign * ((n.x * n.x) * a), sign * b, -(sign * n.x));
}

// [mueller.h: rotate_stokes_basis(forward, current, target)] = rotator(theta), theta the angle from current to target,
// negative when dot(forward, cross(current, target)) < 0.  The rotator needs cos 2 theta and sin 2 theta only: with unit
// bases perpendicular to forward, cos theta = dot(current, target) and sin theta = dot(forward, cross(current, target)), so
// no angle is formed (mitsuba: unit_angle, then sincos(2 theta)).  The pair is normalised, so that the rotator stays orthogonal.
MTR_HD void rotate_stokes_basis_cs(f3 fwd, f3 cur, f3 tgt, float &c2, float &s2)
{
    const f3 cn = normalize(cur), tn = normalize(tgt);
    const float c = dot(cn, tn), s = dot(fwd, cross(cn, tn));
    const float r = c * c + s * s;
    c2 = (c * c - s * s) / r; s2 = (2.0f * s * c) / r;
}

// R_out * M * transpose(R_in) with R = rotator(c, s): only rows 1, 2 (left factor) and columns 1, 2 (right factor) mix —
// bit for bit the general product m44_mul(m44_mul(R_out, M), transpose(R_in)), whose other terms are exact zeros
MTR_HD M44 rotate_mueller_cs(M44 M, float ci, float si, float co, float so)
{
    for (int j = 0; j < 4; ++j) {           // R_out * M: row1' = c row1 + s row2, row2' = -s row1 + c row2
        const float r1 = M.m[4 + j], r2 = M.m[8 + j];
        M.m[4 + j] = co * r1 + so * r2;
        M.m[8 + j] = (-so) * r1 + co * r2;
    }
    for (int i = 0; i < 4; ++i) {           // (.) * R_in^T: col1' = c col1 + s col2, col2' = -s col1 + c col2
        const float c1 = M.m[4 * i + 1], c2 = M.m[4 * i + 2];
        M.m[4 * i + 1] = ci * c1 + si * c2;
        M.m[4 * i + 2] = (-si) * c1 + ci * c2;
    }
    return M;
}
// [mueller.h: rotate_mueller_basis(M, in_forward, in_current, in_target, out_forward, out_current, out_target)]
MTR_HD M44 rotate_mueller_basis(const M44 &M, f3 in_fwd, f3 in_cur, f3 in_tgt, f3 out_fwd, f3 out_cur, f3 out_tgt)
{
    float ci, si, co, so;
    rotate_stokes_basis_cs(in_fwd, in_cur, in_tgt, ci, si);
    rotate_stokes_basis_cs(out_fwd, out_cur, out_tgt, co, so);
    return rotate_mueller_cs(M, ci, si, co, so);
}

// a local direction to world space through a shading frame (SurfaceInteraction::to_world)
MTR_HD f3 frame_to_world(f3 s, f3 t, f3 n, f3 v)
{
    return mk(fmaf(n.x, v.z, fmaf(t.x, v.y, s.x * v.x)), fmaf(n.y, v.z, fmaf(t.y, v.y, s.y * v.x)), fmaf(n.z, v.z, fmaf(t.z, v.y, s.z * v.x)));
}
// [SurfaceInteraction::to_world_mueller(M, wi_local, wo_local)]: the Stokes bases of a BSDF's matrix are those of its local
// directions (stokes_basis in the local frame); rotate them onto the implicit bases of the world directions
MTR_HD M44 to_world_mueller(const M44 &M, f3 s, f3 t, f3 n, f3 wi_local, f3 wo_local)
{
    const f3 wi_w = frame_to_world(s, t, n, wi_local), wo_w = frame_to_world(s, t, n, wo_local);
    const f3 bi_w = frame_to_world(s, t, n, stokes_basis(wi_local)), bo_w = frame_to_world(s, t, n, stokes_basis(wo_local));
    return rotate_mueller_basis(M, wi_w, bi_w, stokes_basis(wi_w), wo_w, bo_w, stokes_basis(wo_w));
}

// ---------------------------------------------------------------- Fresnel Mueller matrices
// The Mueller matrix of a specular interface from the reflectances (r_s, r_p) and the phase difference delta of the s and p
// amplitudes [mueller.h: specular_reflection]:
//   ( a  b  0      0     )   a = (r_s + r_p) / 2, b = (r_s - r_p) / 2, c = sqrt(r_s r_p)
//   ( b  a  0      0     )
//   ( 0  0  c cos  c sin )
//   ( 0  0 -c sin  c cos )
MTR_HD M44 mueller_interface(float rs, float rp, float cos_d, float sin_d)
{
    M44 r = m44_zero();
    const float a = 0.5f * (rs + rp), b = 0.5f * (rs - rp), c = sqrtf(rs * rp);
    if (c == 0.0f) { cos_d = 0.0f; sin_d = 0.0f; }      // (mitsuba masks the phase where c == 0)
    r.m[0] = a; r.m[1] = b; r.m[4] = b; r.m[5] = a;
    r.m[10] = c * cos_d; r.m[11] = c * sin_d; r.m[14] = -(c * sin_d); r.m[15] = c * cos_d;
    return r;
}
// [mitsuba: sincos_arg_diff(a, b)] sin and cos of arg(a) - arg(b) from a * conj(b) (0, 0 when a product is zero)
MTR_HD void sincos_arg_diff(float ar, float ai, float br, float bi, float &sn, float &cs)
{
    const float re = ar * br + ai * bi, im = ai * br - ar * bi;
    const float n2 = re * re + im * im;
    if (!(n2 > 0.0f)) { sn = 0.0f; cs = 0.0f; return; }
    const float inv = 1.0f / sqrtf(n2);
    sn = im * inv; cs = re * inv;
}

// [mueller.h: specular_reflection(cos_theta_i, eta)] of a conductor, eta = er + i ei relative to the outside.
// r_s and r_p are those of fresnel_conductor (mtr_core.h) — same operations, so M00 IS the scalar reflectance to the bit —
// and the phase comes from the complex amplitudes of fresnel_polarized:
//   u = eta cos_t = sqrt(eta^2 - sin^2) = a + i b   (a as in fresnel_conductor, b = er ei / a)
//   a_s = (ci - u) / (ci + u),  a_p = (u - eta^2 ci) / (u + eta^2 ci)     (the p sign convention of fresnel_dielectric)
// Only arg(a_s) - arg(a_p) is needed, so each amplitude is replaced by its numerator times the conjugate denominator.
MTR_HD M44 conductor_reflection_mueller(float ci, float er, float ei)
{
    const float c2 = ci * ci, s2 = 1.0f - c2, s4 = s2 * s2;
    const float t1 = er * er - ei * ei - s2;
    const float q = t1 * t1 + 4.0f * ei * ei * er * er;
    const float a2pb2 = sqrtf(q > 0.0f ? q : 0.0f);
    const float hh = 0.5f * (a2pb2 + t1);
    const float a = sqrtf(hh > 0.0f ? hh : 0.0f);
    const float term1 = a2pb2 + c2, term2 = 2.0f * ci * a;
    const float rs = (term1 - term2) / (term1 + term2);
    const float term3 = a2pb2 * c2 + s4, term4 = term2 * s2;
    const float rp = rs * (term3 - term4) / (term3 + term4);
    // phase difference of the amplitudes
    const float hb = 0.5f * (a2pb2 - t1);
    const float b = a > 0.0f ? (er * ei) / a : sqrtf(hb > 0.0f ? hb : 0.0f);
    // a_s ~ (ci - u)(ci + conj u) = (ci^2 - |u|^2) - 2 i ci b
    const float sr = c2 - a2pb2, si = -2.0f * ci * b;
    // a_p ~ (u - v) conj(u + v), v = eta^2 ci
    const float vr = (er * er - ei * ei) * ci, vi = (2.0f * er * ei) * ci;
    const float xr = a - vr, xi = b - vi, yr = a + vr, yi = -(b + vi);        // (u - v), conj(u + v)
    const float pr = xr * yr - xi * yi, pi = xr * yi + xi * yr;
    float sn, cs;
    sincos_arg_diff(sr, si, pr, pi, sn, cs);
    return mueller_interface(rs, rp, cs, sn);
}

// [fresnel.h: fresnel_polarized(cos_theta_i, eta)] for a real eta: the complex amplitudes, total internal reflection
// included (cos_t imaginary), and the signed cosine of the transmitted direction (0 under total internal reflection).
// Outside total internal reflection a_s, a_p are those of fresnel_dielectric (mtr_core.h), operation for operation.
struct FresnelAmp { float as_r, as_i, ap_r, ap_i, cos_t, eta_it, eta_ti; bool tir; };
MTR_HD FresnelAmp fresnel_polarized(float ci, float eta)
{
    FresnelAmp f;
    const bool outside = ci >= 0.0f;
    const float rcp_eta = 1.0f / eta;
    f.eta_it = outside ? eta : rcp_eta;
    f.eta_ti = outside ? rcp_eta : eta;
    const float ct2 = fmaf(-fmaf(-ci, ci, 1.0f), f.eta_ti * f.eta_ti, 1.0f);
    const float cia = fabsf(ci);
    f.tir = ct2 < 0.0f;
    f.as_i = 0.0f; f.ap_i = 0.0f;
    if (!f.tir) {
        const float cta = sqrtf(ct2);
        f.as_r = fmaf(-f.eta_it, cta, cia) / fmaf(f.eta_it, cta, cia);
        f.ap_r = fmaf(-f.eta_it, cia, cta) / fmaf(f.eta_it, cia, cta);
        f.cos_t = sign_neg(ci) ? cta : -cta;
    } else {
        // cos_t = i q: a_s = (cia - i eta q) / (cia + i eta q), a_p = (i q - eta cia) / (i q + eta cia) — unit moduli
        const float qq = sqrtf(-ct2), x = f.eta_it * qq, y = f.eta_it * cia;
        const float ds = cia * cia + x * x, dp = qq * qq + y * y;
        f.as_r = (cia * cia - x * x) / ds; f.as_i = (-2.0f * cia * x) / ds;
        f.ap_r = (qq * qq - y * y) / dp;   f.ap_i = (2.0f * qq * y) / dp;
        f.cos_t = 0.0f;
    }
    if (eta == 1.0f) { f.as_r = f.as_i = f.ap_r = f.ap_i = 0.0f; }          // index matched
    else if (cia == 0.0f) { f.as_r = -1.0f; f.ap_r = 1.0f; f.as_i = f.ap_i = 0.0f; }   // grazing: the limit of the amplitudes
    return f;
}
// [mueller.h: specular_reflection(cos_theta_i, eta)], real eta.  r_s = a_s^2, r_p = a_p^2 outside total internal reflection
// (so M00 = fresnel_dielectric's r to the bit), 1 under it.
MTR_HD M44 dielectric_reflection_mueller(float ci, float eta)
{
    const FresnelAmp f = fresnel_polarized(ci, eta);
    float rs, rp;
    if (f.tir && eta != 1.0f && fabsf(ci) != 0.0f) { rs = 1.0f; rp = 1.0f; }
    else { rs = f.as_r * f.as_r + f.as_i * f.as_i; rp = f.ap_r * f.ap_r + f.ap_i * f.ap_i; }
    float sn, cs;
    sincos_arg_diff(f.as_r, f.as_i, f.ap_r, f.ap_i, sn, cs);
    return mueller_interface(rs, rp, cs, sn);
}
// [mueller.h: specular_transmission(cos_theta_i, eta)]: factor = -eta_it cos_t / cos_i (0 for |cos_i| <= 1e-8 and under total
// internal reflection), t_s = (Re a_s + 1)^2, t_p = ((1 - Re a_p) eta_ti)^2
//   ( a  b  0  0 )   a = factor (t_s + t_p) / 2, b = factor (t_s - t_p) / 2, c = factor sqrt(t_s t_p)
//   ( b  a  0  0 )
//   ( 0  0  c  0 )
//   ( 0  0  0  c )
MTR_HD M44 dielectric_transmission_mueller(float ci, float eta)
{
    const FresnelAmp f = fresnel_polarized(ci, eta);
    const float factor = -f.eta_it * (fabsf(ci) > 1e-8f ? f.cos_t / ci : 0.0f);
    const float asr = f.as_r + 1.0f, apr = (1.0f - f.ap_r) * f.eta_ti;
    const float ts = asr * asr, tp = apr * apr;
    M44 r = m44_zero();
    const float a = 0.5f * factor * (ts + tp), b = 0.5f * factor * (ts - tp), c = factor * sqrtf(ts * tp);
    r.m[0] = a; r.m[1] = b; r.m[4] = b; r.m[5] = a; r.m[10] = c; r.m[15] = c;
    return r;
}

// The frame rotation every polarized specular BSDF applies to its local matrix (conductor.cpp, roughconductor.cpp,
// dielectric.cpp): light arrives along -wo_hat and leaves along wi_hat (TransportMode::Radiance: wo_hat = the sampled / evaluated
// wo, wi_hat = si.wi); the matrix's s axes are perpendicular to the plane of incidence around the (micro)normal m,
// cross(m, -wo_hat) and cross(m, wi_hat) — (1, 0, 0) both when the directions are collinear with m — and are rotated onto the
// implicit Stokes bases of -wo_hat and wi_hat.
MTR_HD M44 interface_to_local(const M44 &M, f3 m, f3 wo_hat, f3 wi_hat)
{
    f3 s_in = cross(m, -wo_hat), s_out = cross(m, wi_hat);
    if (s_in.x == 0.0f && s_in.y == 0.0f && s_in.z == 0.0f) { s_in = mk(1, 0, 0); s_out = mk(1, 0, 0); }
    else if (s_out.x == 0.0f && s_out.y == 0.0f && s_out.z == 0.0f) s_out = s_in;
    return rotate_mueller_basis(M, -wo_hat, s_in, stokes_basis(-wo_hat), wi_hat, s_out, stokes_basis(wi_hat));
}

// ---------------------------------------------------------------- polarized BSDFs
// Which materials the polarized path implements: diffuse, conductor, roughconductor (GGX / Beckmann, anisotropic), dielectric,
// each optionally two-sided.  The host refuses everything else (scene.py); a material outside the set shades as a black absorber.
MTR_HD bool polar_bsdf_supported(uint32_t type)
{
    return type == MTR_BSDF_DIFFUSE || type == MTR_BSDF_CONDUCTOR || type == MTR_BSDF_ROUGHCONDUCTOR || type == MTR_BSDF_DIELECTRIC;
}

struct PolarSample { f3 wo; float pdf, eta; bool delta; M44 w; };

// BSDF::sample (local frame, Mueller weight before to_world_mueller).  Sample consumption, directions, pdfs and eta are
// those of bsdf_sample (mtr_core.h) — the scalar weights are replaced by the Mueller matrices of the polarized branches
MTR_HD PolarSample polar_bsdf_sample(const mtr_material &m, f3 wi, float u1, float ua, float ub, float albedo)
{
    PolarSample ps;
    ps.wo = mk(0, 0, 0); ps.pdf = 0.0f; ps.eta = 1.0f; ps.delta = false; ps.w = m44_zero();
    const bool flip = (m.flags & MTR_MAT_TWOSIDED) && wi.z < 0.0f;         // [twosided.cpp] the back side mirrored
    if (flip) wi.z = -wi.z;
    const float ci = wi.z;
    if (m.type == MTR_BSDF_DIFFUSE) {
        ps.wo = cosine_hemisphere(ua, ub);
        ps.pdf = kInvPi * ps.wo.z;
        if (ci > 0.0f && ps.pdf > 0.0f) ps.w = depolarizer(albedo);
    } else if (m.type == MTR_BSDF_CONDUCTOR) {
        ps.wo = mk(-wi.x, -wi.y, wi.z); ps.pdf = 1.0f; ps.delta = true;
        if (ci > 0.0f)
            ps.w = m44_scale(interface_to_local(conductor_reflection_mueller(ps.wo.z, m.a[0], m.b[0]), mk(0, 0, 1), ps.wo, wi), m.c[0]);
    } else if (m.type == MTR_BSDF_DIELECTRIC) {
        float r, ct, eit, eti;
        fresnel_dielectric(ci, m.int_ior / m.ext_ior, r, ct, eit, eti);
        const bool refl = u1 <= r;
        ps.delta = true;
        ps.pdf = refl ? r : 1.0f - r;
        const float eta = m.int_ior / m.ext_ior;
        if (refl) ps.wo = mk(-wi.x, -wi.y, wi.z);
        else { ps.wo = mk(-eti * wi.x, -eti * wi.y, ct); ps.eta = eit; }
        // [dielectric.cpp, polarized] R or T at cos(wo_hat) = cos(wo), divided by the probability of the lobe that was chosen
        M44 M = refl ? dielectric_reflection_mueller(ps.wo.z, eta) : dielectric_transmission_mueller(ps.wo.z, eta);
        M = m44_scale(M, 1.0f / ps.pdf);
        M = interface_to_local(M, mk(0, 0, 1), ps.wo, wi);
        const float k = refl ? m.c[0] : m.c2[0] * (eti * eti);             // (radiance: the solid-angle compression, as bsdf_sample)
        ps.w = m44_scale(M, k);
        if (!(ps.pdf > 0.0f)) ps.w = m44_zero();
    } else if (m.type == MTR_BSDF_ROUGHCONDUCTOR) {
        if (ci > 0.0f) {
            const bool beck = (m.flags & MTR_MAT_BECKMANN) != 0u;
            const float au = m.alpha, av = rough_alpha_v(m);
            float pdf;
            const f3 mm = ggx_sample(wi, au, av, ua, ub, pdf, beck);
            const float wim = dot(wi, mm);
            const f3 wo = mk(fmaf(mm.x, 2.0f * wim, -wi.x), fmaf(mm.y, 2.0f * wim, -wi.y), fmaf(mm.z, 2.0f * wim, -wi.z));     // reflect(wi, m)
            ps.wo = wo;
            const bool ok = (pdf != 0.0f) && (wo.z > 0.0f);
            const float g1 = mf_smith_g1(wo, mm, au, av, beck);
            ps.pdf = pdf / (4.0f * dot(wo, mm));
            if (ok) {
                // [roughconductor.cpp sample, polarized] F at dot(wo_hat, m), s axes around the microfacet normal
                const M44 F = interface_to_local(conductor_reflection_mueller(dot(wo, mm), m.a[0], m.b[0]), mm, wo, wi);
                ps.w = m44_scale(F, g1 * m.c[0]);
            }
        }
    }
    if (flip) ps.wo.z = -ps.wo.z;
    return ps;
}

// BSDF::eval_pdf for the emitter-sampling term (smooth lobes only: diffuse, roughconductor); wi, wo local, not yet flipped
MTR_HD void polar_bsdf_eval_pdf(const mtr_material &m, f3 wi, f3 wo, float albedo, M44 &val, float &pdf)
{
    val = m44_zero(); pdf = 0.0f;
    if ((m.flags & MTR_MAT_TWOSIDED) && wi.z < 0.0f) { wi.z = -wi.z; wo.z = -wo.z; }
    const float ci = wi.z, co = wo.z;
    if (!(ci > 0.0f && co > 0.0f)) return;
    if (m.type == MTR_BSDF_DIFFUSE) {
        pdf = kInvPi * co;
        val = depolarizer((albedo * kInvPi) * co);
        return;
    }
    if (m.type != MTR_BSDF_ROUGHCONDUCTOR) return;
    const f3 H = normalize(mk(wo.x + wi.x, wo.y + wi.y, wo.z + wi.z));
    const bool beck = (m.flags & MTR_MAT_BECKMANN) != 0u;
    const float au = m.alpha, av = rough_alpha_v(m);
    const float D = mf_eval(H, au, av, beck);
    const float g1i = mf_smith_g1(wi, H, au, av, beck);
    if (dot(wi, H) > 0.0f && dot(wo, H) > 0.0f) pdf = (D * g1i) / (4.0f * ci);
    if (D != 0.0f) {
        const float G = g1i * mf_smith_g1(wo, H, au, av, beck);
        const float r = (D * G) / (4.0f * ci);
        // [roughconductor.cpp eval, polarized] F at dot(wo_hat, H), s axes cross(H, -wo_hat), cross(H, wi_hat)
        val = m44_scale(interface_to_local(conductor_reflection_mueller(dot(wo, H), m.a[0], m.b[0]), H, wo, wi), r * m.c[0]);
    }
}

// ---------------------------------------------------------------- path state
// beta: the Mueller throughput; L: the Stokes radiance of the path so far.  `base` keeps everything else — ray, eta, distance,
// previous vertex, depth, the sampler — exactly as path_bounce does (its beta and L fields are unused).
struct PolarPath {
    Path base;
    M44 beta;
    float L[4];
};

// [mitransient utils.py:9-21 beta_init]: rotate the Stokes basis of -ray.d onto cross(ray.d, to_world * (0, 1, 0)), the
// camera's horizontal axis — S1 > 0 is horizontally polarized light in the image
MTR_HD M44 beta_init(const Camera &cam, f3 d)
{
    const f3 vertical = mk(cam.tw[1], cam.tw[5], cam.tw[9]);
    float c2, s2;
    rotate_stokes_basis_cs(-d, stokes_basis(-d), cross(d, vertical), c2, s2);
    return rotator_cs(c2, s2);
}

MTR_HD void polar_begin(PolarPath &p, const Camera &cam, const Film &f, const RenderConst &rc, uint32_t pixel, uint32_t s)
{
    path_begin(p.base, cam, f, rc, pixel, s);
    p.beta = beta_init(cam, p.base.ray.d);
    p.L[0] = p.L[1] = p.L[2] = p.L[3] = 0.0f;
}

// a Stokes contribution of a depolarizing emitter: column 0 of beta, each entry times mis, times the radiance
// (Le = beta * Spectrum(mis) * depolarizer(radiance), transientpath.py:172-176)
struct PolarSinkArgs { uint32_t fx, fy; bool in_film; };
template <class Sink>
MTR_HD void polar_splat(Sink &sink, const Film &film, const RenderConst &rc, const PolarSinkArgs &pa, const float v[4], float opl,
                        uint32_t depth, uint32_t kind)
{
    const float s0 = v[0] * rc.sample_scale, s1 = v[1] * rc.sample_scale, s2 = v[2] * rc.sample_scale, s3 = v[3] * rc.sample_scale;
    if (pa.in_film && (s0 != 0.0f || s1 != 0.0f || s2 != 0.0f || s3 != 0.0f)) {
        const int32_t bin = film_bin(film, opl);
        if (bin >= 0) sink.splat4(pa.fx, pa.fy, (uint32_t)bin, s0, s1, s2, s3, opl, depth, kind);
    }
}

// One whole iteration of the loop of transientpath.py:140-319 in the polarized variants: path_bounce (mtr_core.h) with
// Mueller weights.  Same traversals, the same sampler draws in the same order, the same directions, pdfs and optical path
// lengths.  unwarp_here: camera_unwarp at depth 0 from this bounce's own closest hit (as path_bounce).  Returns active_next.
template <class Stack, class Sink>
MTR_HD bool polar_bounce(PolarPath &pp, const SceneView &sc, const Film &film, const RenderConst &rc, Stack &st, Sink &sink,
                         BounceStats &stats, bool unwarp_here)
{
    Path &p = pp.base;
    const Hit h = traverse<false>(sc, p.ray.o, p.ray.d, p.ray.tmax, st);                              // :148-151
    stats.closest++;
    if (unwarp_here && p.depth == 0u && h.prim >= 0) p.dist = -h.t;
    const bool valid = h.prim >= 0;
    const float eta = p.eta;
    const bool prev_delta = p.prev_delta != 0u;
    const uint32_t n_emitters = sc.n_emitters;
    p.dist += h.t * eta;                                                                             // :154
    bool active_next = ((p.depth + 1u) < rc.max_depth) & valid;                                      // :185
    PolarSinkArgs pa;
    pa.fx = p.px - film.crop_x; pa.fy = p.py - film.crop_y;
    pa.in_film = (pa.fx < film.width) & (pa.fy < film.height);
    float u1 = rng_f32(p.rng), u2 = rng_f32(p.rng);                                                  // :193
    float Le[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, Lr[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    float opl_r = 0.0f;
    bool has_shadow = false;
    Ray shadow; shadow.o = mk(0, 0, 0); shadow.d = mk(0, 0, 1); shadow.tmax = 0.0f;
    HitCtx c;
    c.sp = mk(0, 0, 0); c.sn = mk(0, 0, 1); c.gn = mk(0, 0, 1); c.ss = mk(1, 0, 0); c.stt = mk(0, 1, 0); c.wi = mk(0, 0, 0); c.mat = 0; c.em_plus1 = 0;
    if (valid) {
        c = hit_ctx<true>(sc, p.ray.d, h);
        const mtr_material &mat = sc.mats[c.mat];
        // direct emission (:166-176)
        if (c.em_plus1 != 0u && !(rc.flags & MTR_FLAG_DISCARD_DIRECT_LIGHT)) {
            const Emitter &E = sc.ems[c.em_plus1 - 1u];
            const f3 rel = c.sp - p.prev_p;
            const float dist = sqrtf(dot(rel, rel));
            const f3 dd = rel / dist;
            float em_pdf = 0.0f;
            if (!prev_delta) {
                const float dp = dot(dd, c.sn);
                if (dp < 0.0f) {
                    const float adp = fabsf(dp);
                    em_pdf = E.inv_area * (adp != 0.0f ? (dist * dist) / adp : 0.0f);
                    if (n_emitters > 1) em_pdf *= rc.inv_n_emitters;
                }
            }
            const float mis = mis_weight(p.prev_pdf, em_pdf);
            if (c.wi.z > 0.0f)
                for (int i = 0; i < 4; ++i) Le[i] = (pp.beta.m[4 * i] * mis) * E.radiance[0];
            polar_splat(sink, film, rc, pa, Le, p.dist, p.depth, 0u);                                 // :179-180
        }
        // emitter sampling (:188-213): the smooth lobes — diffuse, roughconductor
        if (active_next && (mat.type == MTR_BSDF_DIFFUSE || mat.type == MTR_BSDF_ROUGHCONDUCTOR) && n_emitters > 0) {
            uint32_t ei = 0;
            if (n_emitters > 1) {
                const float su = u1 * rc.n_emitters_f;
                uint32_t i = (uint32_t)su;
                if (i > n_emitters - 1) i = n_emitters - 1;
                ei = i; u1 = su - (float)i;
            }
            const Emitter &E = sc.ems[ei];
            f3 ep, en;
            if (E.kind != kEmRect) mesh_sample_position(sc.samp_tris, sc.face_cdf, sc.face_pmf, E.first_tri, E.n_tris, u1, u2, ep, en, sc.samp_vn);
            else {
                const float a = fmaf(u1, 2.0f, -1.0f), b = fmaf(u2, 2.0f, -1.0f);
                ep = mk(fmaf(E.du[0], a, fmaf(E.dv[0], b, E.center[0])), fmaf(E.du[1], a, fmaf(E.dv[1], b, E.center[1])),
                        fmaf(E.du[2], a, fmaf(E.dv[2], b, E.center[2])));
                en = ld3(E.n);
            }
            f3 dd = ep - c.sp;
            const float dist2 = dot(dd, dd), dist = sqrtf(dist2);
            dd = dd / dist;
            const float dp = dot(dd, en), adp = fabsf(dp);
            const float x = dist2 / adp;
            const float pdf_dir = E.inv_area * ((fabsf(x) <= 3.402823466e+38f) ? x : 0.0f);
            if ((dp < 0.0f) & (pdf_dir != 0.0f)) {
                float emw = E.radiance[0] * (1.0f / pdf_dir), pdf = pdf_dir;          // (ld3(radiance) / pdf_dir of shade_hit: times the reciprocal)
                if (n_emitters > 1) { pdf = pdf_dir * rc.inv_n_emitters; emw = emw * rc.n_emitters_f; }
                if (pdf != 0.0f) {
                    const f3 wo = mk(dot(dd, c.ss), dot(dd, c.stt), dot(dd, c.sn));
                    const f3 so = offset_point(c.sp, c.gn, ep - c.sp);
                    const f3 sd = ep - so;
                    const float sdist = sqrtf(dot(sd, sd));
                    shadow.o = so; shadow.d = sd / sdist; shadow.tmax = sdist * (1.0f - kShadowEps);
                    has_shadow = true;
                    M44 bval; float bpdf;
                    polar_bsdf_eval_pdf(mat, c.wi, wo, mat.a[0], bval, bpdf);
                    // bsdf_value_em = si.to_world_mueller(bsdf_value_em, -wo, si.wi) (:210); a depolarizer needs no rotation
                    // (its rotated form is itself, exactly)
                    if (mat.type != MTR_BSDF_DIFFUSE) bval = to_world_mueller(bval, c.ss, c.stt, c.sn, -wo, c.wi);
                    const float mis_em = mis_weight(pdf, bpdf);
                    // Lr_dir = beta * Spectrum(mis_em) * bsdf_value_em * em_weight (:212): column 0, the emitter a depolarizer
                    for (int i = 0; i < 4; ++i) {
                        const float b0 = pp.beta.m[4 * i] * mis_em, b1 = pp.beta.m[4 * i + 1] * mis_em;
                        const float b2 = pp.beta.m[4 * i + 2] * mis_em, b3 = pp.beta.m[4 * i + 3] * mis_em;
                        Lr[i] = (((b0 * bval.m[0] + b1 * bval.m[4]) + b2 * bval.m[8]) + b3 * bval.m[12]) * emw;
                    }
                    opl_r = p.dist + dist * eta;                                                     // :217
                }
            }
        }
    }
    bool occluded = false;
    if (has_shadow) {
        stats.shadow++;
        const Hit sh = traverse<true>(sc, shadow.o, shadow.d, shadow.tmax, st);
        occluded = sh.prim >= 0;
    }
    if (has_shadow && !occluded) polar_splat(sink, film, rc, pa, Lr, opl_r, p.depth, 1u);
    else { Lr[0] = Lr[1] = Lr[2] = Lr[3] = 0.0f; }
    // BSDF sampling (:222-233)
    const float s1 = rng_f32(p.rng), s2a = rng_f32(p.rng), s2b = rng_f32(p.rng);
    const float rr_u = rng_f32(p.rng);
    PolarSample bs;
    bs.wo = mk(0, 0, 0); bs.pdf = 0.0f; bs.eta = 1.0f; bs.delta = false; bs.w = m44_zero();
    for (int i = 0; i < 4; ++i) pp.L[i] = (pp.L[i] + Le[i]) + Lr[i];                                  // :230
    bool diffuse = false;
    if (valid && active_next) {
        const mtr_material &mat = sc.mats[c.mat];
        diffuse = mat.type == MTR_BSDF_DIFFUSE;
        bs = polar_bsdf_sample(mat, c.wi, s1, s2a, s2b, mat.a[0]);
        // bsdf_weight = si.to_world_mueller(bsdf_weight, -bs.wo, si.wi) (:226)
        if (!diffuse) bs.w = to_world_mueller(bs.w, c.ss, c.stt, c.sn, -bs.wo, c.wi);
        const f3 wo_w = frame_to_world(c.ss, c.stt, c.sn, bs.wo);
        p.ray.o = offset_point(c.sp, c.gn, wo_w);                                                    // :231
        p.ray.d = wo_w;
        p.ray.tmax = kInf;
    }
    p.eta *= bs.eta;                                                                                 // :232
    // beta = beta * bsdf_weight (:233).  A depolarizer keeps column 0 times its value and zeroes the rest — the general product
    // with its zero terms dropped
    if (diffuse) {
        const float w = bs.w.m[0];
        for (int i = 0; i < 4; ++i) {
            pp.beta.m[4 * i] = pp.beta.m[4 * i] * w;
            pp.beta.m[4 * i + 1] = 0.0f; pp.beta.m[4 * i + 2] = 0.0f; pp.beta.m[4 * i + 3] = 0.0f;
        }
    } else pp.beta = m44_mul(pp.beta, bs.w);
    p.prev_p = valid ? c.sp : mk(0, 0, 0); p.prev_pdf = bs.pdf;                                       // :237-240
    p.prev_delta = bs.delta ? 1u : 0u;
    // stopping criterion (:245-257) on unpolarized_spectrum(beta) = M00
    const float bmax = pp.beta.m[0];
    active_next &= (bmax != 0.0f);
    const float rr_prob = fminf(bmax * (p.eta * p.eta), 0.95f);
    active_next &= rr_prob > 0.0f;
    const bool rr_active = p.depth >= rc.rr_depth;
    if (rr_active) {
        const float inv = rr_prob > 0.0f ? 1.0f / rr_prob : 0.0f;
        pp.beta = m44_scale(pp.beta, inv);
    }
    active_next &= (!rr_active) | (rr_u < rr_prob);
    if (valid) p.depth += 1;                                                                         // :318
    return active_next;
}

} // namespace mtr
