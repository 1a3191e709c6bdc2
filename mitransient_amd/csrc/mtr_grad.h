// mtr_grad.h — reverse-mode gradients of transient_path (ABI 15, mtr_render_grad; ABI 16, mtr_render_grad_tex): the per-lane
// arithmetic, shared by the gfx950 kernel (mtr_grad.hip) and the host builds of the tests (tests/host_grad.cpp,
// tests/host_grad_tex.cpp).
//
// What is differentiated: the constant RGB reflectance of `diffuse` materials, the texels of a bitmap on a
// `diffuse` reflectance (through the texel hook below) and the constant RGB radiance of
// `area` / `angulararea` emitters, for the loss  sum g_s . steady + sum g_t . transient  of the seeded estimator, sampling
// detached as in the reference's PRB (transientpath.py:284-299, integrators/common.py:325-409): Russian-roulette probabilities,
// BSDF sampling and emitter sampling are constants.  Each contribution c (an emission or an emitter-sampling term) carries the
// adjoint weight  w_c = g_s[pixel] * steady_scale + g_t[pixel, film_bin(opl_c)] * transient_scale  (the transient term only when
// the bin is in range), and
//   d loss / d a_m = sum_c w_c (.) c (.) n_m(c) / a_m       n_m(c): vertices on m whose BSDF factor is part of c
//   d loss / d L_e = sum_{c lit by e} w_c (.) c / L_e      computed from c with the radiance left out: the traced emitter table
//                                                         carries UNIT radiance, c = c_unit (.) L_e
//   d loss / d t   = sum_{vertices v on a bitmap} w_t(v) R(v) / a(v)   t a texel, a(v) the interpolated colour at the vertex,
//                                                         w_t(v) the bilinear weight of t in a(v) (texture_taps), R(v) the
//                                                         remaining sum at v: a(v) is linear in its four taps
// PATH REPLAY in the time domain: a lane traces its path once to sum A = sum_c w_c (.) c, then again from the same seed,
// subtracting each term as it is re-emitted; at every diffuse vertex the remaining sum (this vertex's emitter-sampling term and
// every later term) divided by the vertex's albedo goes to its material.  Nothing per path is kept in memory between the walks.
//
// transient_nlos_path (ABI 17): the same replay over nlos_bounce (mtr_nlos.h), grad_nlos_walk below.  A term is one
// emitter_nee_sample splat  Lr = beta (.) bsdf(c) [(.) bsdf(c2) / pdf_ls] (.) w_projector  (transientnlospath.py:432-564): its albedo
// factors are the vertices whose weight is in beta, c itself and — with laser sampling — the laser spot c2; its irradiance factor
// is the projector's `irradiance` (the walk runs with UNIT irradiance, the true one goes alongside as the one "emitter").  Every
// diffuse vertex receives R / a as above; c2's material receives its own term over its albedo.  Detached as well: the laser-target
// and hidden-geometry sampling, the method coin and the dr.epsilon cut-offs (:539-540).  Texels (ABI 20): grad_nlos_walk with a
// texel hook — the bitmap-textured vertices in beta and at c give R / a(v) to their taps, a textured laser spot its term over a(c2).
#pragma once
#include "mtr_core.h"
#include "mtr_nlos.h"

namespace mtr {

struct GradConst {
    const float *g_s;          // (H, W, 3): upstream gradient of the developed steady image
    const float *g_t;          // (H, W, T, 3): upstream gradient of the developed transient tensor
    const float *em_radiance;  // [n_emitters * 3]: the emitters' true radiance (the traced table has unit radiance)
    float steady_scale;        // d steady / d contribution: 1 / total spp (develop divides the sum by the sample count)
    float transient_scale;     // d transient / d contribution: the sample scale the splat multiplies by (common.py:417-421)
};

struct d3 { double x, y, z; };

// shade_hit's emitter-pick hook (mtr_core.h): the index of the emitter its sampling term samples
struct EmitterPickTo {
    uint32_t *out;
    MTR_HD void operator()(uint32_t e) const { *out = e; }
};

// Acc: add_mat(m, g) / add_em(e, g) receive the gradients; vertex(m, dist, active_next) and term(kind, e, opl, c_unit) see the
// replay's vertices and terms in path order (kind 0 emission, 1 emitter sampling) — no-ops in the kernel, per-vertex records in
// the host build of the tests (tests/host_grad.cpp)
struct NullGradSink {
    MTR_HD void splat(uint32_t, uint32_t, uint32_t, float, float, float, float, uint32_t, uint32_t) {}
};

// The texel hook of grad_walk: tex(i, g) receives g = w_t R / a for the texel at index i of the scene's texel array (all textures
// in scene order), once per tap — taps that wrap onto one texel (width or height 1) arrive as separate calls and add up.
// The default does nothing and compiles the texel code out (kOn): callers that pass no hook are what they were.
struct NoTexelGrad {
    static constexpr bool kOn = false;
    MTR_HD void operator()(uint32_t, f3) const {}
};

// The tint hook of grad_walk (ABI 19, mtr_render_grad_tint): the constant RGB `specular_reflectance` (which 0, mtr_material::c) and
// `specular_transmittance` (which 1, ::c2) of conductor, roughconductor, dielectric, thindielectric and roughdielectric.  The tint
// multiplies the BSDF weight or value linearly and no sampling decision reads it (lobe choice is by Fresnel, the visible normal by
// alpha, the pdfs carry no tint), so a term stays multilinear in the tints:  d loss / d s = sum_c w_c (.) c (.) k_s(c) / s,  k_s(c) the
// vertices at which the factor s is part of c.  WHICH tint a vertex contributes depends on the lobe: the vertex's emitter-sampling
// term (rough lobes only) carries the tint of the lobe bsdf_eval_cos evaluates for the shadow direction, every later term the tint
// of the lobe that was sampled — known after shade_finish, from the side of the new ray (the shading code's own test, ci * co > 0:
// reflection).  tint(m, which, g) receives the term over its tint, then the remaining sum over the sampled lobe's tint; a channel
// whose tint is exactly 0 receives 0.  lobes(m, nee, sampled): the two lobes of the vertex for the records of a host build (nee -1:
// no emitter-sampling term).  The default does nothing and compiles the tint code out (kOn).
struct NoTintGrad {
    static constexpr bool kOn = false;
    MTR_HD void operator()(uint32_t, uint32_t, f3) const {}
    MTR_HD void lobes(uint32_t, int, int) const {}
};
MTR_HD bool bsdf_has_tints(uint32_t type)
{
    return type == MTR_BSDF_CONDUCTOR || type == MTR_BSDF_ROUGHCONDUCTOR || type == MTR_BSDF_DIELECTRIC ||
           type == MTR_BSDF_THINDIELECTRIC || type == MTR_BSDF_ROUGHDIELECTRIC;
}
// the tint of the lobe that takes wi (local, cosine ci) to a direction with cosine co about the same normal: conductors reflect;
// a dielectric interface transmits unless both are on one side (rough_dielectric_eval_pdf's `reflect`)
MTR_HD uint32_t tint_of_lobe(uint32_t type, float ci, float co)
{
    const bool dielectric = type == MTR_BSDF_DIELECTRIC || type == MTR_BSDF_THINDIELECTRIC || type == MTR_BSDF_ROUGHDIELECTRIC;
    return (dielectric && !(ci * co > 0.0f)) ? 1u : 0u;
}
// cosine about the shading normal sn of the direction from the vertex sp to the sampled emitter point, rebuilt from the shadow ray
// shade_hit emitted (origin offset along the geometric normal, tmax = distance (1 - kShadowEps)): the point to rounding
MTR_HD float shadow_cos(const Ray &shadow, f3 sp, f3 sn)
{
    const float t = shadow.tmax / (1.0f - kShadowEps);
    const f3 ep = mk(fmaf(shadow.d.x, t, shadow.o.x), fmaf(shadow.d.y, t, shadow.o.y), fmaf(shadow.d.z, t, shadow.o.z));
    return dot(ep - sp, sn);
}
MTR_HD f3 over_tint(const mtr_material &m, uint32_t which, double rx, double ry, double rz)
{
    const float *s = which ? m.c2 : m.c;
    return mk(s[0] != 0.0f ? (float)(rx / (double)s[0]) : 0.0f, s[1] != 0.0f ? (float)(ry / (double)s[1]) : 0.0f,
              s[2] != 0.0f ? (float)(rz / (double)s[2]) : 0.0f);
}

// w_c of a contribution of film pixel (fx, fy) at optical path length opl; the bin is the splat's own (film_bin)
MTR_HD f3 grad_weight(const GradConst &gc, const Film &film, uint32_t fx, uint32_t fy, float opl)
{
    if (!((fx < film.width) & (fy < film.height))) return mk(0, 0, 0);
    const size_t pix = (size_t)fy * film.width + fx;
    const float *gs = gc.g_s + 3u * pix;
    f3 w = mk(gs[0] * gc.steady_scale, gs[1] * gc.steady_scale, gs[2] * gc.steady_scale);
    const int32_t bin = film_bin(film, opl);
    if (bin >= 0) {
        const float *gt = gc.g_t + 3u * (pix * film.bins + (uint32_t)bin);
        w = mk(fmaf(gt[0], gc.transient_scale, w.x), fmaf(gt[1], gc.transient_scale, w.y), fmaf(gt[2], gc.transient_scale, w.z));
    }
    return w;
}

// One walk of a lane's path (transientpath.py:140-319 through shade_hit / shade_finish, the general shading code).
// REPLAY = false: returns A = sum_c w_c (.) c.  REPLAY = true: R starts at A; every term is subtracted as it is met, emitter
// gradients go to acc.add_em(e, w_c (.) c_unit), material gradients to acc.add_mat(m, R / a_m) at each diffuse vertex whose
// BSDF factor enters the remaining terms.  unwarp: camera_unwarp from bounce 0's own closest hit (as path_bounce).
// tex: the texel hook (bitmap-textured `diffuse` vertices; extended shading code only: a bitmap implies it).
// tint: the tint hook (vertices on conductors and dielectric interfaces).
template <bool ROUGH, bool REPLAY, class Stack, class Acc, class Tex = NoTexelGrad, class Tint = NoTintGrad>
MTR_HD d3 grad_walk(Path p, const SceneView &sc, const Film &film, const RenderConst &rc, const GradConst &gc, Stack &st,
                    Acc &acc, d3 R, Tex tex = Tex(), Tint tint = Tint())
{
    NullGradSink ns;
    const bool unwarp = (rc.flags & MTR_FLAG_CAMERA_UNWARP) != 0u;
    const uint32_t fx = p.px - film.crop_x, fy = p.py - film.crop_y;
    bool alive = true;
    while (alive) {
        const Hit h = traverse<false>(sc, p.ray.o, p.ray.d, p.ray.tmax, st);
        if (unwarp && p.depth == 0u && h.prim >= 0) p.dist = -h.t;
        Pending pd; Ray shadow; HitCtx hc;
        shadow.o = mk(0, 0, 0); shadow.d = mk(0, 0, 1); shadow.tmax = 0.0f;
        hc.em_plus1 = 0u; hc.mat = 0u;
        uint32_t e_sampled = 0u;                             // which emitter shade_hit's emitter-sampling term samples
        shade_hit<ROUGH>(p, h, sc, film, rc, ns, pd, shadow, &hc, EmitterPickTo{ &e_sampled });
        const bool valid = h.prim >= 0;
        if (REPLAY && valid) acc.vertex(hc.mat, p.dist, pd.active_next != 0u);
        // emission (transientpath.py:166-180), at the distance of this vertex
        if (valid && hc.em_plus1 != 0u) {
            const uint32_t e = hc.em_plus1 - 1u;
            const float *L = gc.em_radiance + 3u * e;
            const f3 w = grad_weight(gc, film, fx, fy, p.dist);
            const f3 cu = pd.Le;
            const double cx = (double)w.x * (double)(cu.x * L[0]), cy = (double)w.y * (double)(cu.y * L[1]),
                         cz = (double)w.z * (double)(cu.z * L[2]);
            if (REPLAY) {
                R.x -= cx; R.y -= cy; R.z -= cz;
                acc.add_em(e, mk(w.x * cu.x, w.y * cu.y, w.z * cu.z));
                acc.term(0u, e, p.dist, cu);
            } else { R.x += cx; R.y += cy; R.z += cz; }
        }
        // the BSDF factor of this vertex is part of its emitter-sampling term and of every later term
        if (REPLAY && valid && pd.active_next) {
            const mtr_material &m = sc.mats[hc.mat];
            if (m.type == MTR_BSDF_DIFFUSE && m.albedo_texture == 0u) {
                // a zero channel gets no gradient from paths through m (its remaining sum is zero up to rounding)
                acc.add_mat(hc.mat, mk(m.a[0] != 0.0f ? (float)(R.x / (double)m.a[0]) : 0.0f,
                                       m.a[1] != 0.0f ? (float)(R.y / (double)m.a[1]) : 0.0f,
                                       m.a[2] != 0.0f ? (float)(R.z / (double)m.a[2]) : 0.0f));
            }
            if (Tex::kOn && ROUGH && m.type == MTR_BSDF_DIFFUSE && m.albedo_texture != 0u && sc.texels) {
                // a = sum of four taps w_t t: d loss / d a = R / a per channel (0 where a is 0, as above), times w_t to each tap
                float u, v;
                hit_uv(sc, h, u, v);
                const TexTaps k = texture_taps(sc.tex_info[m.albedo_texture - 1u], u, v);
                const f3 a = pd.has_alb ? pd.alb : texture_eval(sc.texels, k);
                const f3 g = mk(a.x != 0.0f ? (float)(R.x / (double)a.x) : 0.0f, a.y != 0.0f ? (float)(R.y / (double)a.y) : 0.0f,
                                a.z != 0.0f ? (float)(R.z / (double)a.z) : 0.0f);
                tex(k.first + (uint32_t)k.i00, g * (k.w0x * k.w0y)); tex(k.first + (uint32_t)k.i10, g * (k.w1x * k.w0y));
                tex(k.first + (uint32_t)k.i01, g * (k.w0x * k.w1y)); tex(k.first + (uint32_t)k.i11, g * (k.w1x * k.w1y));
            }
        }
        bool tinted = false; int nee_lobe = -1;
        if constexpr (Tint::kOn) tinted = REPLAY && valid && pd.active_next && bsdf_has_tints(sc.mats[hc.mat].type);
        bool occluded = false;
        if (pd.has_shadow) occluded = traverse<true>(sc, shadow.o, shadow.d, shadow.tmax, st).prim >= 0;
        // emitter sampling (:188-218), at distance + ds.dist * eta
        if (pd.has_shadow && !occluded) {
            const uint32_t e = e_sampled;
            const float *L = gc.em_radiance + 3u * e;
            const f3 w = grad_weight(gc, film, fx, fy, pd.opl);
            const f3 cu = pd.Lr;
            const double cx = (double)w.x * (double)(cu.x * L[0]), cy = (double)w.y * (double)(cu.y * L[1]),
                         cz = (double)w.z * (double)(cu.z * L[2]);
            if (REPLAY) {
                R.x -= cx; R.y -= cy; R.z -= cz;
                acc.add_em(e, mk(w.x * cu.x, w.y * cu.y, w.z * cu.z));
                acc.term(1u, e, pd.opl, cu);
            } else { R.x += cx; R.y += cy; R.z += cz; }
            if constexpr (Tint::kOn) if (tinted) {
                // the term carries the tint of the lobe evaluated for the shadow direction
                const mtr_material &m = sc.mats[hc.mat];
                nee_lobe = (int)tint_of_lobe(m.type, hc.wi.z, shadow_cos(shadow, hc.sp, hc.sn));
                tint(hc.mat, (uint32_t)nee_lobe, over_tint(m, (uint32_t)nee_lobe, cx, cy, cz));
            }
        }
        alive = shade_finish<ROUGH>(p, h, occluded, pd, sc, film, rc, ns);
        if constexpr (Tint::kOn) if (tinted) {
            // ... and every later term the tint of the lobe that was sampled: the side of the new ray
            const mtr_material &m = sc.mats[hc.mat];
            const uint32_t lobe = tint_of_lobe(m.type, hc.wi.z, dot(p.ray.d, hc.sn));
            tint(hc.mat, lobe, over_tint(m, lobe, R.x, R.y, R.z));
            tint.lobes(hc.mat, nee_lobe, (int)lobe);
        }
    }
    return R;
}

// lane (pixel, s) of the render: identity = RNG identity (lane = pixel * spp_total + s), as every primal organisation
template <bool ROUGH, class Stack, class Acc, class Tex = NoTexelGrad, class Tint = NoTintGrad>
MTR_HD void grad_lane(const SceneView &sc, const Camera &cam, const Film &film, const RenderConst &rc, const GradConst &gc,
                      uint32_t pixel, uint32_t s, Stack &st, Acc &acc, Tex tex = Tex(), Tint tint = Tint())
{
    Path p;
    path_begin(p, cam, film, rc, pixel, s);
    const d3 zero = { 0.0, 0.0, 0.0 };
    const d3 A = grad_walk<ROUGH, false>(p, sc, film, rc, gc, st, acc, zero);
    grad_walk<ROUGH, true>(p, sc, film, rc, gc, st, acc, A, tex, tint);
}

// d loss / d a of a `diffuse` material with a constant reflectance from the sum r its factor is part of: r / a per channel, 0 for
// a zero channel (never NaN) and for any other material
MTR_HD bool grad_over_albedo(const mtr_material &m, double rx, double ry, double rz, f3 &g)
{
    if (m.type != MTR_BSDF_DIFFUSE || m.albedo_texture != 0u) return false;
    g = mk(m.a[0] != 0.0f ? (float)(rx / (double)m.a[0]) : 0.0f, m.a[1] != 0.0f ? (float)(ry / (double)m.a[1]) : 0.0f,
           m.a[2] != 0.0f ? (float)(rz / (double)m.a[2]) : 0.0f);
    return true;
}

// nlos_bounce's hook (mtr_nlos.h: NoNlosHook) of the replay.  replay false: *R gathers A = sum_c w_c (.) c.  replay true: *R starts at
// A; a vertex whose BSDF factor enters its own term and every later one receives R / a, a term is subtracted as it is met, the
// laser spot's material receives the term over its albedo and the laser (emitter 0) the term without its irradiance.
template <class Acc>
struct NlosGradHook {
    static constexpr bool kOn = true;
    static constexpr bool kTex = false;
    const SceneView *sc; const Film *film; const GradConst *gc; Acc *acc; d3 *R;
    uint32_t fx, fy; bool replay;
    MTR_HD void vertex(uint32_t m, bool active_next) const
    {
        if (!replay) return;
        acc->vertex(m, 0.0f, active_next);
        f3 g;
        if (active_next && grad_over_albedo(sc->mats[m], R->x, R->y, R->z, g)) acc->add_mat(m, g);
    }
    MTR_HD void term(f3 cu, float opl, uint32_t m, bool at_laser_spot) const
    {
        const float *L = gc->em_radiance;
        const f3 w = grad_weight(*gc, *film, fx, fy, opl);
        const double cx = (double)w.x * (double)(cu.x * L[0]), cy = (double)w.y * (double)(cu.y * L[1]),
                     cz = (double)w.z * (double)(cu.z * L[2]);
        if (!replay) { R->x += cx; R->y += cy; R->z += cz; return; }
        f3 g;
        if (at_laser_spot && grad_over_albedo(sc->mats[m], cx, cy, cz, g)) acc->add_mat(m, g);
        R->x -= cx; R->y -= cy; R->z -= cz;
        acc->add_em(0u, mk(w.x * cu.x, w.y * cu.y, w.z * cu.z));
        acc->term(1u, m, opl, cu);
    }
};

// NlosGradHook with the texel hook of grad_walk (ABI 20; extended shading code only: a bitmap implies it).  A bounce vertex on a
// bitmap-textured `diffuse` gives R / a to its four taps, a(v) the albedo nlos_bounce shaded with; a textured laser spot c2 gives
// the term over a(c2) to c2's taps (spot() keeps c2's lookup until the term arrives: *spot_h, *spot_a).  Materials and the laser
// receive what NlosGradHook gives them (a textured material: nothing).
template <class Acc, class Tex>
struct NlosGradTexHook {
    static constexpr bool kOn = true;
    static constexpr bool kTex = true;
    const SceneView *sc; const Film *film; const GradConst *gc; Acc *acc; d3 *R;
    uint32_t fx, fy; bool replay;
    Tex tex; Hit *spot_h; f3 *spot_a;
    // r / a per channel (0 where a is 0) to the four taps of the lookup at h, times texture_taps' own weights
    MTR_HD void taps(const mtr_material &m, const Hit &h, f3 a, double rx, double ry, double rz) const
    {
        if (m.type != MTR_BSDF_DIFFUSE || m.albedo_texture == 0u || !sc->texels) return;
        float u, v;
        hit_uv(*sc, h, u, v);
        const TexTaps k = texture_taps(sc->tex_info[m.albedo_texture - 1u], u, v);
        const f3 g = mk(a.x != 0.0f ? (float)(rx / (double)a.x) : 0.0f, a.y != 0.0f ? (float)(ry / (double)a.y) : 0.0f,
                        a.z != 0.0f ? (float)(rz / (double)a.z) : 0.0f);
        tex(k.first + (uint32_t)k.i00, g * (k.w0x * k.w0y)); tex(k.first + (uint32_t)k.i10, g * (k.w1x * k.w0y));
        tex(k.first + (uint32_t)k.i01, g * (k.w0x * k.w1y)); tex(k.first + (uint32_t)k.i11, g * (k.w1x * k.w1y));
    }
    MTR_HD void vertex(uint32_t m, bool active_next) const
    {
        if (!replay) return;
        acc->vertex(m, 0.0f, active_next);
        f3 g;
        if (active_next && grad_over_albedo(sc->mats[m], R->x, R->y, R->z, g)) acc->add_mat(m, g);
    }
    MTR_HD void vertex_tex(Hit h, f3 albedo, uint32_t m, bool active_next) const
    {
        if (replay && active_next) taps(sc->mats[m], h, albedo, R->x, R->y, R->z);
    }
    MTR_HD void spot(Hit h2, f3 albedo2) const { *spot_h = h2; *spot_a = albedo2; }
    MTR_HD void term(f3 cu, float opl, uint32_t m, bool at_laser_spot) const
    {
        const float *L = gc->em_radiance;
        const f3 w = grad_weight(*gc, *film, fx, fy, opl);
        const double cx = (double)w.x * (double)(cu.x * L[0]), cy = (double)w.y * (double)(cu.y * L[1]),
                     cz = (double)w.z * (double)(cu.z * L[2]);
        if (!replay) { R->x += cx; R->y += cy; R->z += cz; return; }
        f3 g;
        if (at_laser_spot && grad_over_albedo(sc->mats[m], cx, cy, cz, g)) acc->add_mat(m, g);
        if (at_laser_spot) taps(sc->mats[m], *spot_h, *spot_a, cx, cy, cz);
        R->x -= cx; R->y -= cy; R->z -= cz;
        acc->add_em(0u, mk(w.x * cu.x, w.y * cu.y, w.z * cu.z));
        acc->term(1u, m, opl, cu);
    }
};

// One walk of a lane's NLOS path (TransientNLOSPath.sample, :740-918, through nlos_bounce): `replay` as REPLAY of grad_walk.
// nc carries unit irradiance; reload: nlos_bounce's (a kernel re-reads nc / film / rc after every traversal).
// tex: the texel hook of grad_walk; the default compiles the texel code out (NlosGradHook, as before ABI 20).
template <bool EXT, class Stack, class Acc, class Reload = NoReload, class Tex = NoTexelGrad>
MTR_HD d3 grad_nlos_walk(Path p, bool replay, const SceneView &sc, const NlosConst &nc, const Film &film, const RenderConst &rc,
                         const GradConst &gc, Stack &st, Acc &acc, d3 R, const Reload &reload = Reload(), Tex tex = Tex())
{
    NullGradSink ns;
    BounceStats bs{ 0u, 0u };
    if constexpr (Tex::kOn && EXT) {
        Hit spot_h; f3 spot_a = mk(0, 0, 0);
        spot_h.t = 0.0f; spot_h.u = 0.0f; spot_h.v = 0.0f; spot_h.prim = 0;
        const NlosGradTexHook<Acc, Tex> hook{ &sc, &film, &gc, &acc, &R, p.px - film.crop_x, p.py - film.crop_y, replay, tex, &spot_h, &spot_a };
        bool alive = true;
        while (alive) alive = nlos_bounce<EXT, 0u>(p, sc, nc, film, rc, st, ns, bs, reload, hook);
        return R;
    } else {
        const NlosGradHook<Acc> hook{ &sc, &film, &gc, &acc, &R, p.px - film.crop_x, p.py - film.crop_y, replay };
        bool alive = true;
        while (alive) alive = nlos_bounce<EXT, 0u>(p, sc, nc, film, rc, st, ns, bs, reload, hook);
        return R;
    }
}

// lane (pixel, s) of a NLOS render: both walks through ONE copy of the loop (four traversals per bounce are inlined in it)
template <bool EXT, class Stack, class Acc, class Reload = NoReload, class Tex = NoTexelGrad>
MTR_HD void grad_nlos_lane(const SceneView &sc, const NlosConst &nc, const Film &film, const RenderConst &rc, const GradConst &gc,
                           uint32_t pixel, uint32_t s, Stack &st, Acc &acc, const Reload &reload = Reload(), Tex tex = Tex())
{
    Path p;
    nlos_begin(p, nc, film, rc, pixel, s);
    d3 R = { 0.0, 0.0, 0.0 };
    for (int pass = 0; pass < 2; ++pass) R = grad_nlos_walk<EXT>(p, pass != 0, sc, nc, film, rc, gc, st, acc, R, reload, tex);
}

} // namespace mtr
