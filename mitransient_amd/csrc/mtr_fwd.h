// mtr_fwd.h — forward-mode derivatives of transient_path (ABI 18, mtr_render_fwd): the per-lane arithmetic, shared by the gfx950
// kernel (mtr_fwd.hip) and the host build of the tests (tests/host_fwd.cpp).
//
// The transpose of mtr_grad.h: the same parameters — the constant RGB reflectance of `diffuse` materials, the texels of
// a bitmap on a `diffuse` reflectance, the constant RGB radiance of `area` / `angulararea` emitters — the same detached sampling
// (Russian roulette, BSDF sampling and emitter sampling are constants), every term at its own bin.  With tangents  da_m, dt, dL_e  the
// output is the tangent of the DEVELOPED film, J v, where mtr_render_grad computes J^T g.
//
// ONE walk per lane.  Every term c is multilinear in the albedos at the vertices whose BSDF factor it carries and linear in the
// radiance of the emitter e that lights it, c = c_unit (.) L_e (the traced emitter table carries UNIT radiance), so
//   dc = c_unit (.) (L_e (.) D + dL_e)        D = sum over those vertices of  da / a  (the path's running LOG-DERIVATIVE, f64)
// D is updated at every vertex on a `diffuse` material with active_next — where grad_walk calls add_mat — by  da_m / a_m,  or with a
// bitmap by  (sum_taps w_t dt) / a(v)  (texture_taps' f32 weights, a(v) the interpolated colour).  ZERO RULE: a channel whose albedo
// is exactly 0 adds nothing (0, never NaN or Inf), as in the reverse mode.  The emission term of a vertex uses D BEFORE that vertex's
// update, its emitter-sampling term D AFTER it (n_m(c) of mtr_grad.h).  dc is computed in f64 and rounded to f32 once.
// Film: dc is splatted like the primal term — times the sample scale into (pixel, film_bin(opl)) when the bin is in range, and into
// the pixel's steady sum through the lane's own f32 sum (as the primal's p.L), once per lane.
#pragma once
#include "mtr_core.h"
#include "mtr_grad.h"

namespace mtr {

// the tangent source: device (or host) tables
struct FwdConst {
    const float *em_radiance;  // [n_emitters * 3]: the emitters' true radiance (the traced table has unit radiance)
    const float *tan_mats;     // [n_materials * 3]: da_m (entries of other than plain `diffuse` materials are not read)
    const float *tan_ems;      // [n_emitters * 3]: dL_e
    const float *tan_texels;   // [n_texels * 3]: dt, all textures in scene order (mtr_scene_texture_layout); null: no texel tangents
};

// The tint hook of fwd_walk (ABI 19, mtr_render_fwd_tint; the transpose of mtr_grad.h's): tint(m, which) answers the tangent ds of
// `specular_reflectance` (which 0) or `specular_transmittance` (which 1) of material m, three floats, or null.  At a vertex on a
// conductor or a dielectric interface the emitter-sampling term uses  D + ds_nee / s_nee  (the lobe evaluated for the shadow
// direction) and the continued path  D + ds_sampled / s_sampled  (the lobe that was sampled); zero rule as for albedos.  The default
// answers nothing and compiles the tint code out (kOn).
struct NoTintTan {
    static constexpr bool kOn = false;
    MTR_HD const float *operator()(uint32_t, uint32_t) const { return nullptr; }
};
MTR_HD d3 plus_tint(d3 D, const mtr_material &m, uint32_t which, const float *ds)
{
    const float *s = which ? m.c2 : m.c;
    if (ds) {
        if (s[0] != 0.0f) D.x += (double)ds[0] / (double)s[0];
        if (s[1] != 0.0f) D.y += (double)ds[1] / (double)s[1];
        if (s[2] != 0.0f) D.z += (double)ds[2] / (double)s[2];
    }
    return D;
}

// Sink: splat(fx, fy, opl, dc) receives every non-zero term's tangent (before the sample scale), steady(fx, fy, sum) the lane's f32
// sum of them at the end of its path.
template <bool ROUGH, class Stack, class Sink, class Tint = NoTintTan>
MTR_HD void fwd_walk(Path p, const SceneView &sc, const Film &film, const RenderConst &rc, const FwdConst &fc, Stack &st, Sink &sink,
                     Tint tint = Tint())
{
    NullGradSink ns;
    const bool unwarp = (rc.flags & MTR_FLAG_CAMERA_UNWARP) != 0u;
    const uint32_t fx = p.px - film.crop_x, fy = p.py - film.crop_y;
    d3 D = { 0.0, 0.0, 0.0 };
    f3 sum = mk(0, 0, 0);
    // dc of the term c_unit lit by emitter e, at optical path length opl, with the log-derivative Dv
    auto term = [&](f3 cu, uint32_t e, float opl, const d3 &Dv) {
        const float *L = fc.em_radiance + 3u * e, *dL = fc.tan_ems + 3u * e;
        const f3 dc = mk((float)((double)cu.x * ((double)L[0] * Dv.x + (double)dL[0])),
                         (float)((double)cu.y * ((double)L[1] * Dv.y + (double)dL[1])),
                         (float)((double)cu.z * ((double)L[2] * Dv.z + (double)dL[2])));
        if (dc.x != 0.0f || dc.y != 0.0f || dc.z != 0.0f) {
            sum = mk(sum.x + dc.x, sum.y + dc.y, sum.z + dc.z);
            sink.splat(fx, fy, opl, dc);
        }
    };
    bool alive = true;
    while (alive) {
        const Hit h = traverse<false>(sc, p.ray.o, p.ray.d, p.ray.tmax, st);
        if (unwarp && p.depth == 0u && h.prim >= 0) p.dist = -h.t;
        Pending pd; Ray shadow; HitCtx hc;
        shadow.o = mk(0, 0, 0); shadow.d = mk(0, 0, 1); shadow.tmax = 0.0f;
        hc.em_plus1 = 0u; hc.mat = 0u;
        uint32_t e_sampled = 0u;
        shade_hit<ROUGH>(p, h, sc, film, rc, ns, pd, shadow, &hc, EmitterPickTo{ &e_sampled });
        const bool valid = h.prim >= 0;
        // emission (transientpath.py:166-180), at the distance of this vertex, with D before this vertex
        if (valid && hc.em_plus1 != 0u) term(pd.Le, hc.em_plus1 - 1u, p.dist, D);
        // the BSDF factor of this vertex is part of its emitter-sampling term and of every later term
        if (valid && pd.active_next) {
            const mtr_material &m = sc.mats[hc.mat];
            if (m.type == MTR_BSDF_DIFFUSE && m.albedo_texture == 0u) {
                const float *da = fc.tan_mats + 3u * hc.mat;
                if (m.a[0] != 0.0f) D.x += (double)da[0] / (double)m.a[0];
                if (m.a[1] != 0.0f) D.y += (double)da[1] / (double)m.a[1];
                if (m.a[2] != 0.0f) D.z += (double)da[2] / (double)m.a[2];
            }
            if (ROUGH && m.type == MTR_BSDF_DIFFUSE && m.albedo_texture != 0u && sc.texels && fc.tan_texels) {
                float u, v;
                hit_uv(sc, h, u, v);
                const TexTaps k = texture_taps(sc.tex_info[m.albedo_texture - 1u], u, v);
                const f3 a = pd.has_alb ? pd.alb : texture_eval(sc.texels, k);
                const float *t00 = fc.tan_texels + 3u * ((size_t)k.first + k.i00), *t10 = fc.tan_texels + 3u * ((size_t)k.first + k.i10),
                            *t01 = fc.tan_texels + 3u * ((size_t)k.first + k.i01), *t11 = fc.tan_texels + 3u * ((size_t)k.first + k.i11);
                const double w00 = (double)(k.w0x * k.w0y), w10 = (double)(k.w1x * k.w0y), w01 = (double)(k.w0x * k.w1y),
                             w11 = (double)(k.w1x * k.w1y);
                if (a.x != 0.0f) D.x += (w00 * t00[0] + w10 * t10[0] + w01 * t01[0] + w11 * t11[0]) / (double)a.x;
                if (a.y != 0.0f) D.y += (w00 * t00[1] + w10 * t10[1] + w01 * t01[1] + w11 * t11[1]) / (double)a.y;
                if (a.z != 0.0f) D.z += (w00 * t00[2] + w10 * t10[2] + w01 * t01[2] + w11 * t11[2]) / (double)a.z;
            }
        }
        bool occluded = false;
        if (pd.has_shadow) occluded = traverse<true>(sc, shadow.o, shadow.d, shadow.tmax, st).prim >= 0;
        // emitter sampling (:188-218), at distance + ds.dist * eta, with D after this vertex
        bool tinted = false;
        if constexpr (Tint::kOn) tinted = valid && pd.active_next && bsdf_has_tints(sc.mats[hc.mat].type);
        if (pd.has_shadow && !occluded) {
            if (tinted) {
                if constexpr (Tint::kOn) {
                    const mtr_material &m = sc.mats[hc.mat];
                    const uint32_t lobe = tint_of_lobe(m.type, hc.wi.z, shadow_cos(shadow, hc.sp, hc.sn));
                    term(pd.Lr, e_sampled, pd.opl, plus_tint(D, m, lobe, tint(hc.mat, lobe)));
                }
            } else term(pd.Lr, e_sampled, pd.opl, D);
        }
        alive = shade_finish<ROUGH>(p, h, occluded, pd, sc, film, rc, ns);
        if constexpr (Tint::kOn) if (tinted) {
            const mtr_material &m = sc.mats[hc.mat];
            const uint32_t lobe = tint_of_lobe(m.type, hc.wi.z, dot(p.ray.d, hc.sn));
            D = plus_tint(D, m, lobe, tint(hc.mat, lobe));
        }
    }
    if (sum.x != 0.0f || sum.y != 0.0f || sum.z != 0.0f) sink.steady(fx, fy, sum);
}

// lane (pixel, s) of the render: identity = RNG identity (lane = pixel * spp_total + s), as every primal organisation
template <bool ROUGH, class Stack, class Sink, class Tint = NoTintTan>
MTR_HD void fwd_lane(const SceneView &sc, const Camera &cam, const Film &film, const RenderConst &rc, const FwdConst &fc,
                     uint32_t pixel, uint32_t s, Stack &st, Sink &sink, Tint tint = Tint())
{
    Path p;
    path_begin(p, cam, film, rc, pixel, s);
    fwd_walk<ROUGH>(p, sc, film, rc, fc, st, sink, tint);
}

} // namespace mtr
