// host_polarized.cpp — TEST-ONLY.  Compiles the product's polarized per-path arithmetic (mtr_polar.h over mtr_core.h, the
// BVH builder and scene ingestion) for the HOST: whole renders one lane at a time, and the Mueller / Fresnel building blocks on
// arrays, for tests/test_polarized.py and tests/test_gpu_polarized.py.  Never part of libmitransient_amd.so.
#include "../mitransient_amd/csrc/mtr_polar.h"
#include "../mitransient_amd/csrc/mtr_scene_host.h"

#include <cstring>
#include <vector>

using namespace mtr;

namespace {
struct ArrStack {
    static constexpr bool kPark = false;
    void park_prev_p(mtr::f3) {}
    mtr::f3 unpark_prev_p() const { return mtr::mk(0, 0, 0); }
    void park_inc(uint64_t) {}
    uint64_t unpark_inc() const { return 0; }
    void park_prev_pdf(float) {}
    float unpark_prev_pdf() const { return 0.0f; }
    int32_t v[130]; int sp;
    void reset() { sp = 0; }
    void push_if(bool c, int32_t x) { v[sp] = x; sp += c ? 1 : 0; }
    int32_t pop() { return v[--sp]; }
    bool empty() const { return sp == 0; }
    void prof_mark(int) {}
    void count(int) {}
};
// the (H, W, T, 4) Stokes film: S0..S3 in the four floats of a bin
struct StokesSink {
    float *film; uint32_t W, T; uint64_t n;
    void splat4(uint32_t fx, uint32_t fy, uint32_t bin, float s0, float s1, float s2, float s3, float, uint32_t, uint32_t)
    {
        float *d = film + (((size_t)fy * W + fx) * T + bin) * 4u;
        d[0] += s0; d[1] += s1; d[2] += s2; d[3] += s3; ++n;
    }
};
void put16(const M44 &M, float *out) { for (int i = 0; i < 16; ++i) out[i] = M.m[i]; }
M44 get16(const float *in) { M44 M; for (int i = 0; i < 16; ++i) M.m[i] = in[i]; return M; }
}

// a whole polarized render: t4 (H, W, T, 4) Stokes sums, s4 (H, W, 4) = (S0, S1, S2, weight) of the steady image
extern "C" int hp_render(const mtr_scene_desc *d, const mtr_render_params *p, float *t4, float *s4, mtr_counters *out)
{
    HostScene hs;
    if (derive_scene(*d, hs)) return -1;
    for (uint32_t i = 0; i < d->n_materials; ++i) if (!polar_bsdf_supported(d->materials[i].type)) return -3;
    SceneView sv{};
    sv.nodes = hs.nodes.data(); sv.tpairs = hs.tpairs.data(); sv.tshade = hs.tshade.data();
    sv.node_pairs = false; sv.wnodes = nullptr; sv.wnodes4 = nullptr; sv.wnodes8q = nullptr;
    sv.mats = hs.mats.data(); sv.ems = hs.ems.data();
    sv.n_emitters = (uint32_t)hs.ems.size(); sv.n_slots = (uint32_t)hs.tshade.size();
    sv.samp_tris = hs.samp_tris.data(); sv.samp_vn = hs.samp_vn.empty() ? nullptr : hs.samp_vn.data(); sv.face_pmf = hs.face_pmf.data(); sv.face_cdf = hs.face_cdf.data();
    sv.vnormals = hs.vnormals.empty() ? nullptr : hs.vnormals.data();
    sv.texels = hs.texels.empty() ? nullptr : hs.texels.data(); sv.tex_info = hs.tex_info.empty() ? nullptr : hs.tex_info.data();
    sv.uvs = hs.uvs.empty() ? nullptr : hs.uvs.data();
    RenderConst rc = make_render_const(*p, hs.film, sv.n_emitters);
    StokesSink sink{ t4, hs.film.width, hs.film.bins, 0 };
    ArrStack st; st.sp = 0;
    uint64_t closest = 0, shadow = 0, bounces = 0, paths = 0;
    for (uint32_t pix = p->pixel_begin; pix < p->pixel_end; ++pix)
        for (uint32_t s = p->spp_begin; s < p->spp_end; ++s) {
            PolarPath path;
            polar_begin(path, hs.cam, hs.film, rc, pix, s);
            ++paths;
            const bool unwarp = (rc.flags & MTR_FLAG_CAMERA_UNWARP) != 0u;
            if (unwarp) ++closest;                       // (the camera_unwarp ray, as the host harness and k_wf_raygen count it)
            bool alive = true;
            while (alive) {
                BounceStats bs{ 0, 0 };
                alive = polar_bounce(path, sv, hs.film, rc, st, sink, bs, unwarp);
                closest += bs.closest; shadow += bs.shadow; ++bounces;
            }
            const uint32_t fx = path.base.px - hs.film.crop_x, fy = path.base.py - hs.film.crop_y;
            if (fx < hs.film.width && fy < hs.film.height) {
                float *sp = s4 + ((size_t)fy * hs.film.width + fx) * 4u;
                sp[0] += path.L[0]; sp[1] += path.L[1]; sp[2] += path.L[2]; sp[3] += 1.0f;
            }
        }
    if (out) {
        memset(out, 0, sizeof *out);
        out->paths = paths; out->rays_closest = closest; out->rays_shadow = shadow;
        out->bounces = bounces; out->splats_issued = sink.n;
    }
    return 0;
}

// ---- building blocks on arrays (row-major 4x4 matrices, 16 floats each) ----
extern "C" void hp_conductor_reflection(uint32_t n, const float *ci, float er, float ei, float *out16)
{
    for (uint32_t i = 0; i < n; ++i) put16(conductor_reflection_mueller(ci[i], er, ei), out16 + 16 * i);
}
extern "C" void hp_dielectric(uint32_t n, const float *ci, float eta, int transmission, float *out16)
{
    for (uint32_t i = 0; i < n; ++i)
        put16(transmission ? dielectric_transmission_mueller(ci[i], eta) : dielectric_reflection_mueller(ci[i], eta), out16 + 16 * i);
}
// the product's scalar Fresnel terms: which = 0 fresnel_conductor(ci, a, b), 1 fresnel_dielectric(ci, a).r
extern "C" void hp_fresnel_scalar(int which, uint32_t n, const float *ci, float a, float b, float *out)
{
    for (uint32_t i = 0; i < n; ++i) {
        if (which == 0) out[i] = fresnel_conductor(ci[i], a, b);
        else { float r, ct, eit, eti; fresnel_dielectric(ci[i], a, r, ct, eit, eti); out[i] = r; }
    }
}
extern "C" void hp_stokes_basis(uint32_t n, const float *w3, float *out3)
{
    for (uint32_t i = 0; i < n; ++i) {
        const f3 b = stokes_basis(mk(w3[3 * i], w3[3 * i + 1], w3[3 * i + 2]));
        out3[3 * i] = b.x; out3[3 * i + 1] = b.y; out3[3 * i + 2] = b.z;
    }
}
// rotate_stokes_basis(forward, current, target) as a matrix
extern "C" void hp_rotate_stokes_basis(const float *fwd, const float *cur, const float *tgt, float *out16)
{
    float c2, s2;
    rotate_stokes_basis_cs(mk(fwd[0], fwd[1], fwd[2]), mk(cur[0], cur[1], cur[2]), mk(tgt[0], tgt[1], tgt[2]), c2, s2);
    put16(rotator_cs(c2, s2), out16);
}
// to_world_mueller(M, wi_local, wo_local) in the shading frame (s, t, n)
extern "C" void hp_to_world_mueller(const float *M16, const float *stn9, const float *wi, const float *wo, float *out16)
{
    const f3 s = mk(stn9[0], stn9[1], stn9[2]), t = mk(stn9[3], stn9[4], stn9[5]), n = mk(stn9[6], stn9[7], stn9[8]);
    put16(to_world_mueller(get16(M16), s, t, n, mk(wi[0], wi[1], wi[2]), mk(wo[0], wo[1], wo[2])), out16);
}
extern "C" void hp_mul(const float *a16, const float *b16, float *out16) { put16(m44_mul(get16(a16), get16(b16)), out16); }
// one polarized BSDF sample (local frame, the matrix before to_world_mueller): wo3, pdf, eta, w16
extern "C" void hp_bsdf_sample(const mtr_material *m, const float *wi3, float u1, float ua, float ub, float *wo3, float *pdf_eta, float *w16)
{
    const PolarSample ps = polar_bsdf_sample(*m, mk(wi3[0], wi3[1], wi3[2]), u1, ua, ub, m->a[0]);
    wo3[0] = ps.wo.x; wo3[1] = ps.wo.y; wo3[2] = ps.wo.z; pdf_eta[0] = ps.pdf; pdf_eta[1] = ps.eta;
    put16(ps.w, w16);
}
