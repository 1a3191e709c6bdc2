// host_grad_tex.cpp — TEST-ONLY.  host_grad.cpp with the texel hook of mtr_grad.h: the gradient arithmetic of mtr_render_grad_tex
// compiled for the HOST and run one lane at a time, so that the CPU tests can compare texel gradients with finite differences of
// the CPU oracle and the GPU tests can compare both tiers of the kernel with it.  Never part of libmitransient_amd.so.
#include "../mitransient_amd/csrc/mtr_core.h"
#include "../mitransient_amd/csrc/mtr_grad.h"
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
// f64 sums on the host, as the kernel (f64 slab or f64 atomics)
struct HostAcc {
    double *mats, *ems;
    void add_mat(uint32_t m, f3 g) { mats[3 * m] += g.x; mats[3 * m + 1] += g.y; mats[3 * m + 2] += g.z; }
    void add_em(uint32_t e, f3 g) { ems[3 * e] += g.x; ems[3 * e + 1] += g.y; ems[3 * e + 2] += g.z; }
    void vertex(uint32_t, float, bool) {}
    void term(uint32_t, uint32_t, float, f3) {}
};
struct HostTexels {
    static constexpr bool kOn = true;
    double *t;
    void operator()(uint32_t i, f3 g) const { t[3 * (size_t)i] += g.x; t[3 * (size_t)i + 1] += g.y; t[3 * (size_t)i + 2] += g.z; }
};
}

// The gradient of the lanes of `p` (mtr_render_grad_tex's contract): grad_mats (n_materials, 3), grad_ems (n_emitters, 3) and
// grad_texels (the texels of every texture in scene order, 3 each), f64.  *n_texels_out: the number of texels (grad_texels may be
// NULL to ask for it alone).
extern "C" int hg_render_grad_tex(const mtr_scene_desc *d, const mtr_render_params *p, const float *g_s, const float *g_t,
                                  double *grad_mats, double *grad_ems, double *grad_texels, uint64_t *n_texels_out)
{
    HostScene hs;
    if (derive_scene(*d, hs)) return -1;
    if (d->nlos) return -2;
    if (n_texels_out) *n_texels_out = hs.texels.size();
    if (!grad_texels) return 0;
    std::vector<float> rad(3 * hs.ems.size() + 3, 0.0f);
    std::vector<Emitter> unit = hs.ems;
    for (size_t i = 0; i < unit.size(); ++i)
        for (int k = 0; k < 3; ++k) { rad[3 * i + k] = unit[i].radiance[k]; unit[i].radiance[k] = 1.0f; }
    SceneView sv;
    std::memset(&sv, 0, sizeof sv);
    sv.nodes = hs.nodes.data(); sv.tpairs = hs.tpairs.data(); sv.tshade = hs.tshade.data();
    sv.mats = hs.mats.data(); sv.ems = unit.data();
    sv.n_emitters = (uint32_t)hs.ems.size(); sv.n_slots = (uint32_t)hs.tshade.size();
    sv.samp_tris = hs.samp_tris.data(); sv.samp_vn = hs.samp_vn.empty() ? nullptr : hs.samp_vn.data(); sv.face_pmf = hs.face_pmf.data(); sv.face_cdf = hs.face_cdf.data();
    sv.vnormals = hs.vnormals.empty() ? nullptr : hs.vnormals.data();
    sv.texels = hs.texels.empty() ? nullptr : hs.texels.data(); sv.tex_info = hs.tex_info.empty() ? nullptr : hs.tex_info.data();
    sv.uvs = hs.uvs.empty() ? nullptr : hs.uvs.data();
    const RenderConst rc = make_render_const(*p, hs.film, sv.n_emitters);
    GradConst gc;
    gc.g_s = g_s; gc.g_t = g_t; gc.em_radiance = rad.data();
    gc.steady_scale = rc.sample_scale; gc.transient_scale = rc.sample_scale;
    const bool ext = hs.needs_ext;
    std::memset(grad_mats, 0, sizeof(double) * 3 * d->n_materials);
    std::memset(grad_ems, 0, sizeof(double) * 3 * d->n_emitters);
    std::memset(grad_texels, 0, sizeof(double) * 3 * hs.texels.size());
    HostAcc acc{ grad_mats, grad_ems };
    HostTexels tex{ grad_texels };
    ArrStack st; st.sp = 0;
    for (uint32_t pix = p->pixel_begin; pix < p->pixel_end; ++pix)
        for (uint32_t s = p->spp_begin; s < p->spp_end; ++s) {
            st.reset();
            if (ext) grad_lane<true>(sv, hs.cam, hs.film, rc, gc, pix, s, st, acc, tex);
            else grad_lane<false>(sv, hs.cam, hs.film, rc, gc, pix, s, st, acc, tex);
        }
    return 0;
}
