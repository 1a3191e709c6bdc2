// host_grad_nlos_tex.cpp — TEST-ONLY.  host_grad_nlos.cpp with the texel hook of mtr_grad.h: the NLOS gradient arithmetic of
// mtr_render_grad_tex (grad_nlos_lane over mtr_nlos.h's nlos_bounce, NlosGradTexHook) compiled for the HOST and run one lane at a
// time, so that the CPU tests can compare texel gradients with finite differences of the CPU oracle and the GPU tests can compare
// both tiers of the kernel with it.  Never part of libmitransient_amd.so.
#include "../mitransient_amd/csrc/mtr_core.h"
#include "../mitransient_amd/csrc/mtr_nlos.h"
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
// f64 sums on the host, as the kernel (f64 LDS slab per workgroup, f64 over workgroups)
struct HostAcc {
    double *mats, *laser;
    void add_mat(uint32_t m, f3 g) { mats[3 * m] += g.x; mats[3 * m + 1] += g.y; mats[3 * m + 2] += g.z; }
    void add_em(uint32_t, f3 g) { laser[0] += g.x; laser[1] += g.y; laser[2] += g.z; }
    void vertex(uint32_t, float, bool) {}
    void term(uint32_t, uint32_t, float, f3) {}
};
struct HostTexels {
    static constexpr bool kOn = true;
    double *t;
    void operator()(uint32_t i, f3 g) const { t[3 * (size_t)i] += g.x; t[3 * (size_t)i + 1] += g.y; t[3 * (size_t)i + 2] += g.z; }
};
}

// The gradient of the lanes of `p` (mtr_render_grad_tex's contract on a NLOS scene): grad_mats (n_materials, 3), grad_laser (3)
// and grad_texels (the texels of every texture in scene order, 3 each), f64.  *n_texels_out: the number of texels.  grad_texels
// NULL: the walk without a texel hook (host_grad_nlos.cpp's).
// -3: a capture or film the gradient refuses (Exhaustive, exhaustive_scan, phasor)
extern "C" int hgnt_render_grad_tex(const mtr_scene_desc *d, const mtr_render_params *p, const float *g_s, const float *g_t,
                                    double *grad_mats, double *grad_laser, double *grad_texels, uint64_t *n_texels_out)
{
    HostScene hs;
    if (derive_scene(*d, hs)) return -1;
    if (!d->nlos) return -2;
    HostNlos hn;
    if (derive_nlos(*d, hn)) return -2;
    if (hn.k.capture_type == MTR_CAPTURE_EXHAUSTIVE || hs.film.lasers > 1u || hs.film.n_freq) return -3;
    if (n_texels_out) *n_texels_out = hs.texels.size();
    SceneView sv;
    std::memset(&sv, 0, sizeof sv);
    sv.nodes = hs.nodes.data(); sv.tpairs = hs.tpairs.data(); sv.tshade = hs.tshade.data();
    sv.mats = hs.mats.data(); sv.ems = hs.ems.data();
    sv.n_emitters = (uint32_t)hs.ems.size(); sv.n_slots = (uint32_t)hs.tshade.size();
    sv.samp_tris = hs.samp_tris.data(); sv.samp_vn = hs.samp_vn.empty() ? nullptr : hs.samp_vn.data(); sv.face_pmf = hs.face_pmf.data(); sv.face_cdf = hs.face_cdf.data();
    sv.vnormals = hs.vnormals.empty() ? nullptr : hs.vnormals.data();
    sv.texels = hs.texels.empty() ? nullptr : hs.texels.data(); sv.tex_info = hs.tex_info.empty() ? nullptr : hs.tex_info.data();
    sv.uvs = hs.uvs.empty() ? nullptr : hs.uvs.data();
    ArrStack st; st.sp = 0;
    // the scanned points, as tests/host_harness.cpp derives them (the product: k_nlos_prepare)
    NlosConst &k = hn.k;
    k.shapes = hn.shapes.data(); k.shape_pmf = hn.shape_pmf.data(); k.shape_cdf = hn.shape_cdf.data();
    k.face_pmf = hn.face_pmf.data(); k.face_cdf = hn.face_cdf.data(); k.hg_tris = hn.hg_tris.data(); k.hg_vn = hn.hg_vn.empty() ? nullptr : hn.hg_vn.data();
    const uint32_t n = nlos_target_count(k);
    std::vector<q4> targets(n);
    for (uint32_t i = 0; i < n; ++i) {
        const Ray r = nlos_prepare_ray(k, i);
        const Hit h = traverse<false>(sv, r.o, r.d, r.tmax, st);
        f3 pp = mk(0, 0, 0);
        if (h.prim >= 0) pp = hit_ctx<false>(sv, r.d, h).sp;
        targets[i] = q4{ pp.x, pp.y, pp.z, 0.0f };
    }
    k.targets = targets.data();
    // the walk runs with unit irradiance; the true one goes alongside
    const float irr[3] = { k.l_irr.x, k.l_irr.y, k.l_irr.z };
    k.l_irr = mk(1, 1, 1);
    const RenderConst rc = make_render_const(*p, hs.film, sv.n_emitters);
    GradConst gc;
    gc.g_s = g_s; gc.g_t = g_t; gc.em_radiance = irr;
    gc.steady_scale = rc.sample_scale; gc.transient_scale = rc.sample_scale;
    std::memset(grad_mats, 0, sizeof(double) * 3 * d->n_materials);
    std::memset(grad_laser, 0, sizeof(double) * 3);
    if (grad_texels) std::memset(grad_texels, 0, sizeof(double) * 3 * hs.texels.size());
    HostAcc acc{ grad_mats, grad_laser };
    HostTexels tex{ grad_texels };
    for (uint32_t pix = p->pixel_begin; pix < p->pixel_end; ++pix)
        for (uint32_t s = p->spp_begin; s < p->spp_end; ++s) {
            st.reset();
            if (hs.needs_ext && grad_texels) grad_nlos_lane<true>(sv, k, hs.film, rc, gc, pix, s, st, acc, NoReload(), tex);
            else if (hs.needs_ext) grad_nlos_lane<true>(sv, k, hs.film, rc, gc, pix, s, st, acc);
            else grad_nlos_lane<false>(sv, k, hs.film, rc, gc, pix, s, st, acc);
        }
    return 0;
}
