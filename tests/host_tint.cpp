// host_tint.cpp — TEST-ONLY.  The tint hooks of mtr_grad.h / mtr_fwd.h (mtr_render_grad_tint, mtr_render_fwd_tint) compiled for the
// HOST and run one lane at a time over the same scene tables, so that the CPU tests can compare tint gradients with fits of the
// CPU oracle and the GPU tests can compare the kernels of mtr_tint.hip with it.  Never part of libmitransient_amd.so.
#include "../mitransient_amd/csrc/mtr_core.h"
#include "../mitransient_amd/csrc/mtr_grad.h"
#include "../mitransient_amd/csrc/mtr_fwd.h"
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
struct HostAcc {
    double *mats, *ems;
    void add_mat(uint32_t m, f3 g) { mats[3 * m] += g.x; mats[3 * m + 1] += g.y; mats[3 * m + 2] += g.z; }
    void add_em(uint32_t e, f3 g) { ems[3 * e] += g.x; ems[3 * e + 1] += g.y; ems[3 * e + 2] += g.z; }
    void vertex(uint32_t, float, bool) {}
    void term(uint32_t, uint32_t, float, f3) {}
};
// f64 sums per slot; the per-vertex records: vertices on a tinted material, and those whose emitter-sampling lobe and sampled lobe differ
struct HostTints {
    static constexpr bool kOn = true;
    double *t; const int32_t *slots; uint64_t *n_vertices, *n_split;
    void operator()(uint32_t m, uint32_t which, f3 g) const
    {
        const int32_t s = slots[2u * m + which];
        if (s >= 0) { t[3 * s] += g.x; t[3 * s + 1] += g.y; t[3 * s + 2] += g.z; }
    }
    void lobes(uint32_t, int nee, int sampled) const { ++*n_vertices; if (nee >= 0 && nee != sampled) ++*n_split; }
};
struct HostTintTan {
    static constexpr bool kOn = true;
    const float *tan; const int32_t *slots;
    const float *operator()(uint32_t m, uint32_t which) const { const int32_t s = slots[2u * m + which]; return s < 0 ? nullptr : tan + 3 * s; }
};
struct HostFilm {
    const Film *film; float scale;
    double *steady_out, *transient;      // (H, W, 3), (H, W, T, 3)
    void add(double *p, f3 v) const { p[0] += v.x; p[1] += v.y; p[2] += v.z; }
    void splat(uint32_t fx, uint32_t fy, float opl, f3 dc) const
    {
        if (!((fx < film->width) & (fy < film->height))) return;
        const int32_t bin = film_bin(*film, opl);
        if (bin >= 0) add(transient + 3u * (((size_t)fy * film->width + fx) * film->bins + (uint32_t)bin), mk(dc.x * scale, dc.y * scale, dc.z * scale));
    }
    void steady(uint32_t fx, uint32_t fy, f3 sum) const
    {
        if (!((fx < film->width) & (fy < film->height))) return;
        add(steady_out + 3u * ((size_t)fy * film->width + fx), mk(sum.x * scale, sum.y * scale, sum.z * scale));
    }
};
// the scene tables as the kernels see them, with unit radiance in the emitter table
struct HostView {
    HostScene hs; std::vector<float> rad; std::vector<Emitter> unit; std::vector<int32_t> slots; uint32_t n_tints; SceneView sv;
    int init(const mtr_scene_desc *d)
    {
        if (derive_scene(*d, hs)) return -1;
        if (d->nlos) return -2;
        rad.assign(3 * hs.ems.size() + 3, 0.0f);
        unit = hs.ems;
        for (size_t i = 0; i < unit.size(); ++i)
            for (int k = 0; k < 3; ++k) { rad[3 * i + k] = unit[i].radiance[k]; unit[i].radiance[k] = 1.0f; }
        slots.assign(2 * hs.mats.size() + 2, -1);
        n_tints = tint_slot_table(hs.mats.data(), (uint32_t)hs.mats.size(), slots.data());
        std::memset(&sv, 0, sizeof sv);
        sv.nodes = hs.nodes.data(); sv.tpairs = hs.tpairs.data(); sv.tshade = hs.tshade.data();
        sv.mats = hs.mats.data(); sv.ems = unit.data();
        sv.n_emitters = (uint32_t)hs.ems.size(); sv.n_slots = (uint32_t)hs.tshade.size();
        sv.samp_tris = hs.samp_tris.data(); sv.samp_vn = hs.samp_vn.empty() ? nullptr : hs.samp_vn.data(); sv.face_pmf = hs.face_pmf.data(); sv.face_cdf = hs.face_cdf.data();
        sv.vnormals = hs.vnormals.empty() ? nullptr : hs.vnormals.data();
        sv.texels = hs.texels.empty() ? nullptr : hs.texels.data(); sv.tex_info = hs.tex_info.empty() ? nullptr : hs.tex_info.data();
        sv.uvs = hs.uvs.empty() ? nullptr : hs.uvs.data();
        return 0;
    }
};
}

// mtr_scene_tint_layout on the host: *n_slots, and (when not NULL) the material and 0 | 1 of every slot
extern "C" int ht_tint_layout(const mtr_scene_desc *d, uint32_t *n_slots, uint32_t *slot_material, uint32_t *slot_which)
{
    std::vector<int32_t> slots(2 * (size_t)d->n_materials + 2, -1);
    *n_slots = tint_slot_table(d->materials, d->n_materials, slots.data());
    for (size_t i = 0; i < 2 * (size_t)d->n_materials; ++i)
        if (slots[i] >= 0) {
            if (slot_material) slot_material[slots[i]] = (uint32_t)(i / 2);
            if (slot_which) slot_which[slots[i]] = (uint32_t)(i & 1);
        }
    return 0;
}

// mtr_render_grad_tint's contract on the host (no texels): grad_mats (n_materials, 3), grad_ems (n_emitters, 3), grad_tints (n_slots, 3),
// f64; grad_tints NULL: the walk without the tint hook (mtr_render_grad).  counts (may be NULL): [0] vertices on a tinted material,
// [1] those whose emitter-sampling term carries another tint than the continued path
extern "C" int ht_render_grad_tint(const mtr_scene_desc *d, const mtr_render_params *p, const float *g_s, const float *g_t,
                                   double *grad_mats, double *grad_ems, double *grad_tints, uint64_t *counts)
{
    HostView v;
    if (int r = v.init(d)) return r;
    const RenderConst rc = make_render_const(*p, v.hs.film, v.sv.n_emitters);
    GradConst gc;
    gc.g_s = g_s; gc.g_t = g_t; gc.em_radiance = v.rad.data();
    gc.steady_scale = rc.sample_scale; gc.transient_scale = rc.sample_scale;
    std::memset(grad_mats, 0, sizeof(double) * 3 * d->n_materials);
    std::memset(grad_ems, 0, sizeof(double) * 3 * d->n_emitters);
    if (grad_tints) std::memset(grad_tints, 0, sizeof(double) * 3 * v.n_tints);
    uint64_t cnt[2] = { 0, 0 };
    HostAcc acc{ grad_mats, grad_ems };
    const HostTints tint{ grad_tints, v.slots.data(), &cnt[0], &cnt[1] };
    ArrStack st; st.sp = 0;
    for (uint32_t pix = p->pixel_begin; pix < p->pixel_end; ++pix)
        for (uint32_t s = p->spp_begin; s < p->spp_end; ++s) {
            st.reset();
            if (!grad_tints) {
                if (v.hs.needs_ext) grad_lane<true>(v.sv, v.hs.cam, v.hs.film, rc, gc, pix, s, st, acc);
                else grad_lane<false>(v.sv, v.hs.cam, v.hs.film, rc, gc, pix, s, st, acc);
            } else if (v.hs.needs_ext) grad_lane<true>(v.sv, v.hs.cam, v.hs.film, rc, gc, pix, s, st, acc, NoTexelGrad(), tint);
            else grad_lane<false>(v.sv, v.hs.cam, v.hs.film, rc, gc, pix, s, st, acc, NoTexelGrad(), tint);
        }
    if (counts) { counts[0] = cnt[0]; counts[1] = cnt[1]; }
    return 0;
}

// mtr_render_fwd_tint's contract on the host: tan_texels and tan_tints may be NULL; steady (H, W, 3) and transient (H, W, T, 3), f64,
// are ZEROED and receive the lanes of `p`
extern "C" int ht_render_fwd_tint(const mtr_scene_desc *d, const mtr_render_params *p, const float *tan_mats, const float *tan_ems,
                                  const float *tan_texels, const float *tan_tints, double *steady, double *transient)
{
    HostView v;
    if (int r = v.init(d)) return r;
    if (v.hs.film.n_freq || v.hs.film.lasers > 1u) return -3;
    const RenderConst rc = make_render_const(*p, v.hs.film, v.sv.n_emitters);
    FwdConst fc;
    fc.em_radiance = v.rad.data(); fc.tan_mats = tan_mats; fc.tan_ems = tan_ems ? tan_ems : v.rad.data();
    fc.tan_texels = v.hs.texels.empty() ? nullptr : tan_texels;
    const size_t npix = (size_t)v.hs.film.width * v.hs.film.height;
    std::memset(steady, 0, sizeof(double) * 3 * npix);
    std::memset(transient, 0, sizeof(double) * 3 * npix * v.hs.film.bins);
    HostFilm sink{ &v.hs.film, rc.sample_scale, steady, transient };
    const HostTintTan tint{ tan_tints, v.slots.data() };
    ArrStack st; st.sp = 0;
    for (uint32_t pix = p->pixel_begin; pix < p->pixel_end; ++pix)
        for (uint32_t s = p->spp_begin; s < p->spp_end; ++s) {
            st.reset();
            if (!tan_tints) {
                if (v.hs.needs_ext) fwd_lane<true>(v.sv, v.hs.cam, v.hs.film, rc, fc, pix, s, st, sink);
                else fwd_lane<false>(v.sv, v.hs.cam, v.hs.film, rc, fc, pix, s, st, sink);
            } else if (v.hs.needs_ext) fwd_lane<true>(v.sv, v.hs.cam, v.hs.film, rc, fc, pix, s, st, sink, tint);
            else fwd_lane<false>(v.sv, v.hs.cam, v.hs.film, rc, fc, pix, s, st, sink, tint);
        }
    return 0;
}
