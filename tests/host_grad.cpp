// host_grad.cpp — TEST-ONLY.  The gradient arithmetic of mtr_render_grad (mtr_grad.h) compiled for the HOST and run one lane at
// a time over the same scene tables, so that the CPU tests can compare it with finite differences of the CPU oracle and the GPU
// tests can compare the kernel with it.  Never part of libmitransient_amd.so.
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
// one record of the replay walk (hg_grad_records): kind 0 = a lane starts (idx = film pixel y * W + x), 1 = a vertex (idx =
// material, flag = active_next, dist = its distance), 2 = an emission, 3 = an emitter-sampling term (idx = emitter, dist = the
// term's optical path length, c = the term without its radiance factor)
struct GradRec { uint32_t kind, idx, flag, pad; float dist, c[3]; };
// f64 sums on the host, as the kernel (f64 LDS slab per workgroup, f64 over workgroups); optionally the replay's records
struct HostAcc {
    double *mats, *ems; uint32_t n_mats;
    std::vector<GradRec> *rec;
    void add_mat(uint32_t m, f3 g) { mats[3 * m] += g.x; mats[3 * m + 1] += g.y; mats[3 * m + 2] += g.z; }
    void add_em(uint32_t e, f3 g) { ems[3 * e] += g.x; ems[3 * e + 1] += g.y; ems[3 * e + 2] += g.z; }
    void vertex(uint32_t m, float dist, bool active) { if (rec) rec->push_back(GradRec{ 1u, m, active ? 1u : 0u, 0u, dist, { 0, 0, 0 } }); }
    void term(uint32_t kind, uint32_t e, float opl, f3 c) { if (rec) rec->push_back(GradRec{ 2u + kind, e, 0u, 0u, opl, { c.x, c.y, c.z } }); }
};
static std::vector<GradRec> g_rec;
}

// the gradient of the lanes of `p`; with `rec`, the replay walk's records of every lane as well
static int render_grad(const mtr_scene_desc *d, const mtr_render_params *p, const float *g_s, const float *g_t,
                       double *grad_mats, double *grad_ems, std::vector<GradRec> *rec)
{
    HostScene hs;
    if (derive_scene(*d, hs)) return -1;
    if (d->nlos) return -2;
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
    HostAcc acc{ grad_mats, grad_ems, d->n_materials, rec };
    ArrStack st; st.sp = 0;
    for (uint32_t pix = p->pixel_begin; pix < p->pixel_end; ++pix)
        for (uint32_t s = p->spp_begin; s < p->spp_end; ++s) {
            st.reset();
            if (rec) {
                const uint32_t py = pix / hs.film.crop_w, px = pix - py * hs.film.crop_w;    // film pixel of the lane (path_begin)
                rec->push_back(GradRec{ 0u, py * hs.film.width + px, 0u, 0u, 0.0f, { 0, 0, 0 } });
            }
            if (ext) grad_lane<true>(sv, hs.cam, hs.film, rc, gc, pix, s, st, acc);
            else grad_lane<false>(sv, hs.cam, hs.film, rc, gc, pix, s, st, acc);
        }
    return 0;
}

// The gradient of the lanes of `p` (mtr_render_grad's contract): grad_mats (n_materials, 3), grad_ems (n_emitters, 3), f64
extern "C" int hg_render_grad(const mtr_scene_desc *d, const mtr_render_params *p, const float *g_s, const float *g_t,
                              double *grad_mats, double *grad_ems)
{
    return render_grad(d, p, g_s, g_t, grad_mats, grad_ems, nullptr);
}

// ... and the records of every lane's replay walk (GradRec, 32 bytes each): *n_out of them, read with hg_grad_records_copy
extern "C" int hg_grad_records(const mtr_scene_desc *d, const mtr_render_params *p, const float *g_s, const float *g_t,
                               double *grad_mats, double *grad_ems, uint64_t *n_out)
{
    g_rec.clear();
    const int r = render_grad(d, p, g_s, g_t, grad_mats, grad_ems, &g_rec);
    *n_out = g_rec.size();
    return r;
}
extern "C" void hg_grad_records_copy(void *out) { std::memcpy(out, g_rec.data(), g_rec.size() * sizeof(GradRec)); }
