// host_fwd.cpp — TEST-ONLY.  The forward-mode arithmetic of mtr_render_fwd (mtr_fwd.h) compiled for the HOST and run one lane at a
// time over the same scene tables, so that the CPU tests can compare it with the CPU oracle and with the host builds of the reverse
// mode, and the GPU tests can compare the kernel with it.  Never part of libmitransient_amd.so.
#include "../mitransient_amd/csrc/mtr_core.h"
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
// the developed tangent film: every f32 term times the sample scale (as the kernel), summed in f64
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
}

// mtr_render_fwd's contract on the host: tan_texels may be NULL; steady (H, W, 3) and transient (H, W, T, 3), f64, are ZEROED and
// receive the lanes of `p`.  *n_texels_out: the number of texels (steady may be NULL to ask for it alone).
extern "C" int hf_render_fwd(const mtr_scene_desc *d, const mtr_render_params *p, const float *tan_mats, const float *tan_ems,
                             const float *tan_texels, double *steady, double *transient, uint64_t *n_texels_out)
{
    HostScene hs;
    if (derive_scene(*d, hs)) return -1;
    if (d->nlos) return -2;
    if (n_texels_out) *n_texels_out = hs.texels.size();
    if (!steady) return 0;
    if (hs.film.n_freq || hs.film.lasers > 1u) return -3;
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
    FwdConst fc;
    fc.em_radiance = rad.data(); fc.tan_mats = tan_mats; fc.tan_ems = tan_ems ? tan_ems : rad.data();
    fc.tan_texels = hs.texels.empty() ? nullptr : tan_texels;
    const size_t npix = (size_t)hs.film.width * hs.film.height;
    std::memset(steady, 0, sizeof(double) * 3 * npix);
    std::memset(transient, 0, sizeof(double) * 3 * npix * hs.film.bins);
    HostFilm sink{ &hs.film, rc.sample_scale, steady, transient };
    ArrStack st; st.sp = 0;
    for (uint32_t pix = p->pixel_begin; pix < p->pixel_end; ++pix)
        for (uint32_t s = p->spp_begin; s < p->spp_end; ++s) {
            st.reset();
            if (hs.needs_ext) fwd_lane<true>(sv, hs.cam, hs.film, rc, fc, pix, s, st, sink);
            else fwd_lane<false>(sv, hs.cam, hs.film, rc, fc, pix, s, st, sink);
        }
    return 0;
}
