// mtr_api.hip — the C-ABI of include/mitransient_amd.h.
//
// Host side of the library: scene ingestion (derived per-triangle frames, emitter normals,
// BVH2 build, upload), render planning and launches, film develop/clear, the stand-alone
// scatter-add.  There is no CPU execution path: without a HIP device every entry point fails.
#include "../../include/mitransient_amd.h"
#include "mtr_knobs.h"
#include "mtr_scene_host.h"
#include "mtr_core.h"
#include "mtr_kernels.h"
#include "mtr_polar.h"
#include "mtr_grad.h"
#include "mtr_fwd_args.h"
#include "mtr_tint_args.h"
#include "mtr_samples_args.h"
#include "mtr_backproject.h"
#include "mtr_forward_project.h"
#include "mtr_phasor_backproject.h"
#include "mtr_phasor_forward_project.h"
#include "mtr_fk.h"

#include <hip/hip_runtime.h>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>
#include <algorithm>
#include <utility>

using namespace mtr;

struct mtr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    std::string err;
    DevCounters *d_counters = nullptr;
    uint32_t *d_ticket = nullptr;          // work-ticket counters: [0, 16) k_fused launches in rotation (launches of consecutive
                                           // row bands may overlap on two streams: each needs its own), [16, 18) wavefront segments
    uint32_t fused_launches = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev2 = nullptr, ev3 = nullptr;               // mtr_splat_add: the partitioned passes, timed apart from the first pass (the workspace allocation in between is host time)
    float *d_freq = nullptr; size_t freq_cap = 0;        // phasor film frequencies of a ctx-level call (mtr_splat_add); capacities in bytes (grow_device_buffer)
    void *d_runs = nullptr; size_t runs_cap = 0;         // mtr_splat_add variant 1: sortedness flag + run table
    uint32_t *d_band_count = nullptr; size_t band_cap = 0;       // mtr_render_params.n_bands: flushed pixels per band of the launch in flight
    void *d_part = nullptr; size_t part_cap = 0;         // ... and the partition workspace of unsorted input (at most 256 MiB of it kept between calls, until mtr_ctx_trim / destroy)
    void *d_samples = nullptr; size_t samples_cap = 0;   // MTR_MODE_SAMPLES: the slabs' rows (at most 256 MiB kept between calls, until mtr_ctx_trim / destroy)
    void *d_start = nullptr; size_t start_cap = 0;       // k_fused's lean kernels: kStartSlots path-start tables (mtr_start_blocks.h), one per ticket counter of the rotation (until mtr_ctx_trim / destroy)
    void *d_bp = nullptr; size_t bp_cap = 0;             // mtr_backproject / mtr_forward_project / mtr_phasor_backproject / mtr_phasor_forward_project: the slabs' planes of a call with few voxels and many pairs (few rows and many voxels), the weighted rows of a phasor call (until mtr_ctx_trim / destroy)
};

struct WfWorkspace {            // MTR_MODE_WAVEFRONT buffers, sized for one tile, reused across renders
    void *planes = nullptr, *q_live = nullptr, *q_ray = nullptr, *q_mat = nullptr, *r_shadow = nullptr, *occ = nullptr, *counts = nullptr, *rec = nullptr, *rec_count = nullptr, *q_zombie = nullptr;
    uint32_t n_slots = 0, P = 0, rec_cap = 0, rows = 0;
    size_t bytes = 0;                    // of the device buffers together (WfBytes::total)
    bool polar = false;                  // `planes` also holds the polarized planes (wf_polar_planes_bytes) behind the ordinary ones
    uint32_t *host_count = nullptr;       // pinned: live counts read back between bounce chunks (two words, alternating)
    hipEvent_t poll_ev[2] = { nullptr, nullptr };     // ... and the events that say a word has landed
    void release()              // the tile's device buffers; the sizes are valid only while every one of them exists
    {
        n_slots = 0; P = 0; rec_cap = 0; rows = 0; bytes = 0; polar = false;
        for (void **p : { &planes, &q_live, &q_ray, &q_mat, &r_shadow, &occ, &counts, &rec, &rec_count, &q_zombie })
            if (*p) { (void)hipFree(*p); *p = nullptr; }
    }
};

struct NlosDev {                // NLOS tier: device tables + constants (mtr_scene_set_nlos)
    bool on = false;
    NlosConst k{};
    void *shapes = nullptr, *tables = nullptr, *hg_tris = nullptr, *hg_vn = nullptr, *targets = nullptr;
    std::vector<mtr_shape> host_shapes;      // kept: the triangle -> shape table of the scene
};

struct mtr_scene {
    mtr_ctx *ctx = nullptr;
    WfWorkspace wf;
    NlosDev nlos;
    std::vector<float> tri_verts;            // host copy (NLOS tables are re-derived when the laser moves)
    std::vector<float> tri_normals;          // ... and the vertex normals (empty without): Mesh::sample_position on hidden meshes
    uint32_t n_emitters_area = 0;
    bool polar_ok = false;                                   // every material and emitter has a polarized form (mtr_polar.h)
    bool grey_scene = false;                                 // kTrGrey without the NLOS laser (mtr_scene_set_nlos decides with it)
    bool has_sphere = false;                                 // an analytic sphere: never kTrGrey (mtr_core.h tr_spheres)
    SceneDev dev{};
    Camera cam{};
    Film film{};
    mtr_film_desc film_desc{};
    float *d_freq = nullptr;               // phasor film: device copy of film_desc.frequencies
    std::vector<float> h_freq;
    uint32_t n_leaves = 0;
    std::vector<q4> tex_info;                // host copy of dev.tex_info: (first texel, width, height, -) per texture
    uint32_t n_texels = 0;                   // texels of all textures (mtr_render_grad_tex's grad_texels)
    std::vector<void *> allocs;
    SplatLog log{ nullptr, 0, nullptr };
    ShadowHull hull{};                       // SHADOW HULL (mtr_shadow_hull.h): classify_scene's block; a render applies its margin (FusedArgs::hull)
};

static thread_local std::string g_err;

static int fail(mtr_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_err = msg;
    return code;
}
// CUs the persistent fused kernel may occupy (mtr_render_params.reserve_cus: the rest stays free for other streams' kernels)
static int usable_cus(const mtr_ctx *c, const mtr_render_params *p)
{
    const int keep = (int)std::min<uint32_t>(p->reserve_cus, (uint32_t)(c->n_cu > 1 ? c->n_cu - 1 : 0));
    return c->n_cu - keep;
}

#define HIP_TRY(c, expr)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((c), e_ == hipErrorOutOfMemory ? MTR_ERR_OOM : MTR_ERR_HIP,             \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                     \
    } while (0)

extern "C" {

int mtr_abi_version(void) { return MTR_ABI_VERSION; }

const char *mtr_last_error(const mtr_ctx *c) { return c ? c->err.c_str() : g_err.c_str(); }

int mtr_ctx_create(int device_ordinal, mtr_ctx **out)
{
    if (!out) return fail(nullptr, MTR_ERR_INVALID, "mtr_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(nullptr, MTR_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU path");
    if (device_ordinal < 0 || device_ordinal >= n)
        return fail(nullptr, MTR_ERR_INVALID, "mtr_ctx_create: device ordinal out of range");
    mtr_ctx *c = new mtr_ctx();
    c->device = device_ordinal;
    HIP_TRY(nullptr, hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_ordinal));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(nullptr, hipMalloc((void **)&c->d_counters, sizeof(DevCounters)));
    HIP_TRY(nullptr, hipMalloc((void **)&c->d_ticket, 32 * sizeof(uint32_t)));
    for (hipEvent_t *e : { &c->ev0, &c->ev1, &c->ev2, &c->ev3 }) HIP_TRY(nullptr, hipEventCreate(e));
    *out = c;
    return MTR_OK;
}

void mtr_ctx_destroy(mtr_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (void *p : { (void *)c->d_counters, (void *)c->d_ticket, (void *)c->d_freq, c->d_runs, c->d_part, c->d_samples, c->d_start, c->d_bp, (void *)c->d_band_count }) if (p) (void)hipFree(p);
    for (hipEvent_t e : { c->ev0, c->ev1, c->ev2, c->ev3 }) if (e) (void)hipEventDestroy(e);
    delete c;
}

int mtr_ctx_set_stream(mtr_ctx *c, void *s)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_ctx_set_stream: ctx is NULL");
    c->stream = (hipStream_t)s;
    return MTR_OK;
}

} // extern "C"

static int check_film(mtr_ctx *c, const mtr_film_desc &d)
{
    if (d.width == 0 || d.height == 0 || d.temporal_bins == 0)
        return fail(c, MTR_ERR_INVALID, "film: width, height and temporal_bins must be positive");
    if (d.crop_width == 0 || d.crop_height == 0 || d.crop_offset_x + d.crop_width > d.width ||
        d.crop_offset_y + d.crop_height > d.height)
        return fail(c, MTR_ERR_INVALID, "film: invalid crop window");
    if (!(d.bin_width_opl > 0.0f)) return fail(c, MTR_ERR_INVALID, "film: bin_width_opl must be > 0");
    if (d.n_frequencies && !d.frequencies) return fail(c, MTR_ERR_INVALID, "film: n_frequencies > 0 but frequencies is NULL");
    if (d.n_frequencies && (d.laser_scan_width || d.laser_scan_height))
        return fail(c, MTR_ERR_INVALID, "film: a phasor film cannot be an exhaustive_scan film");
    if (d.n_frequencies > (1u << 20)) return fail(c, MTR_ERR_INVALID, "film: too many frequencies");
    if ((d.laser_scan_width == 0) != (d.laser_scan_height == 0))
        return fail(c, MTR_ERR_INVALID, "film: laser_scan_width and laser_scan_height must both be set (exhaustive_scan) or both be 0");
    if ((uint64_t)d.temporal_bins * (d.laser_scan_width ? d.laser_scan_width : 1u) * (d.laser_scan_height ? d.laser_scan_height : 1u) > 0x7fffffffull)
        return fail(c, MTR_ERR_INVALID, "film: laser_scan_width * laser_scan_height * temporal_bins exceeds 2^31");
    return MTR_OK;
}

template <class T>
static int upload(mtr_scene *s, const std::vector<T> &v, const T **out)
{
    size_t bytes = ((v.size() * sizeof(T) + 15) / 16) * 16;
    if (bytes == 0) bytes = 16;
    void *p = nullptr;
    HIP_TRY(s->ctx, hipMalloc(&p, bytes));
    s->allocs.push_back(p);
    HIP_TRY(s->ctx, hipMemset(p, 0, bytes));
    if (!v.empty()) HIP_TRY(s->ctx, hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T *)p;
    return MTR_OK;
}

extern "C" {

static int scene_take_film(mtr_scene *s, const mtr_film_desc &f);

int mtr_scene_create(mtr_ctx *c, const mtr_scene_desc *d, mtr_scene **out)
{
    if (!c || !d || !out) return fail(c, MTR_ERR_INVALID, "mtr_scene_create: NULL argument");
    *out = nullptr;
    int rc = check_film(c, d->film);
    if (rc) return rc;
    HostScene hs;
    if (const char *msg = derive_scene(*d, hs)) return fail(c, MTR_ERR_INVALID, std::string("mtr_scene_create: ") + msg);
    HIP_TRY(c, hipSetDevice(c->device));

    mtr_scene *s = new mtr_scene();
    s->ctx = c;
    s->cam = hs.cam;
    rc = scene_take_film(s, d->film);
    if (rc) { delete s; return rc; }

#define UP(vec, field)                                                       \
    do { rc = upload(s, vec, &s->dev.field); if (rc) { mtr_scene_destroy(s); return rc; } } while (0)
    UP(hs.nodes, nodes); UP(hs.tpairs, tpairs); UP(hs.tshade, tshade); UP(hs.mats, mats); UP(hs.ems, ems);
    // (optional tables stay null: `dev` starts zeroed)
    s->dev.n_wnodes = (uint32_t)hs.wnodes.size(); s->dev.n_wnodes4 = (uint32_t)hs.wnodes4.size(); s->dev.n_wnodes8q = (uint32_t)hs.wnodes8q.size();
    if (hs.has_wide) UP(hs.wnodes, wnodes);
    UP(hs.wnodes4, wnodes4);
    if (!hs.wnodes8q.empty()) UP(hs.wnodes8q, wnodes8q);
    if (!hs.samp_tris.empty()) { UP(hs.samp_tris, samp_tris); UP(hs.face_pmf, face_pmf); UP(hs.face_cdf, face_cdf); }
    if (!hs.samp_vn.empty()) UP(hs.samp_vn, samp_vn);
    if (!hs.vnormals.empty()) UP(hs.vnormals, vnormals);
    if (!hs.texels.empty()) { UP(hs.texels, texels); UP(hs.tex_info, tex_info); UP(hs.uvs, uvs); }
#undef UP
    s->tex_info = hs.tex_info; s->n_texels = (uint32_t)hs.texels.size();
    s->dev.n_nodes = (uint32_t)hs.nodes.size(); s->dev.n_slots = (uint32_t)hs.tshade.size();
    s->dev.n_mats = d->n_materials; s->dev.n_ems = d->n_emitters;
    // what the kernels are chosen by: decided over the host tables (mtr_scene_host.cpp classify_scene)
    s->polar_ok = hs.polar_ok; s->grey_scene = hs.grey_scene; s->has_sphere = hs.has_sphere;
    s->dev.has_rough = hs.needs_ext ? 1u : 0u; s->dev.traits = hs.traits; s->dev.flat = hs.flat; s->hull = hs.hull;
    s->dev.bvh_depth = hs.bvh_depth; s->n_leaves = hs.n_leaves;
    s->dev.wide_levels = hs.wide_levels; s->dev.wide4_levels = hs.wide4_levels; s->dev.wide8q_levels = hs.wide8q_levels;
    s->tri_verts.assign(d->tri_verts, d->tri_verts + 9 * (size_t)d->n_tris);
    if (d->tri_normals) s->tri_normals.assign(d->tri_normals, d->tri_normals + 9 * (size_t)d->n_tris);
    s->n_emitters_area = d->n_emitters;
    if (d->nlos) {
        rc = mtr_scene_set_nlos(s, d->nlos);
        if (rc) { mtr_scene_destroy(s); return rc; }
    }
    *out = s;
    return MTR_OK;
}

int mtr_scene_set_nlos(mtr_scene *s, const mtr_nlos_desc *n)
{
    if (!s || !n) return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_scene_set_nlos: NULL argument");
    mtr_ctx *c = s->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    mtr_scene_desc d{};
    d.n_tris = (uint32_t)(s->tri_verts.size() / 9); d.tri_verts = s->tri_verts.data(); d.n_emitters = s->n_emitters_area;
    d.tri_normals = s->tri_normals.empty() ? nullptr : s->tri_normals.data();
    d.film = s->film_desc;
    memcpy(d.camera.sample_to_camera, s->cam.s2c, sizeof s->cam.s2c);
    memcpy(d.camera.to_world, s->cam.tw, sizeof s->cam.tw);
    d.camera.near_clip = s->cam.near_clip; d.camera.far_clip = s->cam.far_clip;
    d.nlos = n;
    if (d.film.n_frequencies && n->capture_type == MTR_CAPTURE_EXHAUSTIVE)
        return fail(c, MTR_ERR_UNSUPPORTED, "mtr_scene_set_nlos: an Exhaustive capture (MTR_CAPTURE_EXHAUSTIVE) is not available with a phasor_hdr_film");
    HostNlos hn;
    if (const char *msg = derive_nlos(d, hn)) return fail(c, MTR_ERR_INVALID, std::string("mtr_scene_set_nlos: ") + msg);
    NlosDev &D = s->nlos;
    void **old[] = { &D.shapes, &D.tables, &D.hg_tris, &D.hg_vn, &D.targets };
    for (void **p : old) if (*p) { (void)hipFree(*p); *p = nullptr; }
    const size_t ns = hn.shapes.size(), nt = hn.face_pmf.size();
    HIP_TRY(c, hipMalloc(&D.shapes, ns * sizeof(NlosShape)));
    HIP_TRY(c, hipMemcpy(D.shapes, hn.shapes.data(), ns * sizeof(NlosShape), hipMemcpyHostToDevice));
    std::vector<float> tab;                                       // shape_pmf | shape_cdf | face_pmf | face_cdf
    tab.insert(tab.end(), hn.shape_pmf.begin(), hn.shape_pmf.end());
    tab.insert(tab.end(), hn.shape_cdf.begin(), hn.shape_cdf.end());
    tab.insert(tab.end(), hn.face_pmf.begin(), hn.face_pmf.end());
    tab.insert(tab.end(), hn.face_cdf.begin(), hn.face_cdf.end());
    HIP_TRY(c, hipMalloc(&D.tables, tab.size() * 4));
    HIP_TRY(c, hipMemcpy(D.tables, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMalloc(&D.hg_tris, hn.hg_tris.size() * sizeof(q4)));
    HIP_TRY(c, hipMemcpy(D.hg_tris, hn.hg_tris.data(), hn.hg_tris.size() * sizeof(q4), hipMemcpyHostToDevice));
    if (!hn.hg_vn.empty()) {
        HIP_TRY(c, hipMalloc(&D.hg_vn, hn.hg_vn.size() * sizeof(q4)));
        HIP_TRY(c, hipMemcpy(D.hg_vn, hn.hg_vn.data(), hn.hg_vn.size() * sizeof(q4), hipMemcpyHostToDevice));
    }
    const size_t n_targets = nlos_target_count(hn.k);
    HIP_TRY(c, hipMalloc(&D.targets, n_targets * sizeof(q4)));
    D.k = hn.k;
    D.k.shapes = (const NlosShape *)D.shapes;
    D.k.shape_pmf = (const float *)D.tables; D.k.shape_cdf = D.k.shape_pmf + ns;
    D.k.face_pmf = D.k.shape_cdf + ns; D.k.face_cdf = D.k.face_pmf + nt;
    D.k.hg_tris = (const q4 *)D.hg_tris; D.k.hg_vn = (const q4 *)D.hg_vn; D.k.targets = (const q4 *)D.targets;
    HIP_TRY(c, launch_nlos_prepare(s->dev, D.k, (q4 *)D.targets, c->stream));    // scanned points + laser axis hit
    D.on = true;
    s->dev.traits = traits_with_laser(s->dev.traits, s->grey_scene, n->laser_irradiance);
    return MTR_OK;
}

void mtr_scene_destroy(mtr_scene *s)
{
    if (!s) return;
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    for (void *p : s->allocs) (void)hipFree(p);
    s->wf.release();
    if (s->wf.host_count) (void)hipHostFree(s->wf.host_count);
    for (hipEvent_t e : s->wf.poll_ev) if (e) (void)hipEventDestroy(e);
    void *nl[] = { s->nlos.shapes, s->nlos.tables, s->nlos.hg_tris, s->nlos.hg_vn, s->nlos.targets, s->d_freq };
    for (void *p : nl) if (p) (void)hipFree(p);
    delete s;
}

// the scene keeps its own host + device copy of a phasor film's frequencies (the caller's array need not outlive the call)
static int scene_take_film(mtr_scene *s, const mtr_film_desc &f)
{
    mtr_ctx *c = s->ctx;
    s->film = film_from_desc(f);
    s->film_desc = f;
    s->film.freq = nullptr; s->film_desc.frequencies = nullptr;
    if (f.n_frequencies) {
        const std::vector<float> nf(f.frequencies, f.frequencies + f.n_frequencies);
        if (nf != s->h_freq || !s->d_freq) {
            HIP_TRY(c, hipSetDevice(c->device));
            if (s->d_freq) { HIP_TRY(c, hipStreamSynchronize(c->stream)); (void)hipFree(s->d_freq); s->d_freq = nullptr; }
            HIP_TRY(c, hipMalloc((void **)&s->d_freq, nf.size() * 4));
            HIP_TRY(c, hipMemcpy(s->d_freq, nf.data(), nf.size() * 4, hipMemcpyHostToDevice));
            s->h_freq = nf;
        }
        s->film.freq = s->d_freq; s->film_desc.frequencies = s->h_freq.data();
    }
    return MTR_OK;
}

int mtr_scene_set_film(mtr_scene *s, const mtr_film_desc *f)
{
    if (!s || !f) return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_scene_set_film: NULL argument");
    int rc = check_film(s->ctx, *f);
    if (rc) return rc;
    return scene_take_film(s, *f);
}

int mtr_scene_bvh_info(const mtr_scene *s, uint32_t *n_nodes, uint32_t *max_depth, uint32_t *n_leaves)
{
    if (!s) return MTR_ERR_INVALID;
    if (n_nodes) *n_nodes = s->dev.n_nodes;
    if (max_depth) *max_depth = s->dev.bvh_depth;
    if (n_leaves) *n_leaves = s->n_leaves;
    return MTR_OK;
}

int mtr_scene_set_colors(mtr_scene *s, const float *material_a, const float *emitter_radiance)
{
    if (!s || (s->dev.n_mats && !material_a) || (s->dev.n_ems && !emitter_radiance))
        return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_scene_set_colors: NULL argument");
    mtr_ctx *c = s->ctx;
    if (s->nlos.on) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_scene_set_colors: not for the NLOS tier (its laser enters the scene's traits)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // (renders in flight read the tables)
    std::vector<mtr_material> mats(s->dev.n_mats);
    std::vector<Emitter> ems(s->dev.n_ems);
    if (!mats.empty()) HIP_TRY(c, hipMemcpy(mats.data(), s->dev.mats, mats.size() * sizeof(mtr_material), hipMemcpyDeviceToHost));
    if (!ems.empty()) HIP_TRY(c, hipMemcpy(ems.data(), s->dev.ems, ems.size() * sizeof(Emitter), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < mats.size(); ++i) for (int k = 0; k < 3; ++k) mats[i].a[k] = material_a[3 * i + k];
    for (size_t i = 0; i < ems.size(); ++i) for (int k = 0; k < 3; ++k) ems[i].radiance[k] = emitter_radiance[3 * i + k];
    if (!mats.empty()) HIP_TRY(c, hipMemcpy((void *)s->dev.mats, mats.data(), mats.size() * sizeof(mtr_material), hipMemcpyHostToDevice));
    if (!ems.empty()) HIP_TRY(c, hipMemcpy((void *)s->dev.ems, ems.data(), ems.size() * sizeof(Emitter), hipMemcpyHostToDevice));
    // kTrGrey is the only trait that depends on colours: decided again over the new tables
    const bool grey = scene_is_grey(s->has_sphere, mats.data(), (uint32_t)mats.size(), ems.data(), (uint32_t)ems.size(), s->dev.texels != nullptr);
    s->grey_scene = grey;
    s->dev.traits = grey ? (s->dev.traits | kTrGrey) : (s->dev.traits & ~kTrGrey);
    return MTR_OK;
}

int mtr_scene_set_tints(mtr_scene *s, const float *material_c, const float *material_c2)
{
    if (!s || (s->dev.n_mats && (!material_c || !material_c2)))
        return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_scene_set_tints: NULL argument");
    mtr_ctx *c = s->ctx;
    if (s->nlos.on) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_scene_set_tints: not for the NLOS tier");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // (renders in flight read the tables)
    std::vector<mtr_material> mats(s->dev.n_mats);
    std::vector<Emitter> ems(s->dev.n_ems);
    std::vector<int32_t> slots(2u * mats.size() + 2u, -1);
    if (!mats.empty()) HIP_TRY(c, hipMemcpy(mats.data(), s->dev.mats, mats.size() * sizeof(mtr_material), hipMemcpyDeviceToHost));
    if (!ems.empty()) HIP_TRY(c, hipMemcpy(ems.data(), s->dev.ems, ems.size() * sizeof(Emitter), hipMemcpyDeviceToHost));
    tint_slot_table(mats.data(), (uint32_t)mats.size(), slots.data());
    for (size_t i = 0; i < mats.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            if (slots[2u * i] >= 0) mats[i].c[k] = material_c[3 * i + k];
            if (slots[2u * i + 1u] >= 0) mats[i].c2[k] = material_c2[3 * i + k];
        }
    if (!mats.empty()) HIP_TRY(c, hipMemcpy((void *)s->dev.mats, mats.data(), mats.size() * sizeof(mtr_material), hipMemcpyHostToDevice));
    const bool grey = scene_is_grey(s->has_sphere, mats.data(), (uint32_t)mats.size(), ems.data(), (uint32_t)ems.size(), s->dev.texels != nullptr);
    s->grey_scene = grey;
    s->dev.traits = grey ? (s->dev.traits | kTrGrey) : (s->dev.traits & ~kTrGrey);
    return MTR_OK;
}

int mtr_scene_tint_layout(const mtr_scene *s, uint32_t *n_slots, uint32_t *slot_material, uint32_t *slot_which)
{
    if (!s || !n_slots) return MTR_ERR_INVALID;
    mtr_ctx *c = s->ctx;
    std::vector<mtr_material> mats(s->dev.n_mats);
    std::vector<int32_t> slots(2u * mats.size() + 2u, -1);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!mats.empty()) HIP_TRY(c, hipMemcpy(mats.data(), s->dev.mats, mats.size() * sizeof(mtr_material), hipMemcpyDeviceToHost));
    *n_slots = s->nlos.on ? 0u : tint_slot_table(mats.data(), (uint32_t)mats.size(), slots.data());
    if (!s->nlos.on)
        for (size_t i = 0; i < 2u * mats.size(); ++i)
            if (slots[i] >= 0) {
                if (slot_material) slot_material[slots[i]] = (uint32_t)(i / 2u);
                if (slot_which) slot_which[slots[i]] = (uint32_t)(i & 1u);
            }
    return MTR_OK;
}

int mtr_scene_set_texture(mtr_scene *s, uint32_t index, const float *rgb)
{
    if (!s || !rgb) return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_scene_set_texture: NULL argument");
    mtr_ctx *c = s->ctx;
    if (index >= s->tex_info.size()) return fail(c, MTR_ERR_INVALID, "mtr_scene_set_texture: unknown texture");
    if (s->nlos.on) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_scene_set_texture: not for the NLOS tier");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // (renders in flight read the tables)
    const q4 info = s->tex_info[index];
    const size_t first = fbits(info.x), n = (size_t)fbits(info.y) * fbits(info.z);
    std::vector<q4> tx(n);
    for (size_t k = 0; k < n; ++k) tx[k] = q4{ rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2], 0.0f };
    HIP_TRY(c, hipMemcpy((void *)(s->dev.texels + first), tx.data(), n * sizeof(q4), hipMemcpyHostToDevice));
    // the mean colour stands in as `a` of the materials on this bitmap, as the scene builder computes it (f32 texels, f64 sum)
    double mean[3] = { 0.0, 0.0, 0.0 };
    for (size_t k = 0; k < n; ++k) for (int j = 0; j < 3; ++j) mean[j] += (double)rgb[3 * k + j];
    std::vector<mtr_material> mats(s->dev.n_mats);
    if (!mats.empty()) HIP_TRY(c, hipMemcpy(mats.data(), s->dev.mats, mats.size() * sizeof(mtr_material), hipMemcpyDeviceToHost));
    for (mtr_material &m : mats)
        if (m.albedo_texture == index + 1u) for (int j = 0; j < 3; ++j) m.a[j] = (float)(mean[j] / (double)n);
    if (!mats.empty()) HIP_TRY(c, hipMemcpy((void *)s->dev.mats, mats.data(), mats.size() * sizeof(mtr_material), hipMemcpyHostToDevice));
    return MTR_OK;
}

int mtr_scene_texture_layout(const mtr_scene *s, uint32_t index, uint32_t *first_texel, uint32_t *width, uint32_t *height)
{
    if (!s || index > s->tex_info.size()) return MTR_ERR_INVALID;
    const bool end = index == s->tex_info.size();
    if (first_texel) *first_texel = end ? s->n_texels : fbits(s->tex_info[index].x);
    if (width) *width = end ? 0u : fbits(s->tex_info[index].y);
    if (height) *height = end ? 0u : fbits(s->tex_info[index].z);
    return MTR_OK;
}

int mtr_render_grad_tex_tier(const mtr_scene *s, uint32_t *tier)
{
    if (!s || !tier) return MTR_ERR_INVALID;
    *tier = grad_tex_tier(s->dev, s->n_texels, s->nlos.on);
    return MTR_OK;
}

int mtr_scene_traits(const mtr_scene *s, uint32_t *traits)
{
    if (!s || !traits) return MTR_ERR_INVALID;
    static_assert(MTR_TRAIT_DIFFUSE == kTrDiffuse && MTR_TRAIT_ONE_RECT_EMITTER == kTrOneRectEmitter && MTR_TRAIT_LEAF_PAIR == kTrLeafPair &&
                  MTR_TRAIT_FLAT_TOP == kTrFlatTop && MTR_TRAIT_FLAT_LEAVES == kTrFlatLeaves && MTR_TRAIT_NO_LOBES == kTrNoLobes &&
                  MTR_TRAIT_GREY == kTrGrey, "public trait bits");
    *traits = s->dev.traits;
    return MTR_OK;
}

int mtr_scene_shadow_hull(const mtr_scene *s, uint32_t *n_hull_rectangles)
{
    if (!s || !n_hull_rectangles) return MTR_ERR_INVALID;
    *n_hull_rectangles = s->hull.count;
    return MTR_OK;
}

// test hook, outside the C ABI of include/mitransient_amd.h (declared in mtr_kernels.h): the scene's device tables and its SHADOW HULL
// block as classify_scene left it, for mtr_walk_kat.hip — struct mtr_scene is private to this file
int mtr_test_scene_dev(const mtr_scene *s, SceneDev *dev, ShadowHull *hull)
{
    if (!s || !dev || !hull) return MTR_ERR_INVALID;
    *dev = s->dev; *hull = s->hull;
    return MTR_OK;
}

} // extern "C"

// ---- MTR_MODE_WAVEFRONT: host loop over tiles and bounces ------------------------------------
// sizes of a tile's device buffers: what wf_alloc allocates and what wf_render's choice of the tile adds up.  Per slot 317 B
// (planes 120, live lists 8, their rays 64, material lists 20, zombie lists 8, shadow rays 32, occlusion flag 1, records 64;
// polarized 461 B: + 80 B of Mueller / Stokes planes, + 64 B of records), the rest per segment or per pixel
struct WfBytes {
    size_t planes, q_live, q_ray, q_mat, q_zombie, r_shadow, occ, counts, rec, rec_count;
    size_t total() const { return planes + q_live + q_ray + q_mat + q_zombie + r_shadow + occ + counts + rec + rec_count; }
};
static WfBytes wf_bytes(uint32_t n_slots, uint32_t P, uint32_t n_seg, uint32_t rec_cap, bool polar)
{
    WfBytes b;
    b.planes = wf_planes_bytes(n_slots) + (polar ? wf_polar_planes_bytes(n_slots) : 0);
    b.q_live = (size_t)2 * n_slots * 4;
    b.q_ray = (size_t)2 * n_slots * 32;                          // rays of the live lists, in list order
    b.q_mat = (size_t)kWfKeys * n_slots * 4;
    b.q_zombie = (size_t)2 * n_slots * 4;                        // paths that ended with an emitter-sampling term parked, per parity
    b.r_shadow = (size_t)n_slots * 32;
    b.occ = (size_t)n_slots + (size_t)n_seg * 16u + 16u;         // [n_seg][seg rounded up to 16] occlusion flags in shadow-list order
    b.counts = ((size_t)n_seg * (7 + kWfKeys) + 16) * 4;         // seg_live[2][n_seg], seg_mat[n_seg][5], seg_shadow[n_seg], live_total + seg_list_n[2] (16 words), seg_list[2][n_seg], seg_zombie[2][n_seg]
    b.rec = std::max<size_t>(16, (size_t)P * rec_cap * 16);
    b.rec_count = (size_t)P * 4;
    return b;
}
static int wf_alloc(mtr_scene *s, uint32_t n_slots, uint32_t P, uint32_t n_seg, uint32_t rec_cap, bool polar = false)
{
    mtr_ctx *c = s->ctx;
    WfWorkspace &w = s->wf;
    if (w.n_slots >= n_slots && w.P >= P && w.rec_cap == rec_cap && w.rows >= n_seg && w.planes && (w.polar || !polar)) return MTR_OK;
    w.release();
    const WfBytes b = wf_bytes(n_slots, P, n_seg, rec_cap, polar);
    HIP_TRY(c, hipMalloc(&w.planes, b.planes));
    HIP_TRY(c, hipMalloc(&w.q_live, b.q_live));
    HIP_TRY(c, hipMalloc(&w.q_ray, b.q_ray));
    HIP_TRY(c, hipMalloc(&w.q_mat, b.q_mat));
    HIP_TRY(c, hipMalloc(&w.q_zombie, b.q_zombie));
    HIP_TRY(c, hipMalloc(&w.r_shadow, b.r_shadow));
    HIP_TRY(c, hipMalloc(&w.occ, b.occ));
    HIP_TRY(c, hipMalloc(&w.counts, b.counts));
    HIP_TRY(c, hipMalloc(&w.rec, b.rec));
    HIP_TRY(c, hipMalloc(&w.rec_count, b.rec_count));
    if (!w.host_count) HIP_TRY(c, hipHostMalloc((void **)&w.host_count, 64));
    for (hipEvent_t &e : w.poll_ev) if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    w.n_slots = n_slots; w.P = P; w.rec_cap = rec_cap; w.rows = n_seg; w.bytes = b.total(); w.polar = polar;
    return MTR_OK;
}

// launches and (timed renders) kernel times of one render, as mtr_kernel_times reports them
struct RenderStats {
    uint32_t launches = 0, scatter_launches = 0, trace_kernel_launches = 0;
    float trace_ms = 0.0f, shade_ms = 0.0f, scatter_ms = 0.0f;          // k_wf_trace, k_wf_shade, the scatter-add
};
// the timing events of one class of launches: a pair per launch, destroyed with the holder whichever way the render returns
struct EventPairs {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    EventPairs() = default;
    EventPairs(const EventPairs &) = delete;           // (the holder owns its events)
    ~EventPairs() { for (auto &pr : ev) { if (pr.first) (void)hipEventDestroy(pr.first); if (pr.second) (void)hipEventDestroy(pr.second); } }
    hipError_t record_begin(hipStream_t stream)
    {
        ev.push_back({ nullptr, nullptr });
        hipError_t e = hipEventCreate(&ev.back().first);
        if (e == hipSuccess) e = hipEventCreate(&ev.back().second);
        return e == hipSuccess ? hipEventRecord(ev.back().first, stream) : e;
    }
    hipError_t record_end(hipStream_t stream) { return hipEventRecord(ev.back().second, stream); }
    hipError_t sum_ms(float *out) const         // (once the stream has drained)
    {
        *out = 0.0f;
        for (auto &pr : ev) {
            float ms = 0.0f;
            if (hipError_t e = hipEventElapsedTime(&ms, pr.first, pr.second)) return e;
            *out += ms;
        }
        return hipSuccess;
    }
};

static int wf_render(mtr_scene *s, const mtr_render_params *p, float *t4, float *s4, const RenderConst &rc, bool timed, bool may_block,
                     RenderStats *st)
{
    mtr_ctx *c = s->ctx;
    const Film &f = s->film;
    const bool polar = (p->flags & MTR_FLAG_POLARIZED) != 0u;
    WfConfig cfg{};
    if (!wf_plan(s->dev, cfg)) return fail(c, MTR_ERR_UNSUPPORTED, "wavefront: BVH too deep for the LDS stack");
    cfg.spheres = s->has_sphere;
    const uint32_t n_pixels = p->pixel_end - p->pixel_begin;
    const uint32_t spp_chunk = p->spp_end - p->spp_begin;
    // tile = P pixels x S samples (2^25 slots); segment = G whole pixels (about 4096 slots: with the persistent
    // k_wf_trace a segment is drained once per launch, so longer segments waste less — staircase 1024: 425 ms,
    // 2048: 390, 4096: 360, 8192: 397)
    // Tile: as many slots as half of the free device memory holds, at most 2^28 (85 GB of workspace at 317 B per slot: wf_bytes).  Every
    // bounce of every tile costs four launches with ~0.1 ms of fixed cost each, and with max_depth 65 most of them run nearly
    // empty: config 5 (2^29 slots) with tiles of 2^25 / 2^26 / 2^27 / 2^28 slots: 2.01 / 1.80 / 1.70 / 1.59 s per render
    // (config 2 in this organisation: 2^22 269 ms, 2^24 174 ms, 2^25 168 ms).
    // Segment: scenes walked in HBM 8192 slots (config 5: 2048 / 4096 / 8192 / 16384 slots: 338 / 288 / 275 / 273 ms at 256 spp
    // with the 8-wide tree); scenes staged in LDS the same since k_wf_shade's state diet (round 5; config 2 with 2048 / 4096 / 6144 /
    // 8192 / 12288 / 16384 slots: 97.8 / 81.9 / 79.4 / 77.1 - 79.7 / 77.5 / 80.8 ms, 108 triangles 131.9 / 117.2 / 113.9 / 116.1 / 114.7 /
    // 123.4 ms; rounds 2-4 had 4096: 141 against 169 ms with 8192 then).
    uint32_t kTileSlots = 1u << 28; uint32_t kSegSlots = 8192u;
    if (const char *e = mtr::knob("MTR_WF_SEG")) kSegSlots = (uint32_t)atoi(e);      // experiments
    if (kSegSlots > 32768u) kSegSlots = 32768u;          // a segment holds at most 2^16 slots (seg < kSegSlots + S): k_wf_trace packs (list position, slot) into one word
    const uint32_t S = spp_chunk < 4096u ? spp_chunk : 4096u;
    // (at most 1024 pixels per segment: k_wf_shade keeps 20 B of LDS per pixel of its segment — record-list tail, steady sums —
    // and a render of very few samples per pixel would otherwise ask for more LDS than a CU has: 8192 pixels = 164 KB)
    const uint32_t G = std::min<uint32_t>((kSegSlots + S - 1) / S, 1024u);
    // time-bin records: per-pixel lists sized for 4 contributions per path; the rest (and rows that do not
    // fit LDS) fall back to f32 atomics on the film
    const bool rows_fit = (size_t)f.bins * (polar ? 16u : 12u) <= 150u * 1024u;
    const uint32_t rec_cap = rows_fit ? S * (polar ? 8u : 4u) : 0u;        // (polarized: two records per contribution)
    {
        size_t free_b = 0, total_b = 0;
        auto tile_bytes = [&](uint32_t slots) { const uint32_t px = slots / S; return wf_bytes(slots, px, (px + G - 1) / G, rec_cap, polar).total(); };
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            // half of what is free now (the workspace this scene already holds counts as free), and never more than a third of
            // the device: the caller's allocator (films, all-gather buffers, a second scene) needs room the driver cannot see
            size_t budget = (free_b + s->wf.bytes) / 2;
            if (budget > total_b / 3) budget = total_b / 3;
            while (kTileSlots > (1u << 22) && tile_bytes(kTileSlots) > budget) kTileSlots >>= 1;
        } else kTileSlots = 1u << 25;
    }
    if (const char *e = mtr::knob("MTR_WF_TILE_LOG2")) kTileSlots = 1u << atoi(e);      // experiments
    uint32_t P = kTileSlots / S; if (P < G) P = G; if (P > n_pixels) P = n_pixels;
    const uint32_t n_slots_max = P * S;
    const uint32_t seg = G * S;
    const uint32_t n_seg_max = (P + G - 1) / G;      // (of the first attempt; wf_alloc below may settle for a smaller tile)
    int rc_ = wf_alloc(s, n_slots_max, P, n_seg_max, rec_cap, polar);
    // out of memory (someone else took it between hipMemGetInfo and here): halve the tile until the workspace fits
    while (rc_ == MTR_ERR_OOM && P > G && (size_t)P * S > (1u << 22)) {
        (void)hipGetLastError();                       // (the failed hipMalloc must not surface at the next launch check)
        P = std::max(G, ((P / 2 + G - 1) / G) * G);
        rc_ = wf_alloc(s, P * S, P, (P + G - 1) / G, rec_cap, polar);
    }
    if (rc_) return rc_;
    WfWorkspace &w = s->wf;

    WfArgs a{};
    a.sc = s->dev; a.cam = s->cam; a.film = f; a.rc = rc;
    a.planes = (float *)w.planes; a.q_live = (uint32_t *)w.q_live; a.q_ray = (float4 *)w.q_ray; a.q_mat = (uint32_t *)w.q_mat;
    a.r_shadow = (float4 *)w.r_shadow; a.occ = (uint8_t *)w.occ;
    // (The rays of a list are traced in list order.  Tracing them sorted by (cell of the origin, octant of the direction) — a counting
    // sort in k_wf_shade, round 6 — lost: config 5 at 256 spp k_wf_trace 108.2 -> 110.3 ms, render 155.6 -> 160.1 ms; config 2 in this
    // organisation 81.4 -> 88.9 ms.  That code was removed; it can be read in commit fd0fbb2.)
    a.q_zombie = (uint32_t *)w.q_zombie;
    a.rec = (uint4 *)w.rec; a.rec_count = (uint32_t *)w.rec_count; a.rec_cap = rec_cap;
    a.film_out = t4; a.steady_out = s4; a.counters = c->d_counters; a.log = s->log;
    a.G = G; a.seg = seg;
    a.nlos_on = s->nlos.on ? 1u : 0u;
    if (s->nlos.on) a.nlos = s->nlos.k;
    const int grid_full = c->n_cu * 8;
    // NLOS paths end by the integrator's own rules (filter depth, roulette): the host polls the live count like an unbounded render
    // (deep bounded renders poll too: with max_depth 65 no path of config 5 is alive after some 35 bounces, and every bounce of
    // every tile is four launches)
    // ... but only in calls that block anyway (counters / timings requested): a caller that keeps mtr_render asynchronous —
    // row bands overlapped with collectives — is not stalled inside it; its empty bounces cost 4 us per launch (live segment list)
    const bool unbounded = p->max_depth < 0 || s->nlos.on || (p->max_depth > 16 && may_block);
    // the reference loop always runs its first iteration (emission of the camera-ray hit), also at max_depth 0
    const uint32_t max_depth = p->max_depth < 0 ? 0xffffffffu : (p->max_depth == 0 ? 1u : (uint32_t)p->max_depth + (s->nlos.on ? 2u : 0u));
    EventPairs scatter_ev, trace_ev, shade_ev;
    // (timed renders only) events around every k_wf_trace launch — the dominant kernel of scenes in HBM is timed alone — around
    // the HBM-bound k_wf_shade (mtr_kernel_times.wf_shade_ms) and around the scatter-add
    auto launch_timed = [&](WfKernel which, int grid_, EventPairs &bucket) -> hipError_t {
        hipError_t e = timed ? bucket.record_begin(c->stream) : hipSuccess;
        if (e == hipSuccess) e = launch_wf(a, cfg, which, grid_, c->stream);
        if (e == hipSuccess && timed) e = bucket.record_end(c->stream);
        return e;
    };

    for (uint32_t s0 = 0; s0 < spp_chunk; s0 += S) {
        const uint32_t Scur = std::min(S, spp_chunk - s0);
        for (uint32_t pix = 0; pix < n_pixels; pix += P) {
            const uint32_t Pcur = std::min(P, n_pixels - pix);
            a.pix0 = p->pixel_begin + pix; a.P = Pcur; a.spp_begin = p->spp_begin + s0; a.S = Scur;
            a.n_slots = Pcur * Scur;
            a.film_zero = ((p->flags & MTR_FLAG_FILM_ZERO) && s0 == 0 && rec_cap > 0) ? 1u : 0u;
            a.seg = G * Scur;                                       // segments always cover whole pixels
            a.occ_stride = (a.seg + 15u) & ~15u;
            a.n_seg = (Pcur + G - 1) / G;
            a.seg_live = (uint32_t *)w.counts;
            a.seg_mat = (uint32_t *)w.counts + (size_t)2 * a.n_seg;
            a.seg_shadow = (uint32_t *)w.counts + (size_t)(2 + kWfKeys) * a.n_seg;
            uint32_t *live_total = (uint32_t *)w.counts + (size_t)(3 + kWfKeys) * a.n_seg;
            a.live_total = unbounded ? live_total : nullptr;
            a.seg_list_n = live_total + 4;
            a.seg_list = live_total + 16;
            a.seg_zombie = a.seg_list + (size_t)2 * a.n_seg;
            const int grid = (int)std::min<uint32_t>(a.n_seg, (uint32_t)grid_full);
            const int grid_gen = (int)std::min<uint32_t>((a.n_slots + kBlock - 1) / kBlock, (uint32_t)grid_full);
            HIP_TRY(c, hipMemsetAsync(w.rec_count, 0, (size_t)Pcur * 4, c->stream));
            a.parity = 0;
            a.ticket = c->d_ticket + 16; a.ticket_cur = 0u;                          // segment tickets (k_wf_trace / shadow_gen / shade)
            HIP_TRY(c, hipMemsetAsync(a.ticket, 0, 2 * sizeof(uint32_t), c->stream));
            HIP_TRY(c, launch_wf(a, cfg, WfKernel::Raygen, grid_gen, c->stream));    // (writes live list 0)
            HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)a.seg_list_n, (int)a.n_seg, 1, c->stream));     // bounce 0 walks every segment
            uint32_t depth = 0;
            // "Anyone left?" WITHOUT draining the stream (round 5).  Every 8 bounces the live count is copied to a pinned word and an
            // event is recorded behind the copy; the host then waits for the PREVIOUS poll's event — the count of 8 bounces ago —
            // while the chunk it has just enqueued keeps the GPU busy.  The loop therefore runs at most 8 bounces past the last
            // live path (launches over an empty segment list: 4 us each) and the stream never idles while the host decides; rounds
            // 1-4 synchronised the stream here, a bubble per chunk and a stall for a caller overlapping bands with collectives.
            uint32_t n_polls = 0;
            // (the count a poll reads is the one the PREVIOUS chunk of 8 bounces left: an unbounded render issues 8 - 16 bounce launches
            // over empty segment lists after its last path has died — about 4 us each; trace_launches and the kernel times of
            // mtr_kernel_times include that speculative tail)
            auto poll_live = [&](bool &done) -> int {
                const uint32_t cur = n_polls & 1u;
                HIP_TRY(c, hipMemcpyAsync(w.host_count + cur, live_total, 4, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipEventRecord(w.poll_ev[cur], c->stream));
                if (n_polls) {
                    HIP_TRY(c, hipEventSynchronize(w.poll_ev[cur ^ 1u]));
                    if (w.host_count[cur ^ 1u] == 0u) done = true;
                }
                ++n_polls;
                return MTR_OK;
            };
            while (depth < max_depth) {
                if (unbounded) HIP_TRY(c, hipMemsetAsync(live_total, 0, 4, c->stream));
                HIP_TRY(c, hipMemsetAsync(a.seg_list_n + (a.parity ^ 1u), 0, 4, c->stream));     // the list this bounce's survivors build
                if (a.nlos_on || polar) {       // NLOS tier / polarized transport: the whole loop iteration in one launch per bounce
                    if (polar) a.first_bounce = depth == 0u ? 1u : 0u;            // (bounce 0 builds its paths: polar_begin)
                    HIP_TRY(c, launch_wf(a, cfg, polar ? WfKernel::PolarBounce : WfKernel::NlosBounce, grid, c->stream)); a.ticket_cur ^= 1u;
                    st->launches += 1;
                    a.parity ^= 1u;
                    ++depth;
                    if (unbounded && (depth & 7u) == 0) { bool done = false; if (int r = poll_live(done)) return r; if (done) break; }
                    continue;
                }
                a.trace_any = 0u;
                a.first_bounce = depth == 0u ? 1u : 0u;
                HIP_TRY(c, launch_timed(WfKernel::Trace, grid, trace_ev)); a.ticket_cur ^= 1u;       // closest hit + material lists
                // shade: commits the emitter-sampling terms the previous bounce parked, runs the loop iteration once, writes the
                // shadow rays (scene in HBM) or traces them inline (scene in LDS), compacts the survivors
                HIP_TRY(c, launch_timed(WfKernel::Shade, grid, shade_ev)); a.ticket_cur ^= 1u;
                st->launches += 2;
                if (!cfg.scene_lds) {                                                // scene in HBM/L2: the shadow rays get their own persistent trace
                    a.trace_any = 1u;
                    HIP_TRY(c, launch_timed(WfKernel::Trace, grid, trace_ev)); a.ticket_cur ^= 1u;       // occlusion of this bounce's shadow rays: read by the NEXT shade
                    st->launches += 1;
                }
                a.parity ^= 1u;
                ++depth;
                if (unbounded && (depth & 7u) == 0) { bool done = false; if (int r = poll_live(done)) return r; if (done) break; }      // every 8 bounces: anyone left?
            }
            HIP_TRY(c, launch_timed(polar ? WfKernel::PolarScatter : WfKernel::Scatter, (int)std::min<uint32_t>(Pcur, (uint32_t)grid_full), scatter_ev));
            st->scatter_launches += 1;
        }
    }
    if (timed) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, scatter_ev.sum_ms(&st->scatter_ms));
        HIP_TRY(c, trace_ev.sum_ms(&st->trace_ms));
        HIP_TRY(c, shade_ev.sum_ms(&st->shade_ms));
    }
    st->trace_kernel_launches = (uint32_t)trace_ev.ev.size();
    return MTR_OK;
}

// fused_plan's verdict on a render: does a configuration fit, and does it keep the scene / the time-bin rows in LDS
struct FusedProbe { bool scene_lds, hist_lds; };
static FusedProbe fused_probe(mtr_scene *s, const mtr_render_params *p, uint32_t n_pixels, uint32_t spp_chunk)
{
    FusedArgs probe{}; FusedConfig pc{};
    probe.sc = s->dev; probe.cam = s->cam; probe.film = s->film; probe.rc = make_render_const(*p, s->film, s->dev.n_ems); probe.nlos_on = s->nlos.on ? 1u : 0u;
    const bool fits = fused_plan(s->dev, s->film, n_pixels, spp_chunk, usable_cus(s->ctx, p), probe, pc);
    return { fits && pc.scene_lds, fits && pc.hist_lds };
}
// MTR_MODE_AUTO -> the organisation that runs: the fused kernel when the whole scene can be staged in LDS (measured 143 vs
// 168 ms on config 2), the wavefront pipeline otherwise (BVH in HBM/L2: 21 vs 66 ms on an 81k-triangle scene)
static int resolve_mode(mtr_scene *s, const mtr_render_params *p, uint32_t n_pixels, uint32_t spp_chunk, uint32_t *mode_io,
                        uint32_t *developed_ok = nullptr)
{
    mtr_ctx *c = s->ctx;
    const Film &f = s->film;
    uint32_t mode = *mode_io;
    if (p->flags & MTR_FLAG_POLARIZED) {  // polarized transport: the wavefront organisation alone (k_wf_polar_bounce)
        if (s->nlos.on) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: polarized transport is not available for the NLOS tier");
        if (f.n_freq) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: polarized transport is not available with a phasor_hdr_film");
        if (!s->polar_ok)
            return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: polarized transport supports diffuse, conductor, roughconductor and dielectric BSDFs without textures, and area emitters");
        if (mode == MTR_MODE_FUSED)
            return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: polarized transport (MTR_FLAG_POLARIZED) runs in the wavefront mode only");
        if (p->flags & MTR_FLAG_DETERMINISTIC)   // the Stokes rows, the steady image and overflow cells are f32 atomics
            return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: polarized transport (MTR_FLAG_POLARIZED) has no deterministic rows (MTR_FLAG_DETERMINISTIC)");
        *mode_io = MTR_MODE_WAVEFRONT;
        if (developed_ok) *developed_ok = 0u;
        return MTR_OK;
    }
    // a phasor film has one (Re, Im) row per pixel: no [laser_x][laser_y] rows for the illuminated points of an Exhaustive capture
    if (s->nlos.on && f.n_freq && s->nlos.k.capture_type == MTR_CAPTURE_EXHAUSTIVE)
        return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: an Exhaustive capture (MTR_CAPTURE_EXHAUSTIVE) is not available with a phasor_hdr_film");
    if (s->nlos.on && f.n_freq && mode != MTR_MODE_WAVEFRONT) {
        // NLOS tier with a phasor film.  The fused kernel (k_fused<NLOS, PHASOR>) needs plain shading and (Re, Im) rows that fit LDS beside
        // the scene — it has LDS rows or none: fused_plan — and pays 2F LDS float atomics per contribution, where the wavefront
        // organisation appends one 16-byte record and k_wf_phasor_scatter folds the records per frequency in registers.  Config 4's share
        // with the film swapped (confocal 256 x 256, 512 spp, flat-shaded 'Z', tools/nlos_phasor_bench.py), fused / wavefront: F = 16
        // 7.00 / 7.38 ms, F = 27 8.91 / 7.65, F = 43 11.9 / 8.2, F = 412 91.3 / 16.0 (run-to-run spread 0.1 - 0.3 ms): AUTO takes the
        // tier's default, the fused kernel, up to 16 frequencies and the wavefront organisation beyond
        constexpr uint32_t kNlosPhasorFusedMaxF = 16u;
        const bool fused_ok = !s->dev.has_rough && fused_probe(s, p, n_pixels, spp_chunk).hist_lds;
        if (mode == MTR_MODE_FUSED && !fused_ok)
            return fail(c, MTR_ERR_UNSUPPORTED, s->dev.has_rough
                ? "mtr_render: rough BSDFs / smooth-shaded triangles with a phasor film or deterministic rows need the wavefront mode"
                : "mtr_render: the (Re, Im) rows of this phasor_hdr_film do not fit LDS: the NLOS tier renders it in the wavefront mode");
        if (mode == MTR_MODE_AUTO) mode = (fused_ok && f.n_freq <= kNlosPhasorFusedMaxF) ? MTR_MODE_FUSED : MTR_MODE_WAVEFRONT;
    }
    if (s->nlos.on && mode == MTR_MODE_AUTO)                             // (wavefront = the second organisation: on request, and for
        mode = (s->dev.has_rough && (p->flags & MTR_FLAG_DETERMINISTIC)) ? MTR_MODE_WAVEFRONT : MTR_MODE_FUSED;      // deterministic rows with the extended shading)
    if (f.n_freq) {                      // phasor film: (opl, value) records -> wavefront pipeline by default; LDS (Re, Im) rows in the fused kernel on request
        if (mode == MTR_MODE_AUTO) mode = MTR_MODE_WAVEFRONT;
    }
    if (s->dev.has_rough) {              // GGX lobes / smooth normals / bitmaps: f32 rows only (fused), or the wavefront pipeline
        const bool fused_ok = !f.n_freq && !(p->flags & MTR_FLAG_DETERMINISTIC);
        if (mode == MTR_MODE_FUSED && !fused_ok)
            return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: rough BSDFs / smooth-shaded triangles with a phasor film or deterministic rows need the wavefront mode");
        if (mode == MTR_MODE_AUTO && !fused_ok) mode = MTR_MODE_WAVEFRONT;
    }
    // (planned once, and only where the answer depends on it)
    const bool want_rows = developed_ok && !f.n_freq && (mode == MTR_MODE_AUTO || mode == MTR_MODE_FUSED);
    const FusedProbe probe = (mode == MTR_MODE_AUTO || want_rows) ? fused_probe(s, p, n_pixels, spp_chunk) : FusedProbe{ false, false };
    if (mode == MTR_MODE_AUTO) {
        const bool fits = probe.scene_lds;
        // ... and only a SHALLOW tree (a room of rectangles and a few objects: root + object nodes).  k_fused walks in lock-step — every
        // traversal costs its wave the longest walk of 64 lanes — which a deeper tree punishes at once: the Cornell box with its boxes
        // tessellated 2 x 2 per face (108 triangles, 3 levels) renders in 204 ms fused against 125 ms in the wavefront organisation,
        // whose trace kernel refills finished lanes (36 triangles, 2 levels: 58.7 against 97.5 ms; profiles/r05_size_sweep.txt)
        const bool shallow = s->dev.wide_levels <= 2u;
        mode = (fits && shallow) ? MTR_MODE_FUSED : MTR_MODE_WAVEFRONT;
    }
    *mode_io = mode;
    // MTR_FLAG_DEVELOPED_ROWS: the fused kernel's row flush, rows in LDS, time bins (not a phasor film)
    if (developed_ok) *developed_ok = (mode == MTR_MODE_FUSED && want_rows && probe.hist_lds) ? 1u : 0u;
    return MTR_OK;
}

// MTR_MODE_SAMPLES (mtr_samples.hip): what it refuses — before any launch, both tensors untouched — and its plan
static int samples_check(mtr_scene *s, const mtr_render_params *p, uint32_t n_pixels, uint32_t spp_chunk, SamplesPlan *pl)
{
    mtr_ctx *c = s->ctx;
    const Film &f = s->film;
    const char *why = nullptr;
    if (s->nlos.on) why = "the NLOS tier";
    else if (f.n_freq) why = "a phasor_hdr_film";
    else if (f.lasers > 1u) why = "an exhaustive_scan film";
    else if (p->flags & MTR_FLAG_POLARIZED) why = "polarized transport (MTR_FLAG_POLARIZED)";
    else if (p->flags & MTR_FLAG_DETERMINISTIC) why = "deterministic rows (MTR_FLAG_DETERMINISTIC)";
    else if (p->flags & MTR_FLAG_DEVELOPED_ROWS) why = "MTR_FLAG_DEVELOPED_ROWS";
    else if (p->n_bands) why = "band completion words";
    if (why) return fail(c, MTR_ERR_UNSUPPORTED, std::string("mtr_render: MTR_MODE_SAMPLES renders transient_path into a plain transient_hdr_film with f32 rows: not ") + why);
    SamplesPlan local;
    if (n_pixels && spp_chunk && !samples_plan(s->dev, f, n_pixels, spp_chunk, usable_cus(c, p), pl ? *pl : local))
        return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: MTR_MODE_SAMPLES: the time-bin row, the traversal stack and the scene exceed the 160 KiB of LDS");
    return MTR_OK;
}

// the ranges of mtr_render_params that every render entry point checks; `who` prefixes the message, `advice` ends the lane-count one
static int check_render_ranges(mtr_ctx *c, const Film &f, const mtr_render_params *p, const char *who, const char *advice)
{
    const std::string pre = std::string(who) + ": ";
    const uint64_t npix_crop = (uint64_t)f.crop_w * f.crop_h;
    if (p->spp_total == 0 || p->spp_begin > p->spp_end || p->spp_end > p->spp_total)
        return fail(c, MTR_ERR_INVALID, pre + "bad sample range");
    if (p->pixel_begin > p->pixel_end || p->pixel_end > npix_crop)
        return fail(c, MTR_ERR_INVALID, pre + "bad pixel range");
    if (npix_crop * p->spp_total > (1ull << 32))
        return fail(c, MTR_ERR_UNSUPPORTED, pre + "W*H*spp exceeds 2^32 lanes (common.py:51); " + advice);
    if (p->max_depth < -1 || p->rr_depth <= 0) return fail(c, MTR_ERR_INVALID, pre + "bad max_depth / rr_depth");
    return MTR_OK;
}
static int counters_to_abi(mtr_ctx *c, mtr_counters *out)
{
    DevCounters h;
    HIP_TRY(c, hipMemcpy(&h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->paths = h.paths; out->rays_closest = h.rays_closest; out->rays_shadow = h.rays_shadow;
    out->splats_issued = h.splats_issued; out->bounces = h.bounces; out->splats_overflow = h.splats_overflow;
    out->reserved[0] = h.r0; out->reserved[1] = h.r1;
    return MTR_OK;
}
// a context-owned device buffer of at least `need` bytes (a launch in flight may read the old one: the stream drains first)
static int grow_device_buffer(mtr_ctx *c, void **ptr, size_t *cap, size_t need)
{
    if (*cap >= need) return MTR_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr; *cap = 0;
    HIP_TRY(c, hipMalloc(ptr, need));
    *cap = need;
    return MTR_OK;
}

extern "C" {

int mtr_film_clear(mtr_ctx *c, const mtr_film_desc *f, float *t4, float *s4)
{
    if (!c || !f) return fail(c, MTR_ERR_INVALID, "mtr_film_clear: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    size_t npix = (size_t)f->width * f->height;
    const Film fm = film_from_desc(*f);
    const size_t per_pixel = fm.n_freq ? (size_t)2 * fm.n_freq + 1 : (size_t)fm.bins * 4;   // (2F+1) | [lasers][T][4]
    if (t4) HIP_TRY(c, hipMemsetAsync(t4, 0, npix * per_pixel * sizeof(float), c->stream));
    if (s4) HIP_TRY(c, hipMemsetAsync(s4, 0, npix * 4 * sizeof(float), c->stream));
    return MTR_OK;
}

int mtr_render(mtr_scene *s, const mtr_render_params *p, float *t4, float *s4,
               mtr_counters *counters_out, mtr_kernel_times *times_out)
{
    if (!s || !p || !t4 || !s4) return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_render: NULL argument");
    mtr_ctx *c = s->ctx;
    const Film &f = s->film;
    if (int r = check_render_ranges(c, f, p, "mtr_render", "shard the render")) return r;
    if (p->mode > MTR_MODE_SAMPLES) return fail(c, MTR_ERR_INVALID, "mtr_render: unknown mode");
    SamplesPlan spl{};
    if (p->mode == MTR_MODE_SAMPLES)
        if (int r = samples_check(s, p, p->pixel_end - p->pixel_begin, p->spp_end - p->spp_begin, &spl)) return r;
    HIP_TRY(c, hipSetDevice(c->device));

    FusedArgs a{};
    a.sc = s->dev; a.cam = s->cam; a.film = f;
    a.rc = make_render_const(*p, f, s->dev.n_ems);
    a.pixel_begin = p->pixel_begin; a.pixel_end = p->pixel_end;
    a.spp_begin = p->spp_begin; a.spp_chunk = p->spp_end - p->spp_begin;
    a.film_out = t4; a.steady_out = s4;
    a.counters = c->d_counters;
    a.log = s->log;
    {   // SHADOW HULL MARGIN (bits 16..31 of the flags): v + 1 times the derived guard distances, MTR_SHADOW_HULL_OFF: no block
        const uint32_t v = p->flags >> MTR_SHADOW_HULL_SHIFT;
        a.hull = shadow_hull_with_margin(s->hull, v == MTR_SHADOW_HULL_OFF ? 0.0f : (float)(v + 1u));
    }
    a.nlos_on = s->nlos.on ? 1u : 0u;
    if (s->nlos.on) {
        a.nlos = s->nlos.k;
        if (s->nlos.k.film_w != f.width || s->nlos.k.film_h != f.height)
            return fail(c, MTR_ERR_INVALID, "mtr_render: film size changed after mtr_scene_set_nlos; call it again");
    }

    const uint32_t n_pixels = p->pixel_end - p->pixel_begin;
    const bool want_stats = counters_out || times_out;
    if (!(p->flags & MTR_FLAG_KEEP_COUNTERS)) HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, sizeof(DevCounters), c->stream));
    if (s->log.count) HIP_TRY(c, hipMemsetAsync(s->log.count, 0, sizeof(unsigned long long), c->stream));
    if (times_out) HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    RenderStats st;
    if (n_pixels && a.spp_chunk && p->mode == MTR_MODE_SAMPLES) {
        // the slabs' rows: context-owned, like the partition workspace of mtr_splat_add (kept up to 256 MiB between calls)
        constexpr size_t kSamplesRetain = (size_t)256 << 20;
        if (int r = grow_device_buffer(c, &c->d_samples, &c->samples_cap, spl.partial_bytes)) return r;
        SamplesArgs sa{};
        sa.sc = s->dev; sa.cam = s->cam; sa.film = f; sa.rc = a.rc;
        sa.pixel_begin = p->pixel_begin; sa.n_pixels = n_pixels; sa.spp_begin = p->spp_begin; sa.spp_chunk = a.spp_chunk;
        sa.film_zero = (p->flags & MTR_FLAG_FILM_ZERO) ? 1u : 0u;
        sa.partial = (float *)c->d_samples; sa.film_out = t4; sa.steady_out = s4; sa.counters = c->d_counters;
        HIP_TRY(c, launch_samples(sa, spl, c->stream));
        st.launches = 2;
        if (c->samples_cap > kSamplesRetain) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_samples);
            c->d_samples = nullptr; c->samples_cap = 0;
        }
    } else if (n_pixels && a.spp_chunk) {
        uint32_t mode = p->mode, dev_ok = 0u;
        if (int r = resolve_mode(s, p, n_pixels, a.spp_chunk, &mode, &dev_ok)) return r;
        if ((p->flags & MTR_FLAG_DEVELOPED_ROWS) && !dev_ok)
            return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: MTR_FLAG_DEVELOPED_ROWS needs the fused organisation with time-bin rows in LDS (see mtr_render_plan)");
        if (p->n_bands && (mode == MTR_MODE_WAVEFRONT || !p->band_done || p->n_bands > n_pixels))
            return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: band completion words need the fused organisation, a band_done array and at most one band per pixel");
        if (mode == MTR_MODE_WAVEFRONT) {
            if (int r = wf_render(s, p, t4, s4, a.rc, times_out != nullptr, want_stats, &st)) return r;
        } else {
            FusedConfig cfg{};
            if (!fused_plan(s->dev, f, n_pixels, a.spp_chunk, usable_cus(c, p), a, cfg))
                return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render: no kernel configuration fits (BVH depth / LDS)");
            const uint32_t launch_slot = c->fused_launches++ & 15u;
            a.ticket = c->d_ticket + launch_slot;
            // START BLOCKS: the launch's path-start table, one per ticket counter for the same reason (fused_start_table_bytes: 0 for
            // every kernel but the lean flat-walk ones; config 2's grid: 12 MiB per table)
            static_assert(kStartSlots == 16u, "one path-start table per ticket counter of the rotation");
            if (const size_t tab_bytes = fused_start_table_bytes(a, cfg)) {
                // The slot stride follows from the ALLOCATION (start_slot_stride), not from this launch's grid: launches of different
                // grids in flight on two streams keep disjoint tables.  A larger table re-allocates: grow_device_buffer drains this
                // context's stream and hipFree waits for the device's other work before the old tables go.
                if (start_slot_stride(c->start_cap) < tab_bytes)
                    if (int r = grow_device_buffer(c, &c->d_start, &c->start_cap, start_alloc_bytes(tab_bytes))) return r;
                a.start_tab = (unsigned char *)c->d_start + start_slot_off(start_slot_stride(c->start_cap), launch_slot);
            }
            a.n_bands = 0u;
            if (p->n_bands) {
                // (one banded launch in flight per context: the counts are the context's; callers that overlap launches on two
                // streams — the per-band pipeline — do not use band words)
                if (int r = grow_device_buffer(c, (void **)&c->d_band_count, &c->band_cap, (size_t)p->n_bands * sizeof(uint32_t))) return r;
                HIP_TRY(c, hipMemsetAsync(c->d_band_count, 0, (size_t)p->n_bands * sizeof(uint32_t), c->stream));
                a.n_bands = p->n_bands; a.band_px = n_pixels / p->n_bands; a.band_epoch = p->band_epoch;      // (>= 1: n_bands <= n_pixels, checked above; the last band takes the remainder)
                a.band_count = c->d_band_count; a.band_done = (uint32_t *)(uintptr_t)p->band_done;
            }
            HIP_TRY(c, launch_fused(a, cfg, c->stream));
            st.launches = 1;
        }
    }
    if (times_out) HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if (want_stats) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (counters_out) if (int r = counters_to_abi(c, counters_out)) return r;
        if (times_out) {
            memset(times_out, 0, sizeof *times_out);
            float ms = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
            times_out->total_ms = ms; times_out->trace_ms = ms - st.scatter_ms; times_out->scatter_ms = st.scatter_ms;
            times_out->trace_launches = st.launches; times_out->scatter_launches = st.scatter_launches;
            times_out->wf_trace_ms = st.trace_ms; times_out->wf_trace_kernel_launches = st.trace_kernel_launches; times_out->wf_shade_ms = st.shade_ms;
        }
    }
    return MTR_OK;
}

int mtr_render_plan(mtr_scene *s, const mtr_render_params *p, uint32_t *mode_out, uint32_t *developed_rows_ok)
{
    if (!s || !p || !mode_out) return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_render_plan: NULL argument");
    if (p->mode > MTR_MODE_SAMPLES) return fail(s->ctx, MTR_ERR_INVALID, "mtr_render_plan: unknown mode");
    if (p->pixel_begin > p->pixel_end || p->spp_begin > p->spp_end) return fail(s->ctx, MTR_ERR_INVALID, "mtr_render_plan: bad range");
    if (p->mode == MTR_MODE_SAMPLES) {           // on request only: MTR_MODE_AUTO never resolves to it
        if (int r = samples_check(s, p, p->pixel_end - p->pixel_begin, p->spp_end - p->spp_begin, nullptr)) return r;
        *mode_out = MTR_MODE_SAMPLES;
        if (developed_rows_ok) *developed_rows_ok = 0u;
        return MTR_OK;
    }
    uint32_t mode = p->mode;
    if (int r = resolve_mode(s, p, p->pixel_end - p->pixel_begin, p->spp_end - p->spp_begin, &mode, developed_rows_ok)) return r;
    *mode_out = mode;
    return MTR_OK;
}

// ---- what the derivative entry points (render_grad, render_fwd) share -------------------------
// the tint slot table of the scene's materials (tint_slot_table, mtr_scene_host.h: 2 n_mats + 2 entries) and the number of slots
static int scene_tint_slots(mtr_scene *s, std::vector<int32_t> &slots, uint32_t *n_tints)
{
    mtr_ctx *c = s->ctx;
    const uint32_t n_m = s->dev.n_mats;
    std::vector<mtr_material> mats(n_m);
    slots.assign(2u * (size_t)n_m + 2u, -1);
    if (n_m) HIP_TRY(c, hipMemcpy(mats.data(), s->dev.mats, n_m * sizeof(mtr_material), hipMemcpyDeviceToHost));
    *n_tints = tint_slot_table(mats.data(), n_m, slots.data());
    return MTR_OK;
}

// the first n_e emitters of the scene with unit radiance — what a derivative kernel traces: a contribution without its radiance
// factor — and the true radiances beside them: rad holds 3 n_rad + 3 words (n_rad >= n_e; the NLOS tier's one "emitter" is the
// laser, which the caller fills in), the first 3 n_e of them set here
static int unit_emitters(mtr_scene *s, uint32_t n_e, uint32_t n_rad, std::vector<Emitter> &ems, std::vector<float> &rad)
{
    mtr_ctx *c = s->ctx;
    ems.resize(n_e);
    rad.assign(3u * (size_t)n_rad + 3u, 0.0f);
    if (n_e) HIP_TRY(c, hipMemcpy(ems.data(), s->dev.ems, n_e * sizeof(Emitter), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ems.size(); ++i)
        for (int k = 0; k < 3; ++k) { rad[3u * i + k] = ems[i].radiance[k]; ems[i].radiance[k] = 1.0f; }
    return MTR_OK;
}

// One device allocation handed out in 256-byte-aligned pieces: alloc() takes the sizes of the pieces, take() hands them out in
// that order (NULL for a piece past what alloc() was told: a caller's launch then fails on its own checks instead of writing
// outside the block).  release() waits for the context's stream, frees the block and returns what the wait said; the destructor
// does the same for a caller that returns early.
struct Workspace {
    mtr_ctx *c;
    unsigned char *base = nullptr;
    size_t used = 0, cap = 0;
    explicit Workspace(mtr_ctx *ctx) : c(ctx) {}
    Workspace(const Workspace &) = delete;
    Workspace &operator=(const Workspace &) = delete;
    static size_t piece(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }
    hipError_t alloc(std::initializer_list<size_t> pieces)
    {
        for (size_t b : pieces) cap += piece(b);
        return hipMalloc((void **)&base, cap);
    }
    void *take(size_t bytes)
    {
        assert(used + piece(bytes) <= cap && "Workspace::take beyond what alloc() was told");
        if (used + piece(bytes) > cap) return nullptr;
        void *p = base + used; used += piece(bytes); return p;
    }
    hipError_t release()
    {
        if (!base) return hipSuccess;
        const hipError_t e_sync = hipStreamSynchronize(c->stream);
        (void)hipFree(base);
        base = nullptr;
        return e_sync;
    }
    ~Workspace() { (void)release(); }
};

// mtr_render_grad (grad_texels == nullptr), mtr_render_grad_tex and mtr_render_grad_tint (grad_tints != nullptr)
static int render_grad(mtr_scene *s, const mtr_render_params *p, const float *g_s, const float *g_t,
                       float *grad_materials, float *grad_emitters, float *grad_texels, float *grad_tints = nullptr)
{
    if (!s || !p || !g_s || !g_t || !grad_materials || ((s->dev.n_ems || s->nlos.on) && !grad_emitters))
        return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_render_grad: NULL argument");
    mtr_ctx *c = s->ctx;
    const Film &f = s->film;
    if (int r = check_render_ranges(c, f, p, "mtr_render_grad", "render in passes")) return r;
    if (f.n_freq || f.lasers > 1u || (p->flags & MTR_FLAG_POLARIZED))
        return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render_grad: a plain transient_hdr_film (RGB) only: "
                                            "no phasor film, exhaustive_scan or polarized transport");
    const bool nlos = s->nlos.on;
    if (nlos) {
        if (s->nlos.k.capture_type == MTR_CAPTURE_EXHAUSTIVE)
            return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render_grad: the NLOS tier with a Single or Confocal capture only (no Exhaustive capture)");
        if (grad_tints) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render_grad_tint: tint gradients are for transient_path only (not the NLOS tier)");
        if (s->nlos.k.film_w != f.width || s->nlos.k.film_h != f.height)
            return fail(c, MTR_ERR_INVALID, "mtr_render_grad: film size changed after mtr_scene_set_nlos; call it again");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // (the NLOS tier: the laser is the one "emitter" of the gradient; the scene's emitter table is empty)
    const uint32_t n_m = s->dev.n_mats, n_e = nlos ? 1u : s->dev.n_ems, slab_n = 3u * (n_m + n_e);
    const uint32_t n_pixels = p->pixel_end - p->pixel_begin, chunk = p->spp_end - p->spp_begin;
    const uint64_t n_lanes = (uint64_t)n_pixels * chunk;
    size_t lds = 0; bool scene_lds = false;
    const uint32_t n_tx = s->n_texels;
    // tint slots (mtr_render_grad_tint): from the material table; the tint kernel carries no texel code, so texel gradients asked
    // for beside tints come from a launch of their own first (its materials' and emitters' words are stored again below)
    std::vector<int32_t> slots;
    uint32_t n_tints = 0u;
    if (grad_tints) {
        if (int r = scene_tint_slots(s, slots, &n_tints)) return r;
        if (n_tints == 0u) grad_tints = nullptr;
    }
    if (grad_tints && grad_texels) {
        if (int r = render_grad(s, p, g_s, g_t, grad_materials, grad_emitters, grad_texels)) return r;
        grad_texels = nullptr;
    }
    const uint32_t tier = grad_texels ? grad_tex_tier(s->dev, n_tx, nlos) : MTR_GRAD_TEX_NONE;
    const uint32_t slab_tx = grad_tints ? n_tints : (tier == MTR_GRAD_TEX_SLAB ? n_tx : 0u);     // slab entries behind the emitters'
    const uint32_t grid = n_lanes ? grad_grid(s->dev, n_lanes, c->n_cu, &lds, &scene_lds, slab_tx, nlos) : 0u;
    if (n_lanes && grid == 0u)
        return fail(c, MTR_ERR_UNSUPPORTED, nlos ? "mtr_render_grad: the NLOS tier needs a scene whose tables, gradient slab and traversal stack fit LDS"
                                                 : "mtr_render_grad: the gradient slab and traversal stack exceed LDS");
    if (grid == 0u) {
        if (grad_tints) HIP_TRY(c, hipMemsetAsync(grad_tints, 0, (size_t)n_tints * 3u * sizeof(float), c->stream));
        HIP_TRY(c, hipMemsetAsync(grad_materials, 0, (size_t)n_m * 3u * sizeof(float), c->stream));
        if (n_e) HIP_TRY(c, hipMemsetAsync(grad_emitters, 0, (size_t)n_e * 3u * sizeof(float), c->stream));
        if (tier != MTR_GRAD_TEX_NONE) HIP_TRY(c, hipMemsetAsync(grad_texels, 0, (size_t)n_tx * 3u * sizeof(float), c->stream));
        return MTR_OK;
    }
    // the traced emitter table carries unit radiance (a contribution without its radiance factor); the true radiance goes alongside
    // (the NLOS tier: the walk runs with unit irradiance, and the laser's true irradiance is the one entry of `rad`)
    std::vector<Emitter> ems;
    std::vector<float> rad;
    if (int r = unit_emitters(s, nlos ? 0u : n_e, n_e, ems, rad)) return r;
    NlosConst nlos_unit{};
    if (nlos) {
        nlos_unit = s->nlos.k;
        rad[0] = nlos_unit.l_irr.x; rad[1] = nlos_unit.l_irr.y; rad[2] = nlos_unit.l_irr.z;
        nlos_unit.l_irr = mk(1, 1, 1);
    }
    const size_t ems_b = ems.size() * sizeof(Emitter), rad_b = rad.size() * sizeof(float);
    const size_t partial_b = (size_t)grid * (slab_n + 3u * slab_tx) * sizeof(double);
    const size_t acc_b = tier == MTR_GRAD_TEX_GLOBAL ? (size_t)n_tx * 3u * sizeof(double) : 0u;      // the global tier's f64 sums
    const size_t slots_b = grad_tints ? slots.size() * sizeof(int32_t) : 0u;                         // the tint slot table
    Workspace ws(c);
    HIP_TRY(c, ws.alloc({ ems_b, rad_b, partial_b, acc_b, slots_b }));
    Emitter *d_ems = (Emitter *)ws.take(ems_b);
    float *d_rad = (float *)ws.take(rad_b);
    double *d_partial = (double *)ws.take(partial_b);
    double *d_acc = acc_b ? (double *)ws.take(acc_b) : nullptr;
    int32_t *d_slots = slots_b ? (int32_t *)ws.take(slots_b) : nullptr;
    hipError_t e = hipSuccess;
    if (d_acc) e = hipMemsetAsync(d_acc, 0, acc_b, c->stream);
    if (d_slots && e == hipSuccess) e = hipMemcpy(d_slots, slots.data(), slots_b, hipMemcpyHostToDevice);
    if (!ems.empty() && e == hipSuccess) e = hipMemcpy(d_ems, ems.data(), ems_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rad, rad.data(), rad_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const RenderConst rc = make_render_const(*p, f, s->dev.n_ems);
        GradConst gc;
        gc.g_s = g_s; gc.g_t = g_t; gc.em_radiance = d_rad;
        gc.steady_scale = rc.sample_scale; gc.transient_scale = rc.sample_scale;
        if (grad_tints)
            e = launch_grad_tint(s->dev, d_ems, s->cam, f, rc, gc, p->pixel_begin, n_pixels, p->spp_begin, chunk, d_partial, grid, lds,
                                 scene_lds, grad_materials, grad_emitters, n_tints, d_slots, grad_tints, c->stream);
        else
            e = launch_grad(s->dev, d_ems, s->cam, f, rc, gc, p->pixel_begin, n_pixels, p->spp_begin, chunk, d_partial, grid, lds,
                            scene_lds, grad_materials, grad_emitters, c->stream, tier, n_tx, d_acc, grad_texels, nlos ? &nlos_unit : nullptr);
    }
    const hipError_t e_sync = ws.release();
    HIP_TRY(c, e);
    HIP_TRY(c, e_sync);
    return MTR_OK;
}

int mtr_render_grad(mtr_scene *s, const mtr_render_params *p, const float *g_s, const float *g_t,
                    float *grad_materials, float *grad_emitters)
{
    return render_grad(s, p, g_s, g_t, grad_materials, grad_emitters, nullptr);
}

int mtr_render_grad_tex(mtr_scene *s, const mtr_render_params *p, const float *g_s, const float *g_t,
                        float *grad_materials, float *grad_emitters, float *grad_texels)
{
    return render_grad(s, p, g_s, g_t, grad_materials, grad_emitters, grad_texels);
}

int mtr_render_grad_tint(mtr_scene *s, const mtr_render_params *p, const float *g_s, const float *g_t,
                         float *grad_materials, float *grad_emitters, float *grad_texels, float *grad_tints)
{
    return render_grad(s, p, g_s, g_t, grad_materials, grad_emitters, grad_texels, grad_tints);
}

// mtr_render_fwd (ABI 18): the refusals, shared with mtr_render_fwd_tier
static int check_render_fwd(mtr_scene *s, const mtr_render_params *p)
{
    mtr_ctx *c = s->ctx;
    const Film &f = s->film;
    if (int r = check_render_ranges(c, f, p, "mtr_render_fwd", "a forward-mode render runs in one pass")) return r;
    if (f.n_freq || f.lasers > 1u || (p->flags & MTR_FLAG_POLARIZED))
        return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render_fwd: a plain transient_hdr_film (RGB) only: "
                                            "no phasor film, exhaustive_scan or polarized transport");
    if (s->nlos.on) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render_fwd: transient_path only (not the NLOS tier)");
    if (p->spp_begin != 0u || p->spp_end != p->spp_total || (p->spp_scale != 0u && p->spp_scale != p->spp_total))
        return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render_fwd: every sample of a pixel in one call (no sample sub-range, no pass of a split "
                                            "render): a pixel's developed row is stored once");
    return MTR_OK;
}

int mtr_render_fwd_tier(const mtr_scene *s, const mtr_render_params *p, uint32_t *tier)
{
    if (!s || !p || !tier) return MTR_ERR_INVALID;
    if (int r = check_render_fwd(const_cast<mtr_scene *>(s), p)) return r;
    *tier = fwd_tier(s->dev, s->film);
    return MTR_OK;
}

// mtr_render_fwd (tan_tints == nullptr) and mtr_render_fwd_tint
static int render_fwd(mtr_scene *s, const mtr_render_params *p, const float *tan_materials, const float *tan_emitters,
                      const float *tan_texels, const float *tan_tints, float *steady_hw3, float *transient_hwt3)
{
    if (!s || !p || !tan_materials || (s->dev.n_ems && !tan_emitters) || !steady_hw3 || !transient_hwt3)
        return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_render_fwd: NULL argument");
    mtr_ctx *c = s->ctx;
    const Film &f = s->film;
    if (int r = check_render_fwd(s, p)) return r;
    const uint32_t n_pixels = p->pixel_end - p->pixel_begin;
    if (n_pixels == 0u) return MTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<int32_t> slots;
    if (tan_tints) {
        uint32_t n_tints = 0u;
        if (int r = scene_tint_slots(s, slots, &n_tints)) return r;
        if (n_tints == 0u) tan_tints = nullptr;
    }
    FwdPlan pl{};
    if (!fwd_plan(s->dev, f, n_pixels, p->spp_total, c->n_cu, pl))
        return fail(c, MTR_ERR_UNSUPPORTED, "mtr_render_fwd: the traversal stack and the staged scene exceed LDS");
    // the traced emitter table carries unit radiance; the true radiance goes alongside (as mtr_render_grad)
    const uint32_t n_e = s->dev.n_ems;
    std::vector<Emitter> ems;
    std::vector<float> rad;
    if (int r = unit_emitters(s, n_e, n_e, ems, rad)) return r;
    const size_t ems_b = ems.size() * sizeof(Emitter), rad_b = rad.size() * sizeof(float);
    const size_t slots_b = tan_tints ? slots.size() * sizeof(int32_t) : 0u;
    Workspace ws(c);
    HIP_TRY(c, ws.alloc({ ems_b, rad_b, slots_b }));
    Emitter *d_ems = (Emitter *)ws.take(ems_b);
    float *d_rad = (float *)ws.take(rad_b);
    int32_t *d_slots = (int32_t *)ws.take(slots_b);
    hipError_t e = hipSuccess;
    if (tan_tints) e = hipMemcpy(d_slots, slots.data(), slots_b, hipMemcpyHostToDevice);
    if (n_e && e == hipSuccess) e = hipMemcpy(d_ems, ems.data(), ems_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rad, rad.data(), rad_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const RenderConst rc = make_render_const(*p, f, n_e);
        FwdConst fc;
        fc.em_radiance = d_rad; fc.tan_mats = tan_materials; fc.tan_ems = n_e ? tan_emitters : d_rad;
        fc.tan_texels = (s->n_texels && s->dev.texels) ? tan_texels : nullptr;
        if (tan_tints)
            e = launch_fwd_tint(s->dev, d_ems, s->cam, f, rc, fc, p->pixel_begin, p->pixel_end, p->spp_total, pl, d_slots, tan_tints,
                                steady_hw3, transient_hwt3, c->stream);
        else
            e = launch_fwd(s->dev, d_ems, s->cam, f, rc, fc, p->pixel_begin, p->pixel_end, p->spp_total, pl, steady_hw3, transient_hwt3, c->stream);
    }
    const hipError_t e_sync = ws.release();
    HIP_TRY(c, e);
    HIP_TRY(c, e_sync);
    return MTR_OK;
}

int mtr_render_fwd(mtr_scene *s, const mtr_render_params *p, const float *tan_materials, const float *tan_emitters,
                   const float *tan_texels, float *steady_hw3, float *transient_hwt3)
{
    return render_fwd(s, p, tan_materials, tan_emitters, tan_texels, nullptr, steady_hw3, transient_hwt3);
}

int mtr_render_fwd_tint(mtr_scene *s, const mtr_render_params *p, const float *tan_materials, const float *tan_emitters,
                        const float *tan_texels, const float *tan_tints, float *steady_hw3, float *transient_hwt3)
{
    return render_fwd(s, p, tan_materials, tan_emitters, tan_texels, tan_tints, steady_hw3, transient_hwt3);
}

int mtr_counters_reset(mtr_ctx *c)
{
    if (!c) return fail(c, MTR_ERR_INVALID, "mtr_counters_reset: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, sizeof(DevCounters), c->stream));
    return MTR_OK;
}

int mtr_counters_read(mtr_ctx *c, mtr_counters *out)
{
    if (!c || !out) return fail(c, MTR_ERR_INVALID, "mtr_counters_read: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    return counters_to_abi(c, out);
}

int mtr_film_develop(mtr_ctx *c, const mtr_film_desc *fd, const float *t4, float *t3, const float *s4, float *s3)
{
    if (!c || !fd) return fail(c, MTR_ERR_INVALID, "mtr_film_develop: NULL argument");
    int rc = check_film(c, *fd);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_develop(film_from_desc(*fd), t4, t3, s4, s3, c->stream));
    return MTR_OK;
}

int mtr_splat_add(mtr_ctx *c, const mtr_splat_soa *s, const mtr_film_desc *fd, int variant, float *t4, float *elapsed_ms)
{
    if (!c || !s || !fd || !t4) return fail(c, MTR_ERR_INVALID, "mtr_splat_add: NULL argument");
    int rc = check_film(c, *fd);
    if (rc) return rc;
    const bool film_zero = (variant & MTR_SPLAT_FILM_ZERO) != 0;
    variant &= ~MTR_SPLAT_FILM_ZERO;
    if (variant != 0 && variant != 1) return fail(c, MTR_ERR_INVALID, "mtr_splat_add: variant must be 0 or 1 (| MTR_SPLAT_FILM_ZERO)");
    if (s->n && (!s->pixel || !s->opl || !s->r || !s->g || !s->b))
        return fail(c, MTR_ERR_INVALID, "mtr_splat_add: NULL splat array");
    HIP_TRY(c, hipSetDevice(c->device));
    Film fm = film_from_desc(*fd);
    if (fm.n_freq) {
        if (int r = grow_device_buffer(c, (void **)&c->d_freq, &c->freq_cap, (size_t)fm.n_freq * 4)) return r;
        HIP_TRY(c, hipMemcpyAsync(c->d_freq, fd->frequencies, (size_t)fm.n_freq * 4, hipMemcpyHostToDevice, c->stream));
        fm.freq = c->d_freq;
    }
    void *scratch = nullptr;
    if (variant == 1 && !fm.n_freq) {
        if (int r = grow_device_buffer(c, &c->d_runs, &c->runs_cap, 8u * ((size_t)fm.width * fm.height + 2u))) return r;
        scratch = c->d_runs;
    }
    if (elapsed_ms) HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    // variant 1: pixel-sorted input goes through the LDS rows as it is.  Anything else is PARTITIONED BY PIXEL on the device first
    // (mtr_splat.hip: two scatter passes over 16-byte records, then the same rows) when the film's shape allows it; that path
    // reads the sortedness flag back — one stream synchronisation — and holds 32 bytes of workspace per contribution for the call
    const bool can_partition = variant == 1 && scratch && splat_partition_supported(*s, fm);
    HIP_TRY(c, launch_splat_add(variant, *s, fm, t4, nullptr, scratch, c->stream, film_zero && variant == 1, !can_partition));
    bool second_leg = false;
    if (can_partition && s->n) {
        uint32_t unsorted = 0;
        if (elapsed_ms) HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&unsorted, scratch, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (unsorted) {
            // The workspace (32 B per contribution: 32 GiB for 2^30 of them) is raw device memory that torch's caching allocator
            // cannot see.  At most kPartRetain of it stays with the context between calls; a larger one is released before the
            // call returns (one more stream synchronisation — the call has blocked once already to read the flag).
            constexpr size_t kPartRetain = (size_t)256 << 20;
            const size_t need = splat_partition_scratch_bytes(*s, fm);
            hipError_t e = hipSuccess;
            if (c->part_cap < need) {
                if (c->d_part) (void)hipFree(c->d_part);
                c->d_part = nullptr; c->part_cap = 0;
                e = hipMalloc(&c->d_part, need);
                if (e == hipSuccess) c->part_cap = need; else { c->d_part = nullptr; (void)hipGetLastError(); }
            }
            // (timed calls: the passes below get their own pair of events — the allocation above is host time, not kernel time)
            if (elapsed_ms) { HIP_TRY(c, hipEventRecord(c->ev2, c->stream)); second_leg = true; }
            if (e != hipSuccess) HIP_TRY(c, launch_splat_add(0, *s, fm, t4, nullptr, nullptr, c->stream));     // no room for the workspace: the contract form
            else HIP_TRY(c, launch_splat_partitioned(*s, fm, t4, film_zero, nullptr, c->d_part, c->n_cu, c->stream));
            if (elapsed_ms) HIP_TRY(c, hipEventRecord(c->ev3, c->stream));
            if (c->part_cap > kPartRetain) {
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                (void)hipFree(c->d_part);
                c->d_part = nullptr; c->part_cap = 0;
            }
        }
    } else if (elapsed_ms) HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if (elapsed_ms) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipEventElapsedTime(elapsed_ms, c->ev0, c->ev1));
        if (second_leg) {
            float ms2 = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms2, c->ev2, c->ev3));
            *elapsed_ms += ms2;
        }
    }
    return MTR_OK;
}

int mtr_ctx_trim(mtr_ctx *c)
{
    if (!c) return MTR_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_part) (void)hipFree(c->d_part);
    c->d_part = nullptr; c->part_cap = 0;
    if (c->d_samples) (void)hipFree(c->d_samples);
    c->d_samples = nullptr; c->samples_cap = 0;
    if (c->d_start) (void)hipFree(c->d_start);
    c->d_start = nullptr; c->start_cap = 0;
    if (c->d_bp) (void)hipFree(c->d_bp);
    c->d_bp = nullptr; c->bp_cap = 0;
    return MTR_OK;
}

int mtr_backproject(mtr_ctx *c, const mtr_backproject_desc *d, const float *capture, float *volume)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_backproject: ctx is NULL");
    if (const char *why = bp_check(d, capture, volume)) return fail(c, MTR_ERR_INVALID, std::string("mtr_backproject: ") + why);
    const BpArgs a = bp_args(*d, capture);
    BpPlan pl;
    if (!bp_plan(a.nx, a.ny, a.nz, a.n_pairs, c->n_cu, pl)) return fail(c, MTR_ERR_INVALID, "mtr_backproject: the volume has too many voxels for one call");
    HIP_TRY(c, hipSetDevice(c->device));
    if (pl.n_slabs > 1u)
        if (int r = grow_device_buffer(c, &c->d_bp, &c->bp_cap, (size_t)pl.n_slabs * a.nx * a.ny * a.nz * sizeof(float))) return r;
    HIP_TRY(c, launch_backproject(a, pl, (float *)c->d_bp, volume, c->stream));
    return MTR_OK;
}

int mtr_forward_project(mtr_ctx *c, const mtr_backproject_desc *d, const float *volume, float *capture)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_forward_project: ctx is NULL");
    if (const char *why = bp_check(d, capture, volume)) return fail(c, MTR_ERR_INVALID, std::string("mtr_forward_project: ") + why);
    const BpArgs a = bp_args(*d, nullptr);
    FpPlan pl;
    if (!fp_plan(a.nx, a.ny, a.nz, a.n_pairs, a.T, c->n_cu, pl))
        return fail(c, MTR_ERR_INVALID, "mtr_forward_project: the volume has too many voxels, or the capture too many rows, for one call");
    HIP_TRY(c, hipSetDevice(c->device));
    if (pl.n_slabs > 1u)
        if (int r = grow_device_buffer(c, &c->d_bp, &c->bp_cap, (size_t)pl.n_slabs * a.n_pairs * a.T * sizeof(float))) return r;
    HIP_TRY(c, launch_forward_project(a, pl, volume, (float *)c->d_bp, capture, c->stream));
    return MTR_OK;
}

int mtr_phasor_backproject(mtr_ctx *c, const mtr_phasor_backproject_desc *d, const float *phasors, float *volume)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_phasor_backproject: ctx is NULL");
    if (const char *why = pb_check(d, phasors, volume)) return fail(c, MTR_ERR_INVALID, std::string("mtr_phasor_backproject: ") + why);
    const PbArgs a = pb_args(*d, phasors);
    BpPlan pl;
    if (!bp_plan(a.nx, a.ny, a.nz, a.n_pairs, c->n_cu, pl) || a.n_pairs > (0x7fffffffull * 256u) / a.F)
        return fail(c, MTR_ERR_INVALID, "mtr_phasor_backproject: the volume has too many voxels, or the capture too many phasors, for one call");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const size_t n = pb_weighted_floats(a) + pb_plane_floats(a, pl))
        if (int r = grow_device_buffer(c, &c->d_bp, &c->bp_cap, n * sizeof(float))) return r;
    HIP_TRY(c, launch_phasor_backproject(a, pl, (float *)c->d_bp, volume, c->stream));
    return MTR_OK;
}

int mtr_phasor_forward_project(mtr_ctx *c, const mtr_phasor_backproject_desc *d, const float *volume, float *phasors)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_phasor_forward_project: ctx is NULL");
    if (const char *why = pf_check(d, volume, phasors)) return fail(c, MTR_ERR_INVALID, std::string("mtr_phasor_forward_project: ") + why);
    const PbArgs a = pb_args(*d, nullptr);
    PfPlan pl;
    if (!pf_plan(a.nx, a.ny, a.nz, a.n_pairs, a.F, c->n_cu, pl))
        return fail(c, MTR_ERR_INVALID, "mtr_phasor_forward_project: the volume has too many voxels, or the capture too many rows, for one call");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const size_t n = pf_plane_floats(a, pl))
        if (int r = grow_device_buffer(c, &c->d_bp, &c->bp_cap, n * sizeof(float))) return r;
    HIP_TRY(c, launch_phasor_forward_project(a, pl, volume, (float *)c->d_bp, phasors, c->stream));
    return MTR_OK;
}

int mtr_fk_prepare(mtr_ctx *c, const mtr_fk_desc *d, const float *capture, const int32_t *shift, float *padded)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_fk_prepare: ctx is NULL");
    const char *why = fk_check(d, capture, padded);
    if (!why && !shift) why = "NULL argument";
    if (why) return fail(c, MTR_ERR_INVALID, std::string("mtr_fk_prepare: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_fk_prepare(fk_args(*d), capture, shift, padded, c->stream));
    return MTR_OK;
}

int mtr_fk_stolt(mtr_ctx *c, const mtr_fk_desc *d, const float *spectrum, float *resampled)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_fk_stolt: ctx is NULL");
    if (const char *why = fk_check(d, spectrum, resampled)) return fail(c, MTR_ERR_INVALID, std::string("mtr_fk_stolt: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_fk_stolt(fk_args(*d), spectrum, resampled, c->stream));
    return MTR_OK;
}

int mtr_fk_finish(mtr_ctx *c, const mtr_fk_desc *d, const float *field, float *volume)
{
    if (!c) return fail(nullptr, MTR_ERR_INVALID, "mtr_fk_finish: ctx is NULL");
    if (const char *why = fk_check(d, field, volume)) return fail(c, MTR_ERR_INVALID, std::string("mtr_fk_finish: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_fk_finish(fk_args(*d), field, volume, c->stream));
    return MTR_OK;
}

int mtr_render_samples_plan(mtr_scene *s, const mtr_render_params *p, uint32_t *slab_len, uint32_t *n_slabs, uint32_t *scene_in_lds, uint32_t *extended)
{
    if (!s || !p) return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_render_samples_plan: NULL argument");
    if (p->pixel_begin > p->pixel_end || p->spp_begin > p->spp_end) return fail(s->ctx, MTR_ERR_INVALID, "mtr_render_samples_plan: bad range");
    SamplesPlan pl{};
    if (int r = samples_check(s, p, p->pixel_end - p->pixel_begin, p->spp_end - p->spp_begin, &pl)) return r;
    if (slab_len) *slab_len = pl.slab_len;
    if (n_slabs) *n_slabs = pl.n_slabs;
    if (scene_in_lds) *scene_in_lds = pl.scene_lds ? 1u : 0u;
    if (extended) *extended = s->dev.has_rough ? 1u : 0u;
    return MTR_OK;
}

int mtr_scene_set_camera(mtr_scene *s, const mtr_camera *cam)
{
    if (!s || !cam) return fail(s ? s->ctx : nullptr, MTR_ERR_INVALID, "mtr_scene_set_camera: NULL argument");
    mtr_ctx *c = s->ctx;
    if (s->nlos.on) return fail(c, MTR_ERR_UNSUPPORTED, "mtr_scene_set_camera: not for the NLOS tier (its tables are derived from the sensor: mtr_scene_set_nlos)");
    memcpy(s->cam.s2c, cam->sample_to_camera, sizeof s->cam.s2c);
    memcpy(s->cam.tw, cam->to_world, sizeof s->cam.tw);
    s->cam.near_clip = cam->near_clip; s->cam.far_clip = cam->far_clip;
    return MTR_OK;
}

int mtr_debug_set_splat_log(mtr_scene *s, uint32_t *log_device, uint64_t capacity, uint64_t *n_records_device)
{
    if (!s) return MTR_ERR_INVALID;
    s->log.rec = log_device; s->log.cap = capacity; s->log.count = (unsigned long long *)n_records_device;
    if (!log_device || !n_records_device) { s->log.rec = nullptr; s->log.cap = 0; s->log.count = nullptr; }
    return MTR_OK;
}

} // extern "C"
