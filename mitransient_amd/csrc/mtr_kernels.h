// mtr_kernels.h — host-visible launch interface of the HIP kernels (internal to the library).
#pragma once
#include <hip/hip_runtime.h>
#include "mtr_core.h"
#include "mtr_nlos.h"
#include "mtr_start_blocks.h"

namespace mtr {

#ifndef MTR_BLOCK
#define MTR_BLOCK 256
#endif
constexpr int kBlock = MTR_BLOCK;    // 4 wave64 per workgroup (experiments: -DMTR_BLOCK=320 with -DMTR_FUSED_MIN_WAVES=5)

struct DevCounters {                 // device mirror of mtr_counters (u64 atomics)
    unsigned long long paths, rays_closest, rays_shadow, splats_issued, bounces, splats_overflow, r0, r1;
};

struct SceneDev {
    const Node *nodes; uint32_t n_nodes;
    const WNode *wnodes; uint32_t n_wnodes;                            // 8-wide tree over the same leaves (null for large scenes)
    const QNode4 *wnodes4; uint32_t n_wnodes4;                         // quantised 4-wide tree (always present)
    const QNode8 *wnodes8q; uint32_t n_wnodes8q;                       // quantised 8-wide tree (scenes walked in HBM; null: walk wnodes4)
    const TriPair *tpairs; const TriShade *tshade; uint32_t n_slots;   // triangle slots (even), see mtr_core.h
    const mtr_material *mats; uint32_t n_mats;
    const Emitter *ems; uint32_t n_ems;
    const q4 *samp_tris; const float *face_pmf, *face_cdf;   // mesh-emitter sampling tables (HBM; null without mesh emitters)
    const q4 *samp_vn;               // ... vertex normals of those meshes (null unless a mesh emitter has them)
    const q4 *vnormals;              // [3 * n_slots] vertex normals of smooth-shaded slots (HBM; null when every triangle is flat)
    const q4 *texels, *tex_info, *uvs;   // bitmap textures (HBM; null without): see SceneView
    uint32_t bvh_depth;
    uint32_t wide_levels, wide4_levels, wide8q_levels;   // levels of wnodes / wnodes4 / wnodes8q: a wide walk stacks at most one group per level
    uint32_t lds_bytes;              // bytes needed to stage the whole scene in LDS
    uint32_t traits;                 // kTr* bits (mtr_core.h) that hold for the material / emitter tables: kernels specialised on them are chosen
    uint32_t has_rough;              // the scene needs the EXTENDED shading code (kernels instantiated with ROUGH = true): a material
                                     // is a GGX lobe (MTR_BSDF_ROUGH*), or a triangle is smooth-shaded (vnormals)
    FlatTop flat;                    // traits & kTrFlatTop: the top level as scalar kernel arguments (mtr_core.h)
};

// streaming accesses (data touched once): non-temporal 16-byte load / store
__device__ __forceinline__ uint4 nt_load(const uint4 *p)
{
    const uint32_t *w = (const uint32_t *)p;
    return make_uint4(__builtin_nontemporal_load(w), __builtin_nontemporal_load(w + 1), __builtin_nontemporal_load(w + 2), __builtin_nontemporal_load(w + 3));
}
__device__ __forceinline__ float4 nt_load(const float4 *p)
{
    const float *w = (const float *)p;
    return make_float4(__builtin_nontemporal_load(w), __builtin_nontemporal_load(w + 1), __builtin_nontemporal_load(w + 2), __builtin_nontemporal_load(w + 3));
}
__device__ __forceinline__ void nt_store(float4 *p, float4 v)
{
    float *w = (float *)p;
    __builtin_nontemporal_store(v.x, w); __builtin_nontemporal_store(v.y, w + 1); __builtin_nontemporal_store(v.z, w + 2); __builtin_nontemporal_store(v.w, w + 3);
}

// per-lane traversal stack in LDS: column `tid` of kBlock-wide rows (the wavefront kernels, k_grad_paths)
struct WStack {
    static constexpr bool kPark = false;      // (k_fused's stack can park path state in LDS: mtr_kernels.hip)
    __device__ __forceinline__ void park_prev_p(mtr::f3) {}
    __device__ __forceinline__ mtr::f3 unpark_prev_p() const { return mtr::mk(0, 0, 0); }
    __device__ __forceinline__ void park_inc(uint64_t) {}
    __device__ __forceinline__ uint64_t unpark_inc() const { return 0; }
    __device__ __forceinline__ void park_prev_pdf(float) {}
    __device__ __forceinline__ float unpark_prev_pdf() const { return 0.0f; }
    int32_t *base; int sp;
    __device__ __forceinline__ void reset() { sp = 0; }
    __device__ __forceinline__ void push_if(bool c, int32_t v) { base[sp * kBlock] = v; sp += c ? 1 : 0; }
    __device__ __forceinline__ int32_t pop() { --sp; return base[sp * kBlock]; }
    __device__ __forceinline__ bool empty() const { return sp == 0; }
    __device__ __forceinline__ void prof_mark(int) {}
    __device__ __forceinline__ void prof_flat(int) {}
    __device__ __forceinline__ void count(int) {}
    __device__ __forceinline__ void tail(unsigned int) {}
};

// stage the scene in LDS: sizes, the copy, the stack rows a walk needs (one group per level of the tree walked, + 1: push_if writes
// before it counts)
__host__ __device__ constexpr uint32_t al16(uint32_t x) { return (x + 15u) & ~15u; }
__device__ __forceinline__ void cp16(void *dst, const void *src, uint32_t bytes, int tid)
{
    const uint4 *s = (const uint4 *)src; uint4 *d = (uint4 *)dst;
    for (uint32_t i = tid; i < bytes / 16u; i += kBlock) d[i] = s[i];
}
__host__ __device__ inline uint32_t wf_stack_rows(const SceneDev &sc, bool scene_lds) { return (scene_lds ? sc.wide_levels : (sc.wnodes8q ? sc.wide8q_levels : sc.wide4_levels)) + 1u; }
// bytes of the tables a kernel stages in LDS: 8-wide tree, triangle pairs, shading records, materials, emitters
__host__ __device__ inline uint32_t lds_scene_bytes(const SceneDev &sc)
{
    return al16(sc.n_wnodes * sizeof(WNode)) + al16(sc.n_slots / 2 * sizeof(TriPair)) + al16(sc.n_slots * sizeof(TriShade)) +
           al16(sc.n_mats * sizeof(mtr_material)) + al16(sc.n_ems * sizeof(Emitter));
}
// THE LDS RULES, shared by every kernel and its planner: a compute unit has 160 KiB, and a scene is staged when it has an 8-wide tree
// and its tables take at most 64 KiB (mtr_bvh.cpp's never_in_lds follows the same bound)
constexpr uint32_t kLdsCu = 160u * 1024u;
__host__ __device__ inline bool scene_fits_lds(const SceneDev &sc) { return sc.wnodes != nullptr && lds_scene_bytes(sc) <= 64u * 1024u; }

// The scene of a workgroup: staged in LDS at smem + off (lds_scene_bytes, in that order) or walked in HBM.  `ems` is the emitter
// table the kernel traces (the scene's, or a unit-radiance copy).  flat_off: where SceneDev::flat sits in the kernel's argument
// block, for the kernels that instantiate the flat top-level walk.  The caller synchronises before the first walk.
// (`off` by value and the statements in this order: k_grad_paths, k_fwd_paths and the tint kernels compile to the instructions they
// had with the block written out — profiles/deriv_harness_asm_diff.txt.)
template <bool SCENE_LDS>
__device__ __forceinline__ SceneView stage_scene(const SceneDev &sc, const Emitter *ems, unsigned char *smem, uint32_t off, int tid,
                                                 uint32_t flat_off = 0u)
{
    SceneView sv;
    sv.n_emitters = sc.n_ems; sv.n_slots = sc.n_slots;
    sv.samp_tris = sc.samp_tris; sv.samp_vn = sc.samp_vn; sv.face_pmf = sc.face_pmf; sv.face_cdf = sc.face_cdf; sv.vnormals = sc.vnormals;
    sv.texels = sc.texels; sv.tex_info = sc.tex_info; sv.uvs = sc.uvs;
    sv.flat_off = flat_off;
    if (SCENE_LDS) {
        WNode *n = (WNode *)(smem + off); off += al16(sc.n_wnodes * sizeof(WNode));
        TriPair *tg = (TriPair *)(smem + off); off += al16(sc.n_slots / 2 * sizeof(TriPair));
        TriShade *ts = (TriShade *)(smem + off); off += al16(sc.n_slots * sizeof(TriShade));
        mtr_material *mm = (mtr_material *)(smem + off); off += al16(sc.n_mats * sizeof(mtr_material));
        Emitter *ee = (Emitter *)(smem + off);
        cp16(n, sc.wnodes, al16(sc.n_wnodes * sizeof(WNode)), tid);
        cp16(tg, sc.tpairs, al16(sc.n_slots / 2 * sizeof(TriPair)), tid);
        cp16(ts, sc.tshade, al16(sc.n_slots * sizeof(TriShade)), tid);
        cp16(mm, sc.mats, al16(sc.n_mats * sizeof(mtr_material)), tid);
        cp16(ee, ems, al16(sc.n_ems * sizeof(Emitter)), tid);
        sv.nodes = nullptr; sv.wnodes = n; sv.wnodes4 = nullptr; sv.wnodes8q = nullptr; sv.tpairs = tg; sv.tshade = ts; sv.mats = mm; sv.ems = ee;
        sv.node_pairs = true;
    } else {
        sv.nodes = sc.nodes; sv.tpairs = sc.tpairs; sv.tshade = sc.tshade; sv.mats = sc.mats; sv.ems = ems;
        sv.wnodes = nullptr; sv.wnodes4 = sc.wnodes4; sv.wnodes8q = sc.wnodes8q;
        sv.node_pairs = false;
    }
    return sv;
}

// a kernel launch with `lds` bytes of dynamic LDS (above the 64 KiB a kernel gets unasked)
template <class K, class A>
hipError_t launch_with_lds(K kernel, const A &args, int grid, size_t lds, hipStream_t stream)
{
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, stream, args);
    return hipGetLastError();
}

struct SplatLog { uint32_t *rec; unsigned long long cap; unsigned long long *count; };

struct FusedArgs {
    SceneDev sc;
    Camera cam;
    Film film;
    RenderConst rc;
    uint32_t pixel_begin, pixel_end;     // crop-window pixels
    uint32_t spp_begin, spp_chunk;       // samples [spp_begin, spp_begin + spp_chunk)
    uint32_t G;                          // row slots of a workgroup's pixel ring (k_fused)
    FastDiv div_spp, div_G;              // i / spp_chunk, q / G without the ~35-instruction integer division
    uint32_t stack_rows;                 // rows of the per-lane LDS stack columns: levels of the wide tree walked + 1 (>= 3)
    uint32_t chunk, n_chunks;            // consecutive pixels per work ticket, number of tickets of this launch
    uint32_t *ticket;                    // device counter, zeroed before the launch (launch_fused)
    float *film_out;                     // (H, W, T, 4)
    float *steady_out;                   // (H, W, 4)
    DevCounters *counters;
    SplatLog log;
    uint32_t nlos_on;                    // 1: transient_nlos_path + nlos_capture_meter (nlos valid)
    float fixed_lim; uint32_t fixed_dcap;    // MTR_FLAG_DETERMINISTIC rows: what is summed in fixed point (LdsFixedSink's RANGE GUARD; fused_plan)
    // band completion words (mtr_render_params.n_bands): band b = pixels [b * band_px, (b + 1) * band_px) of the launch's range;
    // band_count[b] counts its flushed pixels (zeroed before the launch), band_done[b] receives band_epoch when it is complete
    uint32_t n_bands, band_px, band_epoch;
    uint32_t *band_count, *band_done;
    NlosConst nlos;
    // the path-start table of this launch (mtr_start_blocks.h; the lean flat-walk kernels: fused_start_blocks), start_table_bytes(grid, waves)
    // bytes of the context's; last, so that every other member keeps its place in the kernarg segment
    unsigned char *start_tab;
    // SHADOW HULL (mtr_core.h flat_walk_device, mtr_shadow_hull.h): the scene's block with this render's margin applied; count 0 switches
    // the shadow walk's tiers off.  Read by the flat-walk kernels of one rectangular emitter alone, at SceneView::hull_off.
    ShadowHull hull;
};

struct FusedConfig { int stack; bool scene_lds; bool hist_lds; bool fixed; bool rough; size_t lds_bytes; int grid; int per_cu; uint32_t traits; };

// k_fused's lean kernels count paths, bounces, shadow rays and contributions of a work ticket in 32-bit wave counters, drained
// between tickets.  What guarantees that none wraps is the kernel's own drain of a wave that has counted 2^30 bounces; this cap is no
// bound by itself (kChunkContribs is an AVERAGE a render is expected to stay under) — it cuts a ticket to pixels x spp_chunk x
// kChunkContribs < 2^32, never below one pixel, so that the drain inside the loop stays a branch ordinary renders do not take.
constexpr uint64_t kChunkContribs = 16u;
inline uint32_t fused_chunk_cap(uint32_t chunk, uint32_t spp_chunk)
{
    const uint64_t per_px = (uint64_t)(spp_chunk ? spp_chunk : 1u) * kChunkContribs;
    const uint64_t cap = ((1ull << 32) - 1ull) / per_px;          // chunk * per_px < 2^32
    if ((uint64_t)chunk > cap) chunk = (uint32_t)cap;
    return chunk < 1u ? 1u : chunk;
}

// pixels per work ticket of a launch of `grid` workgroups (fused_plan): about 32768 samples, at least two tickets per workgroup, capped as above
uint32_t fused_chunk(uint32_t n_pixels, uint32_t spp_chunk, uint32_t grid);
// chooses G, LDS carve-up and grid for a render; returns false if nothing fits
bool fused_plan(const SceneDev &sc, const Film &film, uint32_t n_pixels, uint32_t spp_chunk, int n_cu,
                FusedArgs &args, FusedConfig &cfg);
// bytes of the path-start table the kernel launch_fused picks for (args, cfg) reads through args.start_tab; 0: that kernel has none
// (one predicate for the caller that allocates and the launch that checks: a kernel never indexes a table nobody sized)
size_t fused_start_table_bytes(const FusedArgs &args, const FusedConfig &cfg);
hipError_t launch_fused(const FusedArgs &args, const FusedConfig &cfg, hipStream_t stream);
// NLOS prepare (transientnlospath.py:295-336): one ray per film pixel -> scanned points, + the laser's axis
hipError_t launch_nlos_prepare(const SceneDev &sc, const NlosConst &nc, q4 *targets, hipStream_t stream);

// ---- MTR_MODE_WAVEFRONT (mtr_wavefront.hip) ---------------------------------------------------
constexpr uint32_t kWfKeys = 5;        // material-type queues: diffuse, conductor, dielectric, none, miss

struct WfArgs {
    SceneDev sc;
    Camera cam;
    Film film;
    RenderConst rc;
    uint32_t pix0, P;                    // tile: crop-window pixels [pix0, pix0 + P)
    uint32_t spp_begin, S;               // samples [spp_begin, spp_begin + S) of every pixel of the tile
    uint32_t n_slots;                    // P * S
    uint32_t G, seg, n_seg;              // segment = G whole pixels = G * S slots, owned by one workgroup per launch
    uint32_t parity;                     // which of the two live lists this bounce reads
    uint32_t *ticket; uint32_t ticket_cur;   // segment tickets: two counters alternating between consecutive launches
    float *planes;                       // SoA state, PL_COUNT planes of n_slots
    uint32_t *q_live;                    // [2][n_slots] ping-pong live lists (slot indices), segment sg at sg * seg
    float4 *q_ray;                       // [2][n_slots][2] the rays of the live lists IN LIST ORDER: (o, tmax) (d, eta)
    uint32_t *seg_live;                  // [2][n_seg]   their lengths
    uint32_t *seg_list;                  // [2][n_seg]   the segments that HOLD live paths, per parity (the kernels of a bounce walk this list:
    uint32_t *seg_list_n;                // [2]          its length        a deep bounce of max_depth 65 touches a handful of 32768 segments)
    uint32_t *q_mat;                     // [kWfKeys][n_slots] material-sorted hit lists, same segmentation
    float4 *r_shadow;                    // [n_slots][2] those shadow rays, in list order: (o, tmax) (d, -)
    uint32_t *seg_shadow;                // [n_seg] their counts
    uint32_t *q_zombie;                  // [2][n_slots] scenes in HBM: paths that ended with an emitter-sampling term parked (Q_PEND), per parity
    uint32_t *seg_zombie;                // [2][n_seg] their counts
    uint8_t *occ;                        // [n_seg][occ_stride] shadow-ray results in the order of the segment's shadow list: 1 = occluded
    uint32_t occ_stride;                 // seg rounded up to 16 (the flags of a segment leave LDS as 16-byte stores)
    uint32_t trace_any;                  // k_wf_trace: 0 closest hits of the live lists, 1 occlusion of the shadow lists
    uint32_t first_bounce;               // k_wf_shade: this launch shades bounce 0 — the path state is rebuilt from (pixel, sample), not loaded
    uint32_t *seg_mat;                   // [n_seg][kWfKeys] their lengths
    uint32_t *live_total;                // optional: number of survivors of this bounce (unbounded-depth renders)
    uint4 *rec;                          // [P][rec_cap] time-bin records (bin, r, g, b)
    uint32_t *rec_count;                 // [P]
    uint32_t rec_cap;                    // 0: rows do not fit LDS -> contributions go straight to HBM atomics
    uint32_t film_zero;                  // film rows of this tile are zero on entry: the row flush stores
    float *film_out, *steady_out;
    DevCounters *counters;
    SplatLog log;
    uint32_t nlos_on;                    // NLOS tier in the wavefront organisation: raygen = nlos_begin, one k_wf_nlos_bounce per bounce
    NlosConst nlos;
    // (polarized transport keeps its Mueller / Stokes planes in the same allocation, behind the planes above: wf_polar_planes —
    // WfArgs itself is not extended, so that the argument layout of every existing kernel stays what it was)
};
struct WfConfig { int stack; bool scene_lds; size_t lds_bytes;
                  bool spheres = true; };      // the scene may hold analytic spheres (the caller knows: false picks the kernels without their code)

size_t wf_planes_bytes(uint32_t n_slots);
size_t wf_polar_planes_bytes(uint32_t n_slots);      // polarized transport: what follows wf_planes_bytes, rounded up to 16, in `planes`
bool wf_plan(const SceneDev &sc, WfConfig &cfg);
// Trace: closest hit + material-sorted queues, or occlusion when a.trace_any; Scatter: the time-bin (or phasor) scatter-add;
// NlosBounce / PolarBounce: one whole bounce of the NLOS tier / of polarized transport; PolarScatter: the Stokes scatter-add
enum class WfKernel { Raygen, Trace, Shade, Scatter, NlosBounce, PolarBounce, PolarScatter };
hipError_t launch_wf(const WfArgs &a, const WfConfig &cfg, WfKernel which, int grid, hipStream_t stream);

// scratch (variant 1): device buffer of >= 8 * (width * height + 2) bytes for the run table; NULL forces the atomics
hipError_t launch_splat_add(int variant, const mtr_splat_soa &s, const Film &film, float *film_out,
                            DevCounters *counters, void *scratch, hipStream_t stream, bool film_zero = false, bool fallback_atomics = true);
// device-side partition by pixel in front of the row kernel (mtr_splat.hip)
bool splat_partition_supported(const mtr_splat_soa &s, const Film &film);
size_t splat_partition_scratch_bytes(const mtr_splat_soa &s, const Film &film);
hipError_t launch_splat_partitioned(const mtr_splat_soa &s, const Film &film, float *film_out, bool film_zero, DevCounters *counters,
                                    void *scratch, int n_cu, hipStream_t stream);
hipError_t launch_develop(const Film &film, const float *t4, float *t3, const float *s4, float *s3, hipStream_t stream);

// mtr_render_grad / mtr_render_grad_tex (mtr_grad.hip): the grid of k_grad_paths (0: its LDS does not fit), then the kernels.
// Texel gradients run in one of two tiers (MTR_GRAD_TEX_*), decided by grad_tex_tier from the scene alone: the texel words join
// the workgroup's f64 LDS slab when all of them take at most kGradTexSlabBytes (slab_texels of grad_grid = n_texels: the grid keeps
// its occupancy rule over the larger slab), f64 global atomics into tex_acc otherwise.  8 KiB: a workgroup's share of the 160 KiB
// when eight are resident is 20 KiB, of which the traversal stack takes 4-16 KiB — a larger texel slab would cost resident
// workgroups on every scene staged in LDS; the rows of `partial` and k_grad_reduce's pass grow with it as well.
struct GradConst;
constexpr uint32_t kGradTexSlabBytes = 8u * 1024u;
uint32_t grad_tex_tier(const SceneDev &sc, uint32_t n_texels, bool nlos = false);     // nlos: the laser's words in the slab
// nlos (grad_grid) / nlos_unit (launch_grad: the scene's NlosConst with unit irradiance, gc.em_radiance = the true one): the NLOS
// tier — the laser takes the slab's three emitter words (grad_ems is (1, 3)), the scene must fit LDS, and at most kGradNlosPerCu
// workgroups per compute unit are asked for (the kernel's launch bound)
constexpr int kGradNlosPerCu = 3;
uint32_t grad_grid(const SceneDev &sc, uint64_t n_lanes, int n_cu, size_t *lds_out, bool *scene_lds_out, uint32_t slab_texels = 0u,
                   bool nlos = false);
hipError_t launch_grad(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                       const GradConst &gc, uint32_t pixel_begin, uint32_t n_pixels, uint32_t spp_begin, uint32_t spp_chunk,
                       double *partial, uint32_t grid, size_t lds, bool scene_lds, float *grad_mats, float *grad_ems, hipStream_t stream,
                       uint32_t tex_tier = 0u, uint32_t n_texels = 0u, double *tex_acc = nullptr, float *grad_texels = nullptr,
                       const NlosConst *nlos_unit = nullptr);

} // namespace mtr

// test hooks of the library, outside the C ABI of include/mitransient_amd.h: fused_chunk / fused_chunk_cap as the tests call them
extern "C" uint32_t mtr_test_fused_chunk(uint32_t n_pixels, uint32_t spp_chunk, uint32_t grid);
extern "C" uint32_t mtr_test_fused_chunk_cap(uint32_t chunk, uint32_t spp_chunk);
extern "C" void mtr_test_start_blocks(uint32_t n_lanes, uint32_t grid, uint32_t wg, uint32_t wave, uint32_t entry, uint32_t base, uint32_t *out);
extern "C" int mtr_test_start_blocks_sweep(uint32_t n_lo, uint32_t n_hi, uint32_t g_lo, uint32_t g_hi);
// the device ray-query harness of the walkers (mtr_walk_kat.hip, one hook per flag set; forms and error codes there) and the accessor
// it reads a scene through (mtr_api.hip)
extern "C" int mtr_test_scene_dev(const mtr_scene *s, mtr::SceneDev *dev, mtr::ShadowHull *hull);
extern "C" int mtr_test_dev_walk(const mtr_scene *scene, uint32_t form, uint64_t n, const float *o3, const float *d3, const float *tmax,
                                 uint32_t *hit4, uint8_t *occ);
extern "C" int mtr_test_dev_walk_k(const mtr_scene *scene, uint32_t form, uint64_t n, const float *o3, const float *d3, const float *tmax,
                                   uint32_t *hit4, uint8_t *occ);
