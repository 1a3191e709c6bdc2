// mtr_walk_kat.hip — the ray-query harness of mtr_core.h's walkers on the device (tests/test_gpu_walk.py).  A translation unit of its
// own: the kernels of every other file keep their instructions.  Nothing in the product calls it.
//
// The numerics contract says that a hit does not depend on the walker: culling is conservative, hits are decided by the primitive
// tests alone, ties by the original index.  Three walkers exist on the device only — wide_walk_device (primitives first), flat_walk_device
// (no tree walk at all) and the flat slab pairs — and a host build walks the tree instead.  This file asks each of them about single rays:
//
//   int mtr_test_dev_walk<suffix>(scene, form, n, o3, d3, tmax, hit4, occ)
//
// built ONCE PER FLAG SET as mtr_kat.hip is (among OTHERS; with $(KFLAGS) and -DMTR_KAT_SUFFIX=_k, how k_fused sees the header).  One
// launch on the null stream, 256 threads a workgroup, a grid-stride loop whose trip count is the same for every lane of a workgroup:
// a lane whose index is >= n walks a ray that cannot hit (tmax = 0) and stores nothing, so every ballot of a collective walker sees
// the whole wave.  Each ray runs the closest-hit walk and then the any-hit walk, as tests/host_harness.cpp's hh_walk does.
// The caller synchronises.  tests/walk_cases.py names the forms.
#include "mtr_kernels.h"
#include "mtr_flat_prims.h"

#ifndef MTR_KAT_SUFFIX
#define MTR_KAT_SUFFIX
#endif
#define KAT_CAT2(a, b) a##b
#define KAT_CAT(a, b) KAT_CAT2(a, b)
#define KAT_NAME(x) KAT_CAT(x, MTR_KAT_SUFFIX)

namespace mtr {
namespace {

// how the scene is staged and which instantiation of traverse() runs — each is one the product's kernels run
enum WalkForm : uint32_t {
    kWalkWideLds = 0,        // stage_scene<true>, WStack: wide_walk_device, ONE_PAIR as kTrLeafPair says
    kWalkWideLdsMulti = 1,   // ... the same scene with ONE_PAIR = false (the general leaf test)
    kWalkQ8Hbm = 2,          // stage_scene<false>: the quantised 8-wide tree in HBM
    kWalkQ4Hbm = 3,          // ... the quantised 4-wide tree (the hook's copy of SceneDev has wnodes8q = nullptr)
    kWalkFlatRefs = 4,       // stage_scene<true> with flat_off: flat_walk_device loading WNode::ref[k] (wavefront kernels, kTrFlatTop)
    kWalkFlatLeaves = 5,     // ... with TOP_LEAVES (kTrFlatLeaves)
    kWalkFlatTable = 6,      // ... over the child-ordered primitive table, one kernarg base (k_fused's lean kernels)
    kWalkFlatTableShadow = 7,  // ... the same walk for SHADOW RAYS: o3, d3, tmax hold (sp, gn, (u1, u2)) and the kernel builds each ray as
                               // shade_hit does, rect_emitter_point on the scene's emitter and shadow_ray_to
    kWalkFlatTableHull = 8,    // ... with the scene's ShadowHull (margin 1) in the argument and the any-hit walk's HULL tiers on
    kWalkForms = 9
};
// what the hook answers instead of launching
enum : int { kWalkErrArgs = -1, kWalkErrEmpty = -2, kWalkErrForm = -3, kWalkErrTraits = -4, kWalkErrNotFlat = -5, kWalkErrLds = -6, kWalkErrHull = -7 };

struct WalkArgs {
    SceneDev sc;
    uint64_t n;
    const float *o3, *d3, *tmax;
    uint32_t *hit4;
    uint8_t *occ;
    uint32_t stack_rows;
    ShadowHull hull;         // kWalkFlatTableHull: read at SceneView::hull_off
};

// (k_fused's lean stack names this form of kernarg_copy: mtr_core.h stack_one_kernarg_base)
struct WStackOneBase : WStack { [[maybe_unused]] static constexpr bool kOneKernargBase = true; };

constexpr bool walk_lds(uint32_t form) { return form != kWalkQ8Hbm && form != kWalkQ4Hbm; }
constexpr int walk_flat(uint32_t form) { return form == kWalkFlatLeaves ? 2 : (form == kWalkFlatRefs || form >= kWalkFlatTable) ? 1 : 0; }
constexpr bool walk_table(uint32_t form) { return form >= kWalkFlatTable; }
constexpr bool walk_shadow(uint32_t form) { return form == kWalkFlatTableShadow || form == kWalkFlatTableHull; }

template <uint32_t FORM, bool ONE_PAIR, bool SPH>
__global__ void __launch_bounds__(kBlock) KAT_NAME(k_walk)(const WalkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    constexpr bool kLds = walk_lds(FORM);
    constexpr int kFlat = walk_flat(FORM);
    typedef typename std::conditional<walk_table(FORM), WStackOneBase, WStack>::type Stack;
    static_assert(!walk_table(FORM) || flat_prim_table_on(true, false), "the lean kernels' table is built");
    uint32_t off = 0;
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    if constexpr (walk_table(FORM)) {
        // CHILD-ORDERED PRIMITIVE TABLE (mtr_core.h, mtr_flat_prims.h) in front of the staged tree, where flat_prim_fetch looks for
        // it: this file's own statement of k_fused's staging loop (mtr_kernels.hip keeps its instructions) — entry e, 20 words of the
        // record the reference names and then its first slot, zero where the top level has no such child
        const uint32_t nb = a.sc.flat.n_boxes, n_ent = flat_prim_entries(nb);
        unsigned char *tab = smem + off; off += flat_prim_bytes(nb);
        constexpr uint32_t kWords = kFlatPrimEntryBytes / 4u;
        for (uint32_t w = tid; w < n_ent * kWords; w += kBlock) {
            const uint32_t e = w / kWords, j = w - kWords * e;
            const bool quad = e < kFlatPrimQuads;
            const uint32_t b = quad ? 0u : (e - kFlatPrimQuads) / kFlatPrimFaces, f = quad ? e : (e - kFlatPrimQuads) - kFlatPrimFaces * b;
            const uint32_t node = quad ? 0u : a.sc.flat.node0 + b;
            uint32_t v = 0u;
            if ((!quad || e < a.sc.flat.n_quads) && node < a.sc.n_wnodes) {
                const uint32_t code = ~(uint32_t)a.sc.wnodes[node].ref[f];
                const uint32_t first = (quad ? code & ~kLeafQuadBit : code) >> 2;
                if (first < a.sc.n_slots) v = j < kWords - 1u ? ((const uint32_t *)(a.sc.tpairs + (first >> 1)))[j] : first;
            }
            *(uint32_t *)(tab + (j < kWords - 1u ? flat_prim_rec_off(e) + 4u * j : flat_prim_first_off(nb, e))) = v;
        }
    }
    SceneDev sc = a.sc;
    if (FORM == kWalkQ4Hbm) sc.wnodes8q = nullptr;
    SceneView sv = stage_scene<kLds>(sc, sc.ems, smem, off, tid, (uint32_t)(offsetof(WalkArgs, sc) + offsetof(SceneDev, flat)));
    sv.hull_off = (uint32_t)offsetof(WalkArgs, hull);
    __syncthreads();
    Stack st; st.base = s_stack + tid; st.sp = 0;
    // (whole workgroups of indices: i - tid is the same for every lane, so all 256 leave the loop together)
    const uint64_t n_up = (a.n + (uint64_t)kBlock - 1u) / (uint64_t)kBlock * (uint64_t)kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + (uint64_t)tid; i < n_up; i += (uint64_t)gridDim.x * kBlock) {
        const bool real = i < a.n;
        const uint64_t j = real ? i : 0u;
        f3 o = mk(a.o3[3 * j], a.o3[3 * j + 1], a.o3[3 * j + 2]);
        f3 d = mk(a.d3[3 * j], a.d3[3 * j + 1], a.d3[3 * j + 2]);
        float tmax;
        if constexpr (walk_shadow(FORM)) {
            const Ray r = shadow_ray_to(o, d, rect_emitter_point(sv.ems[0], a.tmax[2 * j], a.tmax[2 * j + 1]));
            o = r.o; d = r.d; tmax = real ? r.tmax : 0.0f;
        } else tmax = real ? a.tmax[j] : 0.0f;
        const Hit h = traverse<false, ONE_PAIR, kFlat, SPH>(sv, o, d, tmax, st);
        const Hit s = traverse<true, ONE_PAIR, kFlat, SPH, FORM == kWalkFlatTableHull>(sv, o, d, tmax, st);
        if (real) {
            a.hit4[4 * i] = fbits(h.t); a.hit4[4 * i + 1] = fbits(h.u); a.hit4[4 * i + 2] = fbits(h.v); a.hit4[4 * i + 3] = (uint32_t)h.prim;
            a.occ[i] = s.prim >= 0 ? 1 : 0;
        }
    }
}

template <uint32_t FORM, bool ONE_PAIR, bool SPH>
int walk_launch(const WalkArgs &a, size_t lds)
{
    const uint64_t g = (a.n + (uint64_t)kBlock - 1u) / (uint64_t)kBlock;
    return (int)launch_with_lds(KAT_NAME(k_walk)<FORM, ONE_PAIR, SPH>, a, (int)(g > 1024u ? 1024u : g), lds, (hipStream_t)0);
}

} // namespace
} // namespace mtr

// test hook of the library, outside the C ABI of include/mitransient_amd.h.  o3, d3 (n x 3), tmax (n), hit4 (n x 4: t, u, v bits and
// the slot of the closest hit, 0xffffffff for none) and occ (n: the any-hit walk found something) are device pointers; the shadow
// forms read (sp, gn) from o3, d3 and (u1, u2) from tmax (n x 2).  Returns the
// hipError_t of the launch, or a negative code — and launches nothing — for a form the scene's traits do not allow, a scene that does
// not fit LDS in an LDS form, a flat form of a scene without a flat top level, the hull form
// of a scene whose hull count is 0, and n == 0.
extern "C" int KAT_NAME(mtr_test_dev_walk)(const mtr_scene *scene, uint32_t form, uint64_t n, const float *o3, const float *d3, const float *tmax,
                                           uint32_t *hit4, uint8_t *occ)
{
    using namespace mtr;
    if (!scene) return kWalkErrArgs;
    if (n == 0u) return kWalkErrEmpty;
    if (!o3 || !d3 || !tmax || !hit4 || !occ) return kWalkErrArgs;
    if (form >= kWalkForms) return kWalkErrForm;
    WalkArgs a{};
    ShadowHull hull;
    if (mtr_test_scene_dev(scene, &a.sc, &hull) != 0) return kWalkErrArgs;
    a.hull = shadow_hull_with_margin(hull, 1.0f);
    a.n = n; a.o3 = o3; a.d3 = d3; a.tmax = tmax; a.hit4 = hit4; a.occ = occ;
    const SceneDev &sc = a.sc;
    const uint32_t tr = sc.traits;
    const bool empty = sc.n_slots == 0u, lds = walk_lds(form), sph = tr_spheres(tr), pair = (tr & kTrLeafPair) != 0u;
    const int flat = walk_flat(form);
    if (flat && flat_kind(tr) == 0) return kWalkErrNotFlat;
    if (flat && flat != flat_kind(tr)) return kWalkErrTraits;                    // (TOP_LEAVES is a compile-time fact of the scene's kernels)
    if (flat && (sc.flat.n_boxes > kFlatMaxBoxes || sc.flat.n_quads > kWide || sc.flat.node0 + sc.flat.n_boxes > sc.n_wnodes)) return kWalkErrTraits;
    if (walk_shadow(form) && ((tr & kTrOneRectEmitter) == 0u || sc.n_ems != 1u)) return kWalkErrTraits;      // (the rays are aimed at THE emitter)
    if (form == kWalkFlatTableHull && a.hull.count == 0u) return kWalkErrHull;
    if (form == kWalkWideLdsMulti && sph) return kWalkErrTraits;                 // (the product has no <false, 0, SPH> walker it does not reach through kWalkWideLds)
    if (form == kWalkQ8Hbm && !empty && !sc.wnodes8q) return kWalkErrTraits;
    if (form == kWalkQ4Hbm && !empty && !sc.wnodes4) return kWalkErrTraits;
    if (lds && !empty && !scene_fits_lds(sc)) return kWalkErrLds;
    if (lds && empty && (sc.n_wnodes != 0u || flat)) return kWalkErrTraits;
    SceneDev walked = sc;
    if (form == kWalkQ4Hbm) walked.wnodes8q = nullptr;
    a.stack_rows = wf_stack_rows(walked, lds);
    if (a.stack_rows > 66u) return kWalkErrTraits;                               // (the walkers' stacks end at 64 levels)
    const size_t bytes = (size_t)a.stack_rows * kBlock * 4u + (walk_table(form) ? flat_prim_bytes(sc.flat.n_boxes) : 0u) +
                         (lds ? lds_scene_bytes(sc) : 0u);
    if (bytes > kLdsCu) return kWalkErrLds;
    switch (form) {
    case kWalkWideLds:
        return sph ? walk_launch<kWalkWideLds, false, true>(a, bytes)
                   : pair ? walk_launch<kWalkWideLds, true, false>(a, bytes) : walk_launch<kWalkWideLds, false, false>(a, bytes);
    case kWalkWideLdsMulti: return walk_launch<kWalkWideLdsMulti, false, false>(a, bytes);
    case kWalkQ8Hbm: return sph ? walk_launch<kWalkQ8Hbm, false, true>(a, bytes) : walk_launch<kWalkQ8Hbm, false, false>(a, bytes);
    case kWalkQ4Hbm: return sph ? walk_launch<kWalkQ4Hbm, false, true>(a, bytes) : walk_launch<kWalkQ4Hbm, false, false>(a, bytes);
    case kWalkFlatRefs: return pair ? walk_launch<kWalkFlatRefs, true, false>(a, bytes) : walk_launch<kWalkFlatRefs, false, false>(a, bytes);
    case kWalkFlatLeaves: return pair ? walk_launch<kWalkFlatLeaves, true, false>(a, bytes) : walk_launch<kWalkFlatLeaves, false, false>(a, bytes);
    case kWalkFlatTable: return pair ? walk_launch<kWalkFlatTable, true, false>(a, bytes) : walk_launch<kWalkFlatTable, false, false>(a, bytes);
    case kWalkFlatTableShadow: return pair ? walk_launch<kWalkFlatTableShadow, true, false>(a, bytes) : walk_launch<kWalkFlatTableShadow, false, false>(a, bytes);
    default: return pair ? walk_launch<kWalkFlatTableHull, true, false>(a, bytes) : walk_launch<kWalkFlatTableHull, false, false>(a, bytes);
    }
}
