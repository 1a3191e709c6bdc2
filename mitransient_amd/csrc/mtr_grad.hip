// mtr_grad.hip — mtr_render_grad (ABI 15): reverse-mode gradients of transient_path with respect to the constant reflectance of
// `diffuse` materials and the constant radiance of `area` / `angulararea` emitters (reference: integrators/common.py:325-409,
// transientpath.py:88-326; semantics in DESIGN.md §2, the arithmetic in mtr_grad.h).
//
//   k_grad_paths   one lane per (pixel, sample), lane identity = RNG identity: the lane's path is walked twice from its seed
//                  (path replay, mtr_grad.h) through the general shading code, over the scene staged in LDS or walked in HBM.
//                  Each workgroup sums its gradients in an LDS slab of (n_materials + n_emitters) x 3 doubles (LDS atomics) and
//                  stores the slab once to its own row of `partial` — no global atomics on the handful of parameter addresses.
//   k_grad_reduce  one thread per gradient word: the rows of `partial`, in workgroup order, summed in f64 (f64 throughout: the
//                  terms of a random upstream gradient cancel, and an f32 slab would lose digits the tests compare).
#include "mtr_kernels.h"
#include "mtr_grad.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

struct GradArgs {
    SceneDev sc;
    const Emitter *ems_unit;      // the scene's emitter table with unit radiance
    Camera cam; Film film; RenderConst rc; GradConst gc;
    uint32_t pixel_begin, spp_begin, spp_chunk;
    uint64_t n_lanes;
    uint32_t n_mats, n_ems;       // slab: materials first, then emitters, 3 doubles each
    uint32_t stack_rows;
    double *partial;              // [gridDim.x][slab]
    float *grad_mats, *grad_ems;  // k_grad_reduce's outputs
    uint32_t n_rows;              // rows of `partial`
};

// LDS slab of the workgroup's gradients
struct SlabAcc {
    double *slab; uint32_t n_mats;
    __device__ __forceinline__ void add3(double *p, f3 g)
    {
        if (g.x != 0.0f) atomicAdd(p, (double)g.x);
        if (g.y != 0.0f) atomicAdd(p + 1, (double)g.y);
        if (g.z != 0.0f) atomicAdd(p + 2, (double)g.z);
    }
    __device__ __forceinline__ void add_mat(uint32_t m, f3 g) { add3(slab + 3u * m, g); }
    __device__ __forceinline__ void add_em(uint32_t e, f3 g) { add3(slab + 3u * (n_mats + e), g); }
    __device__ __forceinline__ void vertex(uint32_t, float, bool) {}
    __device__ __forceinline__ void term(uint32_t, uint32_t, float, f3) {}
};

template <bool SCENE_LDS, bool EXT>
__global__ void __launch_bounds__(kBlock) k_grad_paths(const GradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const uint32_t slab_n = 3u * (a.n_mats + a.n_ems);
    uint32_t off = 0;
    double *s_slab = (double *)smem; off += al16(slab_n * 8u);
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    for (uint32_t i = tid; i < slab_n; i += kBlock) s_slab[i] = 0.0;
    const SceneDev &sc = a.sc;
    SceneView sv;
    sv.n_emitters = sc.n_ems; sv.n_slots = sc.n_slots;
    sv.samp_tris = sc.samp_tris; sv.samp_vn = sc.samp_vn; sv.face_pmf = sc.face_pmf; sv.face_cdf = sc.face_cdf; sv.vnormals = sc.vnormals;
    sv.texels = sc.texels; sv.tex_info = sc.tex_info; sv.uvs = sc.uvs;
    sv.flat_off = 0u;                                   // (the flat top-level walk is not instantiated here)
    if (SCENE_LDS) {
        WNode *n = (WNode *)(smem + off); off += al16(sc.n_wnodes * sizeof(WNode));
        TriPair *tg = (TriPair *)(smem + off); off += al16(sc.n_slots / 2 * sizeof(TriPair));
        TriShade *ts = (TriShade *)(smem + off); off += al16(sc.n_slots * sizeof(TriShade));
        mtr_material *mm = (mtr_material *)(smem + off); off += al16(sc.n_mats * sizeof(mtr_material));
        Emitter *ee = (Emitter *)(smem + off); off += al16(sc.n_ems * sizeof(Emitter));
        cp16(n, sc.wnodes, al16(sc.n_wnodes * sizeof(WNode)), tid);
        cp16(tg, sc.tpairs, al16(sc.n_slots / 2 * sizeof(TriPair)), tid);
        cp16(ts, sc.tshade, al16(sc.n_slots * sizeof(TriShade)), tid);
        cp16(mm, sc.mats, al16(sc.n_mats * sizeof(mtr_material)), tid);
        cp16(ee, a.ems_unit, al16(sc.n_ems * sizeof(Emitter)), tid);
        sv.nodes = nullptr; sv.wnodes = n; sv.wnodes4 = nullptr; sv.wnodes8q = nullptr; sv.tpairs = tg; sv.tshade = ts; sv.mats = mm; sv.ems = ee;
        sv.node_pairs = true;
    } else {
        sv.nodes = sc.nodes; sv.tpairs = sc.tpairs; sv.tshade = sc.tshade; sv.mats = sc.mats; sv.ems = a.ems_unit;
        sv.wnodes = nullptr; sv.wnodes4 = sc.wnodes4; sv.wnodes8q = sc.wnodes8q;
        sv.node_pairs = false;
    }
    __syncthreads();
    WStack st; st.base = s_stack + tid; st.sp = 0;
    SlabAcc acc{ s_slab, a.n_mats };
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t l = (uint64_t)blockIdx.x * kBlock + tid; l < a.n_lanes; l += stride) {
        const uint32_t pixel = a.pixel_begin + (uint32_t)(l / a.spp_chunk);
        const uint32_t s = a.spp_begin + (uint32_t)(l % a.spp_chunk);
        st.reset();
        grad_lane<EXT>(sv, a.cam, a.film, a.rc, a.gc, pixel, s, st, acc);
    }
    __syncthreads();
    double *row = a.partial + (size_t)blockIdx.x * slab_n;
    for (uint32_t i = tid; i < slab_n; i += kBlock) row[i] = s_slab[i];
}

__global__ void __launch_bounds__(kBlock) k_grad_reduce(const GradArgs a)
{
    const uint32_t slab_n = 3u * (a.n_mats + a.n_ems);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= slab_n) return;
    double acc = 0.0;
    for (uint32_t r = 0; r < a.n_rows; ++r) acc += a.partial[(size_t)r * slab_n + i];
    if (i < 3u * a.n_mats) a.grad_mats[i] = (float)acc;
    else a.grad_ems[i - 3u * a.n_mats] = (float)acc;
}

template <bool SL, bool EXT>
hipError_t launch_paths(const GradArgs &a, int grid, size_t lds, hipStream_t stream)
{
    auto k = k_grad_paths<SL, EXT>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), lds, stream, a);
    return hipGetLastError();
}

} // namespace

uint32_t grad_grid(const SceneDev &sc, uint64_t n_lanes, int n_cu, size_t *lds_out, bool *scene_lds_out)
{
    const uint32_t slab_n = 3u * (sc.n_mats + sc.n_ems);
    const uint32_t scene_b = lds_scene_bytes(sc);
    const bool scene_lds = sc.wnodes != nullptr && scene_b <= 64u * 1024u;
    const uint32_t rows = wf_stack_rows(sc, scene_lds);
    const size_t lds = al16(slab_n * 8u) + (size_t)rows * kBlock * 4u + (scene_lds ? scene_b : 0u);
    *lds_out = lds; *scene_lds_out = scene_lds;
    if (lds > 160u * 1024u) return 0u;
    uint32_t per_cu = (uint32_t)((160u * 1024u) / lds);
    if (per_cu > 8u) per_cu = 8u;
    const uint64_t want = (n_lanes + kBlock - 1) / kBlock;
    const uint64_t cap = (uint64_t)n_cu * per_cu;
    return (uint32_t)(want < cap ? want : cap);
}

hipError_t launch_grad(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                       const GradConst &gc, uint32_t pixel_begin, uint32_t n_pixels, uint32_t spp_begin, uint32_t spp_chunk,
                       double *partial, uint32_t grid, size_t lds, bool scene_lds, float *grad_mats, float *grad_ems, hipStream_t stream)
{
    GradArgs a{};
    a.sc = sc; a.ems_unit = ems_unit; a.cam = cam; a.film = film; a.rc = rc; a.gc = gc;
    a.pixel_begin = pixel_begin; a.spp_begin = spp_begin; a.spp_chunk = spp_chunk;
    a.n_lanes = (uint64_t)n_pixels * spp_chunk;
    a.n_mats = sc.n_mats; a.n_ems = sc.n_ems;
    a.stack_rows = wf_stack_rows(sc, scene_lds);
    a.partial = partial; a.grad_mats = grad_mats; a.grad_ems = grad_ems; a.n_rows = grid;
    const bool ext = sc.has_rough != 0u;
    hipError_t e = scene_lds ? (ext ? launch_paths<true, true>(a, (int)grid, lds, stream) : launch_paths<true, false>(a, (int)grid, lds, stream))
                             : (ext ? launch_paths<false, true>(a, (int)grid, lds, stream) : launch_paths<false, false>(a, (int)grid, lds, stream));
    if (e != hipSuccess) return e;
    const uint32_t slab_n = 3u * (sc.n_mats + sc.n_ems);
    hipLaunchKernelGGL(k_grad_reduce, dim3((slab_n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace mtr
