// mtr_grad.hip — mtr_render_grad (ABI 15): reverse-mode gradients of transient_path with respect to the constant reflectance of
// `diffuse` materials and the constant radiance of `area` / `angulararea` emitters (reference: integrators/common.py:325-409,
// transientpath.py:88-326; semantics in DESIGN.md §2, the arithmetic in mtr_grad.h).
//
//   k_grad_paths   one lane per (pixel, sample), lane identity = RNG identity: the lane's path is walked twice from its seed
//                  (path replay, mtr_grad.h) through the general shading code, over the scene staged in LDS or walked in HBM
//                  (stage_scene, mtr_kernels.h).
//                  Each workgroup sums its gradients in an LDS slab of (n_materials + n_emitters) x 3 doubles (LDS atomics) and
//                  stores the slab once to its own row of `partial` — no global atomics on the handful of parameter addresses.
//   k_grad_reduce  one thread per gradient word: the rows of `partial`, in workgroup order, summed in f64 (f64 throughout: the
//                  terms of a random upstream gradient cancel, and an f32 slab would lose digits the tests compare) and stored
//                  to the word's segment: materials, emitters, then texels (slab tier) or tints (grad_reduce_segment,
//                  mtr_grad_reduce.h).
// Texel gradients (ABI 16, mtr_render_grad_tex; extended shading code only), in one of two tiers chosen by grad_tex_tier():
//   slab tier      the texel words extend the LDS slab behind the materials and emitters (k_grad_paths<.., true, kTexSlab>), and
//                  k_grad_reduce sums the rows, the texel words its third segment: no global atomics, bitwise reproducible.
//   global tier    bitmaps whose words do not fit: global_atomic_add_f64 into a zeroed (n_texels, 3) f64 buffer
//                  (k_grad_paths<.., true, kTexGlobal>, zero words skipped), converted to f32 by k_grad_tex_store.
// A launch without texel gradients runs the kernels it ran before (TEX = kTexNone: no texel code in them).
// The NLOS tier (ABI 17; mtr_grad_nlos.hip, a translation unit of its own so that the kernels here keep their instructions):
// k_grad_paths_nlos<EXT> walks grad_nlos_lane over the scene staged in LDS (every NLOS scene
// the project runs fits; one that does not is refused); with texel gradients (ABI 20) k_grad_paths_nlos_tex<TEX> of
// mtr_grad_nlos_tex.hip, in the two tiers above, followed by the same reductions.  The laser is the slab's one "emitter": its
// three words sit behind the materials', and k_grad_reduce stores them to grad_emitters[0].  The ~110 dwords of NlosConst are re-read from the kernarg segment
// after every traversal (kernarg_copy, as k_fused<NLOS> does) instead of living in scalar registers through four walks per bounce.
#include "mtr_kernels.h"
#include "mtr_grad.h"
#include "mtr_grad_args.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

template <bool SCENE_LDS, bool EXT, int TEX = kTexNone>
__global__ void __launch_bounds__(kBlock) k_grad_paths(const GradArgs a)
{
    static_assert(TEX == kTexNone || EXT, "a bitmap implies the extended shading code");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const uint32_t slab_n = 3u * (a.n_mats + a.n_ems) + (TEX == kTexSlab ? 3u * a.n_texels : 0u);
    uint32_t off = 0;
    double *s_slab = (double *)smem; off += al16(slab_n * 8u);
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    for (uint32_t i = tid; i < slab_n; i += kBlock) s_slab[i] = 0.0;
    const SceneView sv = stage_scene<SCENE_LDS>(a.sc, a.ems_unit, smem, off, tid);
    __syncthreads();
    WStack st; st.base = s_stack + tid; st.sp = 0;
    SlabAcc acc{ s_slab, a.n_mats };
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t l = (uint64_t)blockIdx.x * kBlock + tid; l < a.n_lanes; l += stride) {
        const uint32_t pixel = a.pixel_begin + (uint32_t)(l / a.spp_chunk);
        const uint32_t s = a.spp_begin + (uint32_t)(l % a.spp_chunk);
        st.reset();
        if constexpr (TEX == kTexSlab) grad_lane<EXT>(sv, a.cam, a.film, a.rc, a.gc, pixel, s, st, acc, TexelSlab{ s_slab + 3u * (a.n_mats + a.n_ems) });
        else if constexpr (TEX == kTexGlobal) grad_lane<EXT>(sv, a.cam, a.film, a.rc, a.gc, pixel, s, st, acc, TexelGlobal{ a.tex_acc });
        else grad_lane<EXT>(sv, a.cam, a.film, a.rc, a.gc, pixel, s, st, acc);
    }
    __syncthreads();
    double *row = a.partial + (size_t)blockIdx.x * slab_n;
    for (uint32_t i = tid; i < slab_n; i += kBlock) row[i] = s_slab[i];
}

// one thread per word of a row: the rows of `partial`, in workgroup order, summed in f64 and stored as f32 to the word's segment
__global__ void __launch_bounds__(kBlock) k_grad_reduce(const GradReduceArgs r)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.slab_n) return;
    double acc = 0.0;
    for (uint32_t row = 0; row < r.n_rows; ++row) acc += r.partial[(size_t)row * r.slab_n + i];
    uint32_t at;
    const uint32_t k = grad_reduce_segment(r.n, i, &at);
    r.out[k][at] = (float)acc;
}

// global tier: the f64 sums to the f32 output
__global__ void __launch_bounds__(kBlock) k_grad_tex_store(const GradArgs a)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < 3u * (size_t)a.n_texels) a.grad_texels[i] = (float)a.tex_acc[i];
}

template <bool EXT, int TEX = kTexNone>
hipError_t launch_paths(const GradArgs &a, bool scene_lds, int grid, size_t lds, hipStream_t stream)
{
    return scene_lds ? launch_with_lds(k_grad_paths<true, EXT, TEX>, a, grid, lds, stream)
                     : launch_with_lds(k_grad_paths<false, EXT, TEX>, a, grid, lds, stream);
}

} // namespace

uint32_t grad_tex_tier(const SceneDev &sc, uint32_t n_texels, bool nlos)
{
    if (n_texels == 0u || !sc.has_rough || !sc.texels) return MTR_GRAD_TEX_NONE;
    if ((uint64_t)n_texels * 24u > kGradTexSlabBytes) return MTR_GRAD_TEX_GLOBAL;
    // ... and the whole carve-up must still fit (grad_grid's own bound)
    const uint32_t scene_b = lds_scene_bytes(sc);
    const bool scene_lds = scene_fits_lds(sc);
    const size_t lds = al16((3u * (sc.n_mats + (nlos ? 1u : sc.n_ems)) + 3u * n_texels) * 8u) + (size_t)wf_stack_rows(sc, scene_lds) * kBlock * 4u +
                       (scene_lds ? scene_b : 0u);
    return lds <= kLdsCu ? MTR_GRAD_TEX_SLAB : MTR_GRAD_TEX_GLOBAL;
}

uint32_t grad_grid(const SceneDev &sc, uint64_t n_lanes, int n_cu, size_t *lds_out, bool *scene_lds_out, uint32_t slab_texels, bool nlos)
{
    const uint32_t slab_n = 3u * (sc.n_mats + (nlos ? 1u : sc.n_ems)) + 3u * slab_texels;
    const uint32_t scene_b = lds_scene_bytes(sc);
    const bool scene_lds = scene_fits_lds(sc);
    const uint32_t rows = wf_stack_rows(sc, scene_lds);
    const size_t lds = al16(slab_n * 8u) + (size_t)rows * kBlock * 4u + (scene_lds ? scene_b : 0u);
    *lds_out = lds; *scene_lds_out = scene_lds;
    if (lds > kLdsCu || (nlos && !scene_lds)) return 0u;
    uint32_t per_cu = (uint32_t)(kLdsCu / lds);
    const uint32_t most = nlos ? (uint32_t)kGradNlosPerCu : 8u;
    if (per_cu > most) per_cu = most;
    const uint64_t want = (n_lanes + kBlock - 1) / kBlock;
    const uint64_t cap = (uint64_t)n_cu * per_cu;
    return (uint32_t)(want < cap ? want : cap);
}

GradArgs make_grad_args(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                        const GradConst &gc, uint32_t pixel_begin, uint32_t n_pixels, uint32_t spp_begin, uint32_t spp_chunk,
                        double *partial, uint32_t grid, bool scene_lds, float *grad_mats, float *grad_ems)
{
    GradArgs a{};
    a.sc = sc; a.ems_unit = ems_unit; a.cam = cam; a.film = film; a.rc = rc; a.gc = gc;
    a.pixel_begin = pixel_begin; a.spp_begin = spp_begin; a.spp_chunk = spp_chunk;
    a.n_lanes = (uint64_t)n_pixels * spp_chunk;
    a.n_mats = sc.n_mats; a.n_ems = sc.n_ems;
    a.stack_rows = wf_stack_rows(sc, scene_lds);
    a.partial = partial; a.grad_mats = grad_mats; a.grad_ems = grad_ems; a.n_rows = grid;
    return a;
}

hipError_t launch_grad_reduce(const GradArgs &a, uint32_t n_third, float *third, bool tex_acc, hipStream_t stream)
{
    GradReduceArgs r{};
    r.partial = a.partial; r.n_rows = a.n_rows;
    r.n[0] = 3u * a.n_mats; r.n[1] = 3u * a.n_ems; r.n[2] = 3u * n_third;
    r.out[0] = a.grad_mats; r.out[1] = a.grad_ems; r.out[2] = third;
    r.slab_n = r.n[0] + r.n[1] + r.n[2];
    hipLaunchKernelGGL(k_grad_reduce, dim3((r.slab_n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, r);
    if (tex_acc)
        hipLaunchKernelGGL(k_grad_tex_store, dim3((uint32_t)((3u * (size_t)a.n_texels + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_grad(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                       const GradConst &gc, uint32_t pixel_begin, uint32_t n_pixels, uint32_t spp_begin, uint32_t spp_chunk,
                       double *partial, uint32_t grid, size_t lds, bool scene_lds, float *grad_mats, float *grad_ems, hipStream_t stream,
                       uint32_t tex_tier, uint32_t n_texels, double *tex_acc, float *grad_texels, const NlosConst *nlos_unit)
{
    GradArgs a = make_grad_args(sc, ems_unit, cam, film, rc, gc, pixel_begin, n_pixels, spp_begin, spp_chunk, partial, grid, scene_lds,
                                grad_mats, grad_ems);
    a.n_texels = n_texels; a.tex_acc = tex_acc; a.grad_texels = grad_texels;
    const bool ext = sc.has_rough != 0u, tex = tex_tier != MTR_GRAD_TEX_NONE, slab = tex_tier == MTR_GRAD_TEX_SLAB;
    if (nlos_unit) {
        if (!scene_lds) return hipErrorInvalidValue;
        a.n_ems = 1u;                                   // the laser
    }
    if (tex && (!ext || !grad_texels || (tex_tier == MTR_GRAD_TEX_GLOBAL && !tex_acc))) return hipErrorInvalidValue;
    // the paths kernel of the tier ...
    hipError_t e;
    if (nlos_unit)
        e = tex ? launch_grad_paths_nlos_tex(a, *nlos_unit, tex_tier, (int)grid, lds, stream)
                : launch_grad_paths_nlos(a, *nlos_unit, ext, (int)grid, lds, stream);
    else if (tex)
        e = slab ? launch_paths<true, kTexSlab>(a, scene_lds, (int)grid, lds, stream) : launch_paths<true, kTexGlobal>(a, scene_lds, (int)grid, lds, stream);
    else
        e = ext ? launch_paths<true>(a, scene_lds, (int)grid, lds, stream) : launch_paths<false>(a, scene_lds, (int)grid, lds, stream);
    if (e != hipSuccess) return e;
    // ... then the one reduction: the slab tier's texel words are its third segment, the global tier's sums go through k_grad_tex_store
    return launch_grad_reduce(a, slab ? n_texels : 0u, slab ? grad_texels : nullptr, tex && !slab, stream);
}

} // namespace mtr
