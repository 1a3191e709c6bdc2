// mtr_tint.hip — mtr_render_grad_tint / mtr_render_fwd_tint (ABI 19): reverse- and forward-mode derivatives of transient_path with
// respect to the constant `specular_reflectance` / `specular_transmittance` of conductor, roughconductor, dielectric, thindielectric
// and roughdielectric, beside the albedo and radiance derivatives of mtr_render_grad / mtr_render_fwd (reference:
// integrators/common.py:215-409 — a BSDF's tint is an ordinary differentiable parameter there; semantics in DESIGN.md §2, the
// arithmetic in the tint hooks of mtr_grad.h / mtr_fwd.h).  A translation unit of its own, so that the kernels of mtr_grad.hip and
// mtr_fwd.hip keep their instructions.
//
//   k_grad_paths_tint<SCENE_LDS, EXT>       k_grad_paths with the tint hook: the workgroup's f64 LDS slab holds 3
//                  more words per tint slot behind the emitters' (LDS atomics), stored once to the workgroup's row of `partial`;
//                  k_grad_reduce (mtr_grad.hip) sums the longer rows, the tints its third segment: no global atomics, bitwise
//                  reproducible.
//   k_fwd_paths_tint<SCENE_LDS, EXT, ROWS>  k_fwd_paths with the tint hook: the same rows and global tiers, the same fwd_plan; only
//                  the lane arithmetic differs.
#include "mtr_kernels.h"
#include "mtr_tint_args.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

// the tint hook of grad_walk: LDS atomics into the slab's tint words
struct TintSlab {
    static constexpr bool kOn = true;
    double *t; const int32_t *slots;
    __device__ __forceinline__ void operator()(uint32_t m, uint32_t which, f3 g) const
    {
        const int32_t s = slots[2u * m + which];
        if (s < 0) return;
        add3_nonzero(t + 3u * (uint32_t)s, g);
    }
    __device__ __forceinline__ void lobes(uint32_t, int, int) const {}
};
// ... and of fwd_walk: the slot's tangent
struct TintTan {
    static constexpr bool kOn = true;
    const float *tan; const int32_t *slots;
    __device__ __forceinline__ const float *operator()(uint32_t m, uint32_t which) const
    {
        const int32_t s = slots[2u * m + which];
        return s < 0 ? nullptr : tan + 3u * (uint32_t)s;
    }
};

template <bool SCENE_LDS, bool EXT>
__global__ void __launch_bounds__(kBlock) k_grad_paths_tint(const GradTintArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const GradArgs &a = args.g;
    const int tid = threadIdx.x;
    const uint32_t slab_n = 3u * (a.n_mats + a.n_ems + args.n_tints);
    uint32_t off = 0;
    double *s_slab = (double *)smem; off += al16(slab_n * 8u);
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    for (uint32_t i = tid; i < slab_n; i += kBlock) s_slab[i] = 0.0;
    const SceneView sv = stage_scene<SCENE_LDS>(a.sc, a.ems_unit, smem, off, tid);
    __syncthreads();
    WStack st; st.base = s_stack + tid; st.sp = 0;
    SlabAcc acc{ s_slab, a.n_mats };
    const TintSlab tint{ s_slab + 3u * (a.n_mats + a.n_ems), args.tint_slots };
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t l = (uint64_t)blockIdx.x * kBlock + tid; l < a.n_lanes; l += stride) {
        const uint32_t pixel = a.pixel_begin + (uint32_t)(l / a.spp_chunk);
        const uint32_t s = a.spp_begin + (uint32_t)(l % a.spp_chunk);
        st.reset();
        grad_lane<EXT>(sv, a.cam, a.film, a.rc, a.gc, pixel, s, st, acc, NoTexelGrad(), tint);
    }
    __syncthreads();
    double *row = a.partial + (size_t)blockIdx.x * slab_n;
    for (uint32_t i = tid; i < slab_n; i += kBlock) row[i] = s_slab[i];
}

template <bool SCENE_LDS, bool EXT, bool ROWS>
__global__ void __launch_bounds__(kBlock) k_fwd_paths_tint(const FwdTintArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FwdArgs &a = args.f;
    const int tid = threadIdx.x;
    const uint32_t row_words = 3u * a.film.bins + 3u;
    uint32_t off = 0;
    float *s_rows = (float *)smem; off += ROWS ? al16(a.G * row_words * 4u) : 0u;
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    if (ROWS) for (uint32_t i = tid; i < a.G * row_words; i += kBlock) s_rows[i] = 0.0f;
    const SceneView sv = stage_scene<SCENE_LDS>(a.sc, a.ems_unit, smem, off, tid);
    __syncthreads();
    WStack st; st.base = s_stack + tid; st.sp = 0;
    const TintTan tint{ args.tan_tints, args.tint_slots };
    if constexpr (ROWS) {
        // runs of G pixels, their rows in LDS, stored once and developed: k_fwd_paths' loop
        const uint32_t bins3 = 3u * a.film.bins;
        for (uint32_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
            const uint32_t pix0 = a.pixel_begin + run * a.G;
            const uint32_t left = a.pixel_end - pix0, npx = left < a.G ? left : a.G;
            const uint64_t n = (uint64_t)npx * a.spp;
            for (uint64_t i = (uint64_t)tid; i < n; i += kBlock) {
                const uint32_t slot = a.G > 1u ? fastdiv((uint32_t)i, a.div_spp) : 0u;
                const uint32_t s = (uint32_t)(i - (uint64_t)slot * a.spp);
                st.reset();
                RowSink sink{ s_rows + slot * row_words, &a.film, a.rc.sample_scale };
                fwd_lane<EXT>(sv, a.cam, a.film, a.rc, a.fc, pix0 + slot, s, st, sink, tint);
            }
            __syncthreads();
            for (uint32_t k = 0; k < npx; ++k) {
                const uint32_t pixel = pix0 + k, py = fastdiv(pixel, a.rc.div_crop_w), px = pixel - a.film.crop_w * py;
                float *row = s_rows + k * row_words;
                if ((px < a.film.width) & (py < a.film.height)) {
                    const size_t pix = (size_t)py * a.film.width + px;
                    float *t_out = a.transient + pix * bins3;
                    for (uint32_t j = tid; j < bins3; j += kBlock) { t_out[j] = row[j]; row[j] = 0.0f; }
                    if (tid < 3) { a.steady[3u * pix + tid] = row[bins3 + tid]; row[bins3 + tid] = 0.0f; }
                } else
                    for (uint32_t j = tid; j < row_words; j += kBlock) row[j] = 0.0f;
            }
            __syncthreads();
        }
    } else {
        GlobalSink sink{ a.transient, a.steady, &a.film, a.rc.sample_scale };
        const uint64_t stride = (uint64_t)gridDim.x * kBlock, n_lanes = (uint64_t)(a.pixel_end - a.pixel_begin) * a.spp;
        for (uint64_t l = (uint64_t)blockIdx.x * kBlock + tid; l < n_lanes; l += stride) {
            const uint32_t pixel = a.pixel_begin + (uint32_t)(l / a.spp);
            const uint32_t s = (uint32_t)(l % a.spp);
            st.reset();
            fwd_lane<EXT>(sv, a.cam, a.film, a.rc, a.fc, pixel, s, st, sink, tint);
        }
    }
}

template <bool ROWS>
hipError_t launch_fwd_paths(const FwdTintArgs &a, bool sl, bool ext, int grid, size_t lds, hipStream_t stream)
{
    return sl ? (ext ? launch_with_lds(k_fwd_paths_tint<true, true, ROWS>, a, grid, lds, stream)
                     : launch_with_lds(k_fwd_paths_tint<true, false, ROWS>, a, grid, lds, stream))
              : (ext ? launch_with_lds(k_fwd_paths_tint<false, true, ROWS>, a, grid, lds, stream)
                     : launch_with_lds(k_fwd_paths_tint<false, false, ROWS>, a, grid, lds, stream));
}

} // namespace

hipError_t launch_grad_tint(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                            const GradConst &gc, uint32_t pixel_begin, uint32_t n_pixels, uint32_t spp_begin, uint32_t spp_chunk,
                            double *partial, uint32_t grid, size_t lds, bool scene_lds, float *grad_mats, float *grad_ems,
                            uint32_t n_tints, const int32_t *tint_slots, float *grad_tints, hipStream_t stream)
{
    GradTintArgs t{};
    t.g = make_grad_args(sc, ems_unit, cam, film, rc, gc, pixel_begin, n_pixels, spp_begin, spp_chunk, partial, grid, scene_lds, grad_mats, grad_ems);
    t.n_tints = n_tints; t.tint_slots = tint_slots; t.grad_tints = grad_tints;
    const bool ext = sc.has_rough != 0u;
    hipError_t e = scene_lds ? (ext ? launch_with_lds(k_grad_paths_tint<true, true>, t, (int)grid, lds, stream)
                                    : launch_with_lds(k_grad_paths_tint<true, false>, t, (int)grid, lds, stream))
                             : (ext ? launch_with_lds(k_grad_paths_tint<false, true>, t, (int)grid, lds, stream)
                                    : launch_with_lds(k_grad_paths_tint<false, false>, t, (int)grid, lds, stream));
    if (e != hipSuccess) return e;
    return launch_grad_reduce(t.g, n_tints, grad_tints, false, stream);
}

hipError_t launch_fwd_tint(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                           const FwdConst &fc, uint32_t pixel_begin, uint32_t pixel_end, uint32_t spp, const FwdPlan &pl,
                           const int32_t *tint_slots, const float *tan_tints, float *steady, float *transient, hipStream_t stream)
{
    if (pixel_begin >= pixel_end || spp == 0u) return hipSuccess;
    FwdTintArgs t{};
    t.f = make_fwd_args(sc, ems_unit, cam, film, rc, fc, pixel_begin, pixel_end, spp, pl, steady, transient);
    t.tint_slots = tint_slots; t.tan_tints = tan_tints;
    const bool ext = sc.has_rough != 0u;
    if (pl.tier == MTR_FWD_ROWS) return launch_fwd_paths<true>(t, pl.scene_lds, ext, (int)pl.grid, pl.lds, stream);
    hipError_t e = launch_fwd_zero(t.f, stream);
    if (e != hipSuccess) return e;
    return launch_fwd_paths<false>(t, pl.scene_lds, ext, (int)pl.grid, pl.lds, stream);
}

} // namespace mtr
