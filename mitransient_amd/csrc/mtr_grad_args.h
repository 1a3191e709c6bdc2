// mtr_grad_args.h — the argument block, the LDS slab and the shared launch pieces of the gradient kernels (mtr_grad.hip, mtr_grad_nlos.hip,
// mtr_grad_nlos_tex.hip, mtr_tint.hip)
#pragma once
#include "mtr_kernels.h"
#include "mtr_grad.h"
#include "mtr_grad_reduce.h"

#include <hip/hip_runtime.h>

namespace mtr {

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
    // texel gradients (appended: the fields above keep their places in the argument block of the kernels without texel code)
    uint32_t n_texels;            // texels of all textures (slab tier: 3 more doubles each behind the emitters' words)
    double *tex_acc;              // global tier: (n_texels, 3) f64, zeroed before the launch
    float *grad_texels;           // (n_texels, 3) f32: k_grad_reduce's / k_grad_tex_store's output
};

// ... and the NLOS tier's constants behind them (kernarg_copy reads them by offset)
struct GradNlosArgs {
    GradArgs g;
    NlosConst nlos;               // with unit irradiance: gc.em_radiance points at the true one
};

// one f64 atomic per non-zero word of a gradient (LDS or global, by the pointer)
__device__ __forceinline__ void add3_nonzero(double *p, f3 g)
{
    if (g.x != 0.0f) atomicAdd(p, (double)g.x);
    if (g.y != 0.0f) atomicAdd(p + 1, (double)g.y);
    if (g.z != 0.0f) atomicAdd(p + 2, (double)g.z);
}

// LDS slab of the workgroup's gradients
struct SlabAcc {
    double *slab; uint32_t n_mats;
    __device__ __forceinline__ void add_mat(uint32_t m, f3 g) { add3_nonzero(slab + 3u * m, g); }
    __device__ __forceinline__ void add_em(uint32_t e, f3 g) { add3_nonzero(slab + 3u * (n_mats + e), g); }
    __device__ __forceinline__ void vertex(uint32_t, float, bool) {}
    __device__ __forceinline__ void term(uint32_t, uint32_t, float, f3) {}
};

// the texel hooks of grad_walk / grad_nlos_walk (mtr_grad.h)
struct TexelSlab {                  // slab tier: LDS atomics into the workgroup's slab
    static constexpr bool kOn = true;
    double *t;
    __device__ __forceinline__ void operator()(uint32_t i, f3 g) const { add3_nonzero(t + 3u * i, g); }
};
struct TexelGlobal {                // global tier: one no-return global_atomic_add_f64 per non-zero word
    static constexpr bool kOn = true;
    double *t;
    __device__ __forceinline__ void operator()(uint32_t i, f3 g) const { add3_nonzero(t + 3u * (size_t)i, g); }
};
enum : int { kTexNone = 0, kTexSlab = 1, kTexGlobal = 2 };

// the fields of GradArgs that every gradient launch fills alike (launch_grad, launch_grad_tint)
GradArgs make_grad_args(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                        const GradConst &gc, uint32_t pixel_begin, uint32_t n_pixels, uint32_t spp_begin, uint32_t spp_chunk,
                        double *partial, uint32_t grid, bool scene_lds, float *grad_mats, float *grad_ems);
// what follows every paths kernel: k_grad_reduce over the rows of a.partial — the materials' and emitters' words and a third
// segment of n_third words (texels of the slab tier, or tints) to `third` — then, with tex_acc (the global texel tier),
// k_grad_tex_store
hipError_t launch_grad_reduce(const GradArgs &a, uint32_t n_third, float *third, bool tex_acc, hipStream_t stream);

// k_grad_paths_nlos<EXT> (mtr_grad_nlos.hip) over the lanes of `a`; launch_grad runs the reduction behind it
hipError_t launch_grad_paths_nlos(const GradArgs &a, const NlosConst &nlos_unit, bool ext, int grid, size_t lds, hipStream_t stream);
// k_grad_paths_nlos_tex<TEX> (mtr_grad_nlos_tex.hip; extended shading code) in tier MTR_GRAD_TEX_SLAB / _GLOBAL; launch_grad runs
// the reduction of the tier behind it
hipError_t launch_grad_paths_nlos_tex(const GradArgs &a, const NlosConst &nlos_unit, uint32_t tier, int grid, size_t lds, hipStream_t stream);

} // namespace mtr
