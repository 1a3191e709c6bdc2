// mtr_tint_args.h — the argument blocks and the launch interface of the tint kernels (mtr_tint.hip; ABI 19, mtr_render_grad_tint /
// mtr_render_fwd_tint): the blocks of k_grad_paths / k_fwd_paths with the tint tables behind them, so that those kernels keep theirs.
#pragma once
#include "mtr_grad_args.h"
#include "mtr_fwd_args.h"

namespace mtr {

struct GradTintArgs {
    GradArgs g;                   // (n_texels, tex_acc, grad_texels: not used)
    uint32_t n_tints;             // tint slots: 3 more doubles each behind the emitters' words of the slab
    const int32_t *tint_slots;    // device [n_mats * 2]: tint_slot_table (mtr_scene_host.h)
    float *grad_tints;            // (n_tints, 3) f32: the third segment of k_grad_reduce's output
};

struct FwdTintArgs {
    FwdArgs f;
    const int32_t *tint_slots;    // device [n_mats * 2]
    const float *tan_tints;       // device (n_tints, 3)
};

// k_grad_paths_tint over the lanes of the launch (the arguments of launch_grad; grid and lds from grad_grid with n_tints more slab
// entries), then k_grad_reduce with the tints as its third segment: grad_mats, grad_ems and grad_tints
hipError_t launch_grad_tint(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                            const GradConst &gc, uint32_t pixel_begin, uint32_t n_pixels, uint32_t spp_begin, uint32_t spp_chunk,
                            double *partial, uint32_t grid, size_t lds, bool scene_lds, float *grad_mats, float *grad_ems,
                            uint32_t n_tints, const int32_t *tint_slots, float *grad_tints, hipStream_t stream);
// k_fwd_paths_tint: launch_fwd with the tint tangents (same plan, same tiers)
hipError_t launch_fwd_tint(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                           const FwdConst &fc, uint32_t pixel_begin, uint32_t pixel_end, uint32_t spp, const FwdPlan &pl,
                           const int32_t *tint_slots, const float *tan_tints, float *steady, float *transient, hipStream_t stream);

} // namespace mtr
