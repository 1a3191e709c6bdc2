// mtr_fwd_args.h — the argument block, the plan and the launch interface of the forward-mode kernel (mtr_fwd.hip)
#pragma once
#include "mtr_kernels.h"
#include "mtr_fwd.h"

#include <hip/hip_runtime.h>

namespace mtr {

struct FwdArgs {
    SceneDev sc;
    const Emitter *ems_unit;      // the scene's emitter table with unit radiance
    Camera cam; Film film; RenderConst rc; FwdConst fc;
    uint32_t pixel_begin, pixel_end;   // crop-window pixels
    uint32_t spp;                 // samples per pixel: all of them, [0, spp_total)
    FastDiv div_spp;
    uint32_t G, n_runs;           // rows tier: row slots of a workgroup = pixels of a run, runs of this launch
    uint32_t stack_rows;
    float *steady;                // (H, W, 3)
    float *transient;             // (H, W, T, 3)
};

// most workgroups of k_fwd_paths that a compute unit is asked to hold: what its registers allow (132 - 163 VGPRs: three waves per
// SIMD, a workgroup being one wave on each)
constexpr int kFwdPerCu = 3;

struct FwdPlan {
    uint32_t tier;                // MTR_FWD_ROWS / MTR_FWD_GLOBAL
    bool scene_lds;
    uint32_t stack_rows;
    uint32_t G, n_runs;           // rows tier
    uint32_t per_cu, grid;
    size_t lds;
};

// the tier, a function of scene and film alone: rows when one pixel row fits LDS beside the staged scene and the stack
uint32_t fwd_tier(const SceneDev &sc, const Film &film);
// row slots, LDS carve-up and grid of a launch over n_pixels x spp lanes; false: not even the scene's stack fits LDS
bool fwd_plan(const SceneDev &sc, const Film &film, uint32_t n_pixels, uint32_t spp, int n_cu, FwdPlan &pl);
hipError_t launch_fwd(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                      const FwdConst &fc, uint32_t pixel_begin, uint32_t pixel_end, uint32_t spp, const FwdPlan &pl,
                      float *steady, float *transient, hipStream_t stream);

} // namespace mtr
