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

// the film sinks of fwd_walk in the kernels (mtr_fwd.hip, mtr_tint.hip)
__device__ __forceinline__ void add3(float *p, f3 v)
{
    if (v.x != 0.0f) atomicAdd(p, v.x);
    if (v.y != 0.0f) atomicAdd(p + 1, v.y);
    if (v.z != 0.0f) atomicAdd(p + 2, v.z);
}

// rows tier: the lane's pixel row in LDS — [bins][3], then the three steady words
struct RowSink {
    float *row; const Film *film; float scale;
    __device__ __forceinline__ void splat(uint32_t, uint32_t, float opl, f3 dc) const
    {
        const int32_t bin = film_bin(*film, opl);
        if (bin >= 0) add3(row + 3u * (uint32_t)bin, mk(dc.x * scale, dc.y * scale, dc.z * scale));
    }
    __device__ __forceinline__ void steady(uint32_t, uint32_t, f3 sum) const
    {
        add3(row + 3u * film->bins, mk(sum.x * scale, sum.y * scale, sum.z * scale));
    }
};

// global tier: atomics onto the zeroed outputs
struct GlobalSink {
    float *transient, *steady_out; const Film *film; float scale;
    __device__ __forceinline__ void splat(uint32_t fx, uint32_t fy, float opl, f3 dc) const
    {
        if (!((fx < film->width) & (fy < film->height))) return;
        const int32_t bin = film_bin(*film, opl);
        if (bin >= 0) add3(transient + 3u * (((size_t)fy * film->width + fx) * film->bins + (uint32_t)bin), mk(dc.x * scale, dc.y * scale, dc.z * scale));
    }
    __device__ __forceinline__ void steady(uint32_t fx, uint32_t fy, f3 sum) const
    {
        if (!((fx < film->width) & (fy < film->height))) return;
        add3(steady_out + 3u * ((size_t)fy * film->width + fx), mk(sum.x * scale, sum.y * scale, sum.z * scale));
    }
};

// most workgroups of k_fwd_paths that a compute unit is asked to hold: what its registers allow (138 - 165 VGPRs: three waves per
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
// the argument block of such a launch (launch_fwd, launch_fwd_tint)
FwdArgs make_fwd_args(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                      const FwdConst &fc, uint32_t pixel_begin, uint32_t pixel_end, uint32_t spp, const FwdPlan &pl,
                      float *steady, float *transient);

// global tier: k_fwd_zero over the launch's pixels (clears their rows and steady words)
hipError_t launch_fwd_zero(const FwdArgs &a, hipStream_t stream);

} // namespace mtr
