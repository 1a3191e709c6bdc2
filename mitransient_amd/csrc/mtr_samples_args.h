// mtr_samples_args.h — MTR_MODE_SAMPLES (mtr_samples.hip): the argument block of its two kernels, the slab plan and the launch
#pragma once
#include "mtr_kernels.h"

#include <hip/hip_runtime.h>

namespace mtr {

// words of a workgroup's row and of a slot of `partial`: [T][3] time bins, steady R G B, sample count
__host__ __device__ inline uint32_t samples_row_words(const Film &f) { return 3u * f.tbins + 4u; }

struct SamplesArgs {
    SceneDev sc;
    Camera cam; Film film; RenderConst rc;
    uint32_t pixel_begin, n_pixels;       // crop-window pixels [pixel_begin, pixel_begin + n_pixels)
    uint32_t spp_begin, spp_chunk;        // samples [spp_begin, spp_begin + spp_chunk) of every one of them
    uint32_t slab_len, n_slabs;           // slab k of a pixel: the call's samples [k slab_len, min((k + 1) slab_len, spp_chunk))
    uint32_t stack_rows;
    uint32_t film_zero;                   // MTR_FLAG_FILM_ZERO: k_samples_reduce stores the transient words
    float *partial;                       // [n_pixels][n_slabs][3 T + 4]
    float *film_out, *steady_out;         // (H, W, T, 4), (H, W, 4)
    DevCounters *counters;
};

// What samples_plan chooses for a render: the slabs, the LDS carve-up (scene staged in LDS or walked in HBM) and the grid.
struct SamplesPlan {
    bool scene_lds;
    size_t lds_bytes;
    uint32_t stack_rows;
    uint32_t slab_len, n_slabs;           // n_slabs <= ceil(spp_chunk / kBlock) <= spp_chunk: never more slabs than samples
    uint32_t grid;                        // workgroups: min(items, resident workgroups of the device)
    size_t partial_bytes;
};

// false: the row, the traversal stack (and the scene) exceed kLdsCu, the LDS of a compute unit
bool samples_plan(const SceneDev &sc, const Film &film, uint32_t n_pixels, uint32_t spp_chunk, int n_cu, SamplesPlan &pl);
// k_samples_paths over the plan's items, then k_samples_reduce (a.partial: pl.partial_bytes of device memory)
hipError_t launch_samples(SamplesArgs a, const SamplesPlan &pl, hipStream_t stream);
// the instantiation launch_samples runs: "k_samples_paths<lds|hbm,plain|ext>"
const char *samples_kernel_name(const SceneDev &sc, const SamplesPlan &pl);

} // namespace mtr
