// mtr_grad_reduce.h — the argument block of k_grad_reduce (mtr_grad.hip) and its word-to-segment rule; plain C++ beside HIP, so that
// tests/host_grad_reduce.cpp checks the rule with a host compiler alone
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MTR_REDUCE_HD __host__ __device__ inline
#else
#define MTR_REDUCE_HD inline
#endif

namespace mtr {

// A row of `partial` is the workgroup's slab: the words of the materials, of the emitters, then optionally of the texels (slab tier)
// or the tints — each segment summed into an f32 output of its own.
constexpr uint32_t kGradSegments = 3u;
struct GradReduceArgs {
    const double *partial;        // [n_rows][slab_n]
    uint32_t n_rows, slab_n;      // slab_n = n[0] + n[1] + n[2]
    uint32_t n[kGradSegments];    // words of each segment; 0: the segment's pointer is never touched (it may be NULL)
    float *out[kGradSegments];
};

// the segment that holds word i < n[0] + n[1] + n[2] of a row, and the word's place in it: an empty segment is never chosen
MTR_REDUCE_HD uint32_t grad_reduce_segment(const uint32_t n[kGradSegments], uint32_t i, uint32_t *offset)
{
    uint32_t k = 0u;
    while (k + 1u < kGradSegments && i >= n[k]) { i -= n[k]; ++k; }
    *offset = i;
    return k;
}

} // namespace mtr
