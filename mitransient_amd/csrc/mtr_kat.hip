// mtr_kat.hip — the known-answer harness of mtr_core.h on the device (tests/test_gpu_kat.py).  A translation unit of its own: the
// kernels of every other file keep their instructions.  Nothing in the product calls it.
//
// The numerics contract says that the host build and the device build of mtr_core.h perform the same operations, and the Makefile
// that the two flag sets it compiles the header with round the same.  This file is built ONCE PER FLAG SET — among OTHERS (SLP
// vectoriser on, pairs packed: how the wavefront, gradient, tint, samples and reconstruction files see the header) and with $(KFLAGS)
// and -DMTR_KAT_SUFFIX=_k (how k_fused sees it) — and exports, per family of mtr_kat.h,
//
//   int mtr_test_dev_<family><suffix>(..., n, device pointers)
//
// a test hook of the library, outside the C ABI of include/mitransient_amd.h: one launch on the null stream of a kernel whose thread
// i evaluates element i (grid-stride loop, 256 threads a workgroup, no LDS, no atomics, no early return), returning the hipError_t
// of the launch.  The caller synchronises.  tests/host_harness.cpp runs the same elements through the host build (hh_<family>).
#include "mtr_kat.h"

#include <hip/hip_runtime.h>

#ifndef MTR_KAT_SUFFIX
#define MTR_KAT_SUFFIX
#endif
#define KAT_CAT2(a, b) a##b
#define KAT_CAT(a, b) KAT_CAT2(a, b)
#define KAT_NAME(x) KAT_CAT(x, MTR_KAT_SUFFIX)

namespace mtr {
namespace {

constexpr uint32_t kKatBlock = 256u, kKatMaxGrid = 2048u;

struct FalloffConst { uint32_t angular; float cutoff, cos_cutoff, cos_beam, inv_transition; };

#define KAT_LOOP(i, n) for (uint64_t i = (uint64_t)blockIdx.x * kKatBlock + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * kKatBlock)

__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_special)(int which, uint64_t n, const float *__restrict__ x, float *__restrict__ y)
{
    KAT_LOOP(i, n) y[i] = kat::special(which, x[i]);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_trig)(int which, uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    KAT_LOOP(i, n) kat::trig(which, n, i, in, out);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_warps)(int which, uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    KAT_LOOP(i, n) kat::warps(which, n, i, in, out);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_fresnel)(int which, uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    KAT_LOOP(i, n) kat::fresnel(which, n, i, in, out);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_angular_falloff)(const FalloffConst c, uint64_t n, const float *__restrict__ cos_theta,
                                                                             float *__restrict__ y)
{
    Emitter E{};
    E.angular = c.angular; E.cutoff = c.cutoff; E.cos_cutoff = c.cos_cutoff; E.cos_beam = c.cos_beam; E.inv_transition = c.inv_transition;
    KAT_LOOP(i, n) y[i] = angular_falloff(E, cos_theta[i]);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_bsdf_eval_pdf)(const mtr_material m, uint64_t n, const float *__restrict__ wi3,
                                                                           const float *__restrict__ wo3, float *__restrict__ val3, float *__restrict__ pdf)
{
    KAT_LOOP(i, n) kat::bsdf_eval_pdf(m, i, wi3, wo3, val3, pdf);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_bsdf_sample)(const mtr_material m, uint64_t n, const float *__restrict__ wi3,
                                                                         const float *__restrict__ u1, const float *__restrict__ ua,
                                                                         const float *__restrict__ ub, float *__restrict__ wo3,
                                                                         float *__restrict__ pdf, float *__restrict__ w3)
{
    KAT_LOOP(i, n) kat::bsdf_sample_one(m, i, wi3, u1, ua, ub, wo3, pdf, w3);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_rng)(uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    KAT_LOOP(i, n) kat::rng(n, i, in, out);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_film)(float start_opl, float bin_width, uint32_t tbins, uint32_t lasers, uint32_t n_freq,
                                                                  uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    const Film f = kat::film_of(start_opl, bin_width, tbins, lasers, n_freq);
    KAT_LOOP(i, n) kat::film(f, n, i, in, out);
}
__global__ void __launch_bounds__(kKatBlock) KAT_NAME(k_kat_pairs)(uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    KAT_LOOP(i, n) kat::pairs(n, i, in, out);
}

inline dim3 kat_grid(uint64_t n)
{
    const uint64_t g = (n + kKatBlock - 1u) / kKatBlock;
    return dim3((uint32_t)(g < 1u ? 1u : g > kKatMaxGrid ? kKatMaxGrid : g));
}

} // namespace
} // namespace mtr

#define KAT_LAUNCH(kernel, n, ...) \
    do { hipLaunchKernelGGL(mtr::KAT_NAME(kernel), mtr::kat_grid(n), dim3(mtr::kKatBlock), 0, (hipStream_t)0, __VA_ARGS__); return (int)hipGetLastError(); } while (0)

// test hooks of the library, outside the C ABI of include/mitransient_amd.h.  Array layouts: mtr_kat.h; the pointers are device
// pointers (the material and the emitter are read on the host and handed to the kernel by value)
extern "C" int KAT_NAME(mtr_test_dev_special)(int which, uint64_t n, const float *x, float *y) { KAT_LAUNCH(k_kat_special, n, which, n, x, y); }
extern "C" int KAT_NAME(mtr_test_dev_trig)(int which, uint64_t n, const uint32_t *in, uint32_t *out) { KAT_LAUNCH(k_kat_trig, n, which, n, in, out); }
extern "C" int KAT_NAME(mtr_test_dev_warps)(int which, uint64_t n, const uint32_t *in, uint32_t *out) { KAT_LAUNCH(k_kat_warps, n, which, n, in, out); }
extern "C" int KAT_NAME(mtr_test_dev_fresnel)(int which, uint64_t n, const uint32_t *in, uint32_t *out) { KAT_LAUNCH(k_kat_fresnel, n, which, n, in, out); }
extern "C" int KAT_NAME(mtr_test_dev_angular_falloff)(const mtr_emitter *e, uint64_t n, const float *cos_theta, float *y)
{
    const mtr::FalloffConst c{ e->angular, e->cutoff, e->cos_cutoff, e->cos_beam, e->inv_transition };
    KAT_LAUNCH(k_kat_angular_falloff, n, c, n, cos_theta, y);
}
extern "C" int KAT_NAME(mtr_test_dev_bsdf_eval_pdf)(const mtr_material *m, uint32_t n, const float *wi3, const float *wo3, float *val3, float *pdf)
{
    KAT_LAUNCH(k_kat_bsdf_eval_pdf, n, *m, (uint64_t)n, wi3, wo3, val3, pdf);
}
extern "C" int KAT_NAME(mtr_test_dev_bsdf_sample)(const mtr_material *m, uint32_t n, const float *wi3, const float *u1, const float *ua, const float *ub,
                                                  float *wo3, float *pdf, float *w3)
{
    KAT_LAUNCH(k_kat_bsdf_sample, n, *m, (uint64_t)n, wi3, u1, ua, ub, wo3, pdf, w3);
}
extern "C" int KAT_NAME(mtr_test_dev_rng)(uint64_t n, const uint32_t *in, uint32_t *out) { KAT_LAUNCH(k_kat_rng, n, n, in, out); }
extern "C" int KAT_NAME(mtr_test_dev_film)(float start_opl, float bin_width, uint32_t tbins, uint32_t lasers, uint32_t n_freq, uint64_t n,
                                           const uint32_t *in, uint32_t *out)
{
    KAT_LAUNCH(k_kat_film, n, start_opl, bin_width, tbins, lasers, n_freq, n, in, out);
}
extern "C" int KAT_NAME(mtr_test_dev_pairs)(uint64_t n, const uint32_t *in, uint32_t *out) { KAT_LAUNCH(k_kat_pairs, n, n, in, out); }
