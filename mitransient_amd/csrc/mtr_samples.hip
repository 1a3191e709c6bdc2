// mtr_samples.hip — MTR_MODE_SAMPLES (ABI 24): the sample-parallel organisation of transient_path.  A translation unit of its
// own: the kernels of every other file keep their instructions.
//
// The fused and the wavefront organisations hand a whole pixel to ONE workgroup; a one-pixel film (a `radiancemeter`, a SPAD
// looking along a line) or a film of a few pixels with millions of samples therefore runs on a handful of workgroups.  Here the
// work item is (pixel, slab), a slab a contiguous range of the call's samples of that pixel (samples_plan):
//
//   k_samples_paths   a workgroup stages the scene with stage_scene (mtr_kernels.h: LDS when it fits, HBM walk otherwise), keeps ONE row of
//                     3 T f32 time bins + steady RGB + sample count in LDS, walks the slab's lanes through path_bounce — the
//                     general shading code, lane identity = RNG identity as every organisation — with an LDS-row sink, and
//                     stores the row once to its own slot of `partial` (pixels, slabs, 3 T + 4).  No global atomics on the film.
//   k_samples_reduce  one thread per film word: the slabs of its pixel summed in slab order and ADDED into transient_hwt4 /
//                     steady_hw4 (mtr_render's contract: R, G, B, W = 0; steady sums with the count in .w); the transient word
//                     is stored instead under MTR_FLAG_FILM_ZERO.
#include "mtr_kernels.h"
#include "mtr_samples_args.h"

#include <hip/hip_runtime.h>
#include <algorithm>

namespace mtr {

namespace {

// the workgroup's row: [T][3] f32, LDS float atomics
struct LdsRowSink {
    float *row;
    uint32_t n_splats;
    __device__ __forceinline__ void splat(uint32_t, uint32_t, uint32_t bin, float r, float g, float b, float, uint32_t, uint32_t)
    {
        float *p = row + 3u * bin;
        __hip_atomic_fetch_add(p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(p + 1, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(p + 2, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ++n_splats;
    }
};

template <bool SCENE_LDS, bool EXT>
__global__ void __launch_bounds__(kBlock) k_samples_paths(const SamplesArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const uint32_t row_n = samples_row_words(a.film);            // 3 T + 4
    uint32_t off = 0;
    float *s_row = (float *)smem; off += al16(row_n * 4u);
    unsigned long long *s_cnt = (unsigned long long *)(smem + off); off += 48u;      // paths, closest, shadow, splats, bounces (DevCounters order)
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    if (tid < 5) s_cnt[tid] = 0ull;
    const SceneView sv = stage_scene<SCENE_LDS>(a.sc, a.sc.ems, smem, off, tid);      // (the first item's barrier covers it)
    WStack st; st.base = s_stack + tid; st.sp = 0;
    const bool unwarp = (a.rc.flags & MTR_FLAG_CAMERA_UNWARP) != 0u;
    const uint32_t n_items = a.n_pixels * a.n_slabs;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t pl = item / a.n_slabs, slab = item - pl * a.n_slabs;
        const uint32_t pixel = a.pixel_begin + pl;
        const uint32_t s0 = slab * a.slab_len;                                    // of the call's samples [0, spp_chunk)
        const uint32_t s1 = (a.spp_chunk - s0 < a.slab_len) ? a.spp_chunk : s0 + a.slab_len;      // ragged last slab
        for (uint32_t i = tid; i < row_n; i += kBlock) s_row[i] = 0.0f;
        __syncthreads();
        LdsRowSink sink{ s_row, 0u };
        uint32_t n_paths = 0u, n_bounces = 0u;
        BounceStats bs{ 0u, 0u };
        f3 Ls = mk(0, 0, 0); float ws = 0.0f;                                     // this thread's steady sums of the slab
        for (uint64_t s64 = (uint64_t)s0 + (uint32_t)tid; s64 < s1; s64 += kBlock) {       // (64-bit: s1 may be within kBlock of 2^32)
            const uint32_t s = (uint32_t)s64;
            Path p;
            path_begin(p, a.cam, a.film, a.rc, pixel, a.spp_begin + s);
            ++n_paths;
            // camera_unwarp: bounce 0's closest hit is the camera ray's (path_bounce's unwarp_here); the ray the reference traces
            // for it is counted, as in the other organisations
            if (unwarp) bs.closest++;
            st.reset();
            bool alive = true;
            while (alive) {
                alive = path_bounce<EXT, 0u>(p, sv, a.film, a.rc, st, sink, bs, NoRefresh(), unwarp);
                ++n_bounces;
            }
            const uint32_t fx = p.px - a.film.crop_x, fy = p.py - a.film.crop_y;
            if ((fx < a.film.width) & (fy < a.film.height)) {
                Ls = mk(Ls.x + p.L.x, Ls.y + p.L.y, Ls.z + p.L.z);
                ws += 1.0f;
            }
        }
        if (ws != 0.0f) {
            float *sp = s_row + 3u * a.film.tbins;
            __hip_atomic_fetch_add(sp, Ls.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(sp + 1, Ls.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(sp + 2, Ls.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(sp + 3, ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (n_paths) {
            atomicAdd(s_cnt + 0, (unsigned long long)n_paths);
            atomicAdd(s_cnt + 1, (unsigned long long)bs.closest);
            atomicAdd(s_cnt + 2, (unsigned long long)bs.shadow);
            atomicAdd(s_cnt + 3, (unsigned long long)sink.n_splats);
            atomicAdd(s_cnt + 4, (unsigned long long)n_bounces);
        }
        __syncthreads();
        float *out = a.partial + (size_t)item * row_n;
        for (uint32_t i = tid; i < row_n; i += kBlock) out[i] = s_row[i];
        __syncthreads();                                                          // (the row is zeroed again for the next item)
    }
    __syncthreads();
    if (tid < 5 && a.counters && s_cnt[tid]) atomicAdd(&a.counters->paths + tid, s_cnt[tid]);
}

// film words of the launch: [n_pixels][T][4] transient, then [n_pixels][4] steady
__global__ void __launch_bounds__(kBlock) k_samples_reduce(const SamplesArgs a)
{
    const uint32_t T = a.film.tbins, row_n = samples_row_words(a.film);
    const uint64_t n_t = (uint64_t)a.n_pixels * T * 4u, n_all = n_t + (uint64_t)a.n_pixels * 4u;
    const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w >= n_all) return;
    const bool steady = w >= n_t;
    const uint64_t v = steady ? w - n_t : w;
    const uint32_t ch = (uint32_t)(v & 3u);
    const uint32_t pl = steady ? (uint32_t)(v >> 2) : (uint32_t)(v / ((uint64_t)T * 4u));
    const uint32_t bin = steady ? 0u : (uint32_t)((v >> 2) - (uint64_t)pl * T);
    // the film tensor is addressed as the sinks address it: crop-window coordinates on rows of the film's width
    const uint32_t pixel = a.pixel_begin + pl;
    const uint32_t fy = fastdiv(pixel, a.rc.div_crop_w), fx = pixel - a.film.crop_w * fy;
    if (!((fx < a.film.width) & (fy < a.film.height))) return;
    const size_t fp = (size_t)fy * a.film.width + fx;
    float *dst = steady ? a.steady_out + fp * 4u + ch : a.film_out + (fp * T + bin) * 4u + ch;
    if (!steady && ch == 3u) {                                                    // W = 0: nothing to add
        if (a.film_zero) *dst = 0.0f;
        return;
    }
    const float *src = a.partial + (size_t)pl * a.n_slabs * row_n + (steady ? 3u * T + ch : 3u * bin + ch);
    float acc = 0.0f;
    for (uint32_t sl = 0; sl < a.n_slabs; ++sl) acc += src[(size_t)sl * row_n];
    if (!steady && a.film_zero) *dst = acc;
    else *dst += acc;
}

} // namespace

bool samples_plan(const SceneDev &sc, const Film &film, uint32_t n_pixels, uint32_t spp_chunk, int n_cu, SamplesPlan &pl)
{
    pl = SamplesPlan{};
    if (n_pixels == 0u || spp_chunk == 0u || n_cu <= 0) return false;
    const size_t row_b = al16(samples_row_words(film) * 4u) + 48u;               // the row and the workgroup's counters
    const uint32_t scene_b = lds_scene_bytes(sc);
    bool scene_lds = scene_fits_lds(sc);
    size_t lds = row_b + (size_t)wf_stack_rows(sc, scene_lds) * kBlock * 4u + (scene_lds ? scene_b : 0u);
    if (scene_lds && lds > kLdsCu && sc.wnodes4 != nullptr) {             // a long row beside the scene: walk the scene in HBM
        scene_lds = false;
        lds = row_b + (size_t)wf_stack_rows(sc, false) * kBlock * 4u;
    }
    if (lds > kLdsCu) return false;
    // (at most four per compute unit: the path kernel holds 145 - 171 VGPRs, two or three waves per SIMD)
    uint32_t per_cu = (uint32_t)(kLdsCu / lds);
    if (per_cu > 4u) per_cu = 4u;
    const uint64_t cap = (uint64_t)n_cu * per_cu;                                 // workgroups the device keeps resident
    // slabs per pixel: enough items to fill the device, a slab no shorter than one sample per thread of a workgroup
    const uint32_t most = (spp_chunk + kBlock - 1u) / kBlock;                     // (>= 1, <= spp_chunk)
    uint64_t want = (cap + n_pixels - 1u) / n_pixels;
    if (want > most) want = most;
    if (want < 1u) want = 1u;
    uint32_t slab_len = (uint32_t)(((uint64_t)spp_chunk + want - 1u) / want);
    slab_len = (uint32_t)std::min<uint64_t>(((uint64_t)slab_len + kBlock - 1u) / kBlock * kBlock, 0x80000000ull);      // whole workgroup passes
    const uint32_t n_slabs = (uint32_t)(((uint64_t)spp_chunk + slab_len - 1u) / slab_len);      // the last one ragged
    const uint64_t items = (uint64_t)n_pixels * n_slabs;
    if (items > 0xffffffffull) return false;
    pl.scene_lds = scene_lds; pl.lds_bytes = lds; pl.stack_rows = wf_stack_rows(sc, scene_lds);
    pl.slab_len = slab_len; pl.n_slabs = n_slabs;
    pl.grid = (uint32_t)(items < cap ? items : cap);
    pl.partial_bytes = (size_t)items * samples_row_words(film) * sizeof(float);
    return true;
}

hipError_t launch_samples(SamplesArgs a, const SamplesPlan &pl, hipStream_t stream)
{
    a.slab_len = pl.slab_len; a.n_slabs = pl.n_slabs; a.stack_rows = pl.stack_rows;
    const bool ext = a.sc.has_rough != 0u;
    const int grid = (int)pl.grid;
    hipError_t e = pl.scene_lds ? (ext ? launch_with_lds(k_samples_paths<true, true>, a, grid, pl.lds_bytes, stream)
                                       : launch_with_lds(k_samples_paths<true, false>, a, grid, pl.lds_bytes, stream))
                                : (ext ? launch_with_lds(k_samples_paths<false, true>, a, grid, pl.lds_bytes, stream)
                                       : launch_with_lds(k_samples_paths<false, false>, a, grid, pl.lds_bytes, stream));
    if (e != hipSuccess) return e;
    const uint64_t words = (uint64_t)a.n_pixels * ((uint64_t)a.film.tbins * 4u + 4u);
    hipLaunchKernelGGL(k_samples_reduce, dim3((uint32_t)((words + kBlock - 1u) / kBlock)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

const char *samples_kernel_name(const SceneDev &sc, const SamplesPlan &pl)
{
    const bool ext = sc.has_rough != 0u;
    return pl.scene_lds ? (ext ? "k_samples_paths<lds,ext>" : "k_samples_paths<lds,plain>")
                        : (ext ? "k_samples_paths<hbm,ext>" : "k_samples_paths<hbm,plain>");
}

} // namespace mtr

// test hook of the library, outside the C ABI of include/mitransient_amd.h: samples_plan over a bare description of the scene's
// LDS needs (no device): out = { slab_len, n_slabs, grid, scene_lds, lds_bytes }; returns 0 when nothing fits
extern "C" int mtr_test_samples_plan(uint32_t temporal_bins, uint32_t scene_lds_bytes, uint32_t wide_levels, uint32_t n_pixels,
                                     uint32_t spp_chunk, int n_cu, uint32_t *out)
{
    using namespace mtr;
    SceneDev sc{};
    // (a scene whose staged tables take scene_lds_bytes: lds_scene_bytes() sums the table sizes, the material table stands for all)
    sc.n_mats = scene_lds_bytes / (uint32_t)sizeof(mtr_material);
    sc.wnodes = scene_lds_bytes ? (const WNode *)(uintptr_t)16 : nullptr;          // never dereferenced by the plan
    sc.wnodes4 = (const QNode4 *)(uintptr_t)16;
    sc.wide_levels = wide_levels; sc.wide4_levels = wide_levels;
    Film f{};
    f.tbins = temporal_bins; f.bins = temporal_bins; f.lasers = 1u;
    SamplesPlan pl;
    if (!samples_plan(sc, f, n_pixels, spp_chunk, n_cu, pl)) return 0;
    out[0] = pl.slab_len; out[1] = pl.n_slabs; out[2] = pl.grid; out[3] = pl.scene_lds ? 1u : 0u; out[4] = (uint32_t)pl.lds_bytes;
    return 1;
}
