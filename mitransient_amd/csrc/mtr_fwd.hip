// mtr_fwd.hip — mtr_render_fwd (ABI 18): forward-mode derivatives of transient_path, the tangent of the developed film for tangents
// of the constant `diffuse` reflectances, bitmap texels and emitter radiances (reference: integrators/common.py:215-323; semantics in
// DESIGN.md §2, the arithmetic in mtr_fwd.h).  A translation unit of its own, so that the kernels of mtr_grad.hip keep their
// instructions.
//
//   k_fwd_paths<SCENE_LDS, EXT, ROWS>   one lane per (pixel, sample), lane identity = RNG identity; the lane's path is walked ONCE
//                  through the general shading code with its log-derivative (fwd_walk), over the scene staged in LDS (when the
//                  tables fit: scene_fits_lds) or walked in HBM — stage_scene (mtr_kernels.h); the stack as k_grad_paths.
//   rows tier      a workgroup owns RUNS of G consecutive pixels (fwd_plan): run r = pixels [begin + r G, begin + (r + 1) G), its
//                  lanes i = slot * spp + s over trips of 256 — several pixels at once when spp < 256, several trips per pixel when
//                  spp > 256.  Every pixel in flight has an f32 LDS row of T x 3 words + 3 steady words; tangents arrive by
//                  ds_add_f32 (signed values of unknown range: no fixed point), and the finished row is stored once, coalesced and
//                  already developed, to transient[pixel] and steady[pixel].  No clear, no raw block, no develop pass, no global atomics.
//   global tier    a row that does not fit LDS beside the staged scene and the stack: lanes grid-strided as k_grad_paths,
//                  global_atomic_add_f32 onto outputs that k_fwd_zero cleared.
// The tier is a host function of scene and film alone (fwd_tier), reported by mtr_render_fwd_tier.
#include "mtr_kernels.h"
#include "mtr_fwd.h"
#include "mtr_fwd_args.h"

#include <hip/hip_runtime.h>

namespace mtr {

namespace {

template <bool SCENE_LDS, bool EXT, bool ROWS>
__global__ void __launch_bounds__(kBlock) k_fwd_paths(const FwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const uint32_t row_words = 3u * a.film.bins + 3u;
    uint32_t off = 0;
    float *s_rows = (float *)smem; off += ROWS ? al16(a.G * row_words * 4u) : 0u;
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    if (ROWS) for (uint32_t i = tid; i < a.G * row_words; i += kBlock) s_rows[i] = 0.0f;
    const SceneView sv = stage_scene<SCENE_LDS>(a.sc, a.ems_unit, smem, off, tid);
    __syncthreads();
    WStack st; st.base = s_stack + tid; st.sp = 0;
    if constexpr (ROWS) {
        const uint32_t bins3 = 3u * a.film.bins;
        for (uint32_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
            const uint32_t pix0 = a.pixel_begin + run * a.G;                 // (< pixel_end: n_runs = ceil(n_pixels / G))
            const uint32_t left = a.pixel_end - pix0, npx = left < a.G ? left : a.G;
            const uint64_t n = (uint64_t)npx * a.spp;
            for (uint64_t i = (uint64_t)tid; i < n; i += kBlock) {
                // (i < 2^32 except in the one-pixel run of a render with 2^32 samples per pixel: the quotient is 0 there)
                const uint32_t slot = a.G > 1u ? fastdiv((uint32_t)i, a.div_spp) : 0u;
                const uint32_t s = (uint32_t)(i - (uint64_t)slot * a.spp);
                st.reset();
                RowSink sink{ s_rows + slot * row_words, &a.film, a.rc.sample_scale };
                fwd_lane<EXT>(sv, a.cam, a.film, a.rc, a.fc, pix0 + slot, s, st, sink);
            }
            __syncthreads();
            // the finished rows, once and coalesced; the slots are cleared for the next run on the way
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
            fwd_lane<EXT>(sv, a.cam, a.film, a.rc, a.fc, pixel, s, st, sink);
        }
    }
}

// global tier: clears the rows and steady words of the launch's pixels
__global__ void __launch_bounds__(kBlock) k_fwd_zero(const FwdArgs a)
{
    const uint32_t bins3 = 3u * a.film.bins;
    for (uint32_t pixel = a.pixel_begin + blockIdx.x; pixel < a.pixel_end; pixel += gridDim.x) {
        const uint32_t py = fastdiv(pixel, a.rc.div_crop_w), px = pixel - a.film.crop_w * py;
        if (!((px < a.film.width) & (py < a.film.height))) continue;
        const size_t pix = (size_t)py * a.film.width + px;
        float *t_out = a.transient + pix * bins3;
        for (uint32_t j = threadIdx.x; j < bins3; j += kBlock) t_out[j] = 0.0f;
        if (threadIdx.x < 3) a.steady[3u * pix + threadIdx.x] = 0.0f;
    }
}

template <bool ROWS>
hipError_t launch_paths(const FwdArgs &a, bool sl, bool ext, int grid, size_t lds, hipStream_t stream)
{
    return sl ? (ext ? launch_with_lds(k_fwd_paths<true, true, ROWS>, a, grid, lds, stream)
                     : launch_with_lds(k_fwd_paths<true, false, ROWS>, a, grid, lds, stream))
              : (ext ? launch_with_lds(k_fwd_paths<false, true, ROWS>, a, grid, lds, stream)
                     : launch_with_lds(k_fwd_paths<false, false, ROWS>, a, grid, lds, stream));
}

} // namespace

hipError_t launch_fwd_zero(const FwdArgs &a, hipStream_t stream)
{
    const uint32_t n_pixels = a.pixel_end - a.pixel_begin;
    hipLaunchKernelGGL(k_fwd_zero, dim3(n_pixels < 65535u ? n_pixels : 65535u), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

uint32_t fwd_tier(const SceneDev &sc, const Film &film)
{
    const uint32_t scene_b = lds_scene_bytes(sc);
    const bool scene_lds = scene_fits_lds(sc);
    const uint64_t fixed = (uint64_t)wf_stack_rows(sc, scene_lds) * kBlock * 4u + (scene_lds ? scene_b : 0u);
    const uint64_t row_b = ((3ull * film.bins + 3ull) * 4ull + 15ull) & ~15ull;
    return fixed + row_b <= kLdsCu ? MTR_FWD_ROWS : MTR_FWD_GLOBAL;
}

// Row slots and grid.  A trip keeps min(256, G spp) lanes busy and a compute unit holds min(kFwdPerCu, 160 KiB / LDS(G)) workgroups:
// G is the slot count in [1, max(1, 256 / spp)] with the most busy lanes per compute unit, among those the one with the most
// resident workgroups (residency first), among those the largest.
bool fwd_plan(const SceneDev &sc, const Film &film, uint32_t n_pixels, uint32_t spp, int n_cu, FwdPlan &pl)
{
    const uint32_t scene_b = lds_scene_bytes(sc);
    pl.scene_lds = scene_fits_lds(sc);
    pl.stack_rows = wf_stack_rows(sc, pl.scene_lds);
    const uint64_t fixed = (uint64_t)pl.stack_rows * kBlock * 4u + (pl.scene_lds ? scene_b : 0u);
    if (fixed > kLdsCu) return false;
    pl.tier = fwd_tier(sc, film);
    const uint64_t n_lanes = (uint64_t)n_pixels * spp;
    if (pl.tier == MTR_FWD_GLOBAL) {
        pl.G = 0u; pl.n_runs = 0u; pl.lds = (size_t)fixed;
        uint32_t per_cu = (uint32_t)(kLdsCu / (fixed ? fixed : 1u));
        if (per_cu > 8u) per_cu = 8u;                                       // an oversubscribed grid, as grad_grid
        const uint64_t want = (n_lanes + kBlock - 1) / kBlock, cap = (uint64_t)n_cu * per_cu;
        pl.per_cu = per_cu; pl.grid = (uint32_t)(want < cap ? want : cap);
        return true;
    }
    const uint64_t row_words = 3ull * film.bins + 3ull;
    uint32_t g_max = spp >= (uint32_t)kBlock ? 1u : (uint32_t)kBlock / spp;
    if (g_max > n_pixels) g_max = n_pixels ? n_pixels : 1u;
    uint64_t best = 0; uint32_t best_g = 1u, best_cu = 1u; uint64_t best_lds = 0;
    for (uint32_t g = 1u; g <= g_max; ++g) {
        const uint64_t lds = fixed + ((g * row_words * 4ull + 15ull) & ~15ull);
        if (lds > kLdsCu) break;
        uint32_t per_cu = (uint32_t)(kLdsCu / lds);
        if (per_cu > (uint32_t)kFwdPerCu) per_cu = (uint32_t)kFwdPerCu;
        const uint64_t lanes = (uint64_t)g * spp < (uint64_t)kBlock ? (uint64_t)g * spp : (uint64_t)kBlock;
        const uint64_t busy = lanes * per_cu;
        if (busy > best || (busy == best && per_cu >= best_cu)) { best = busy; best_g = g; best_cu = per_cu; best_lds = lds; }
    }
    pl.G = best_g; pl.per_cu = best_cu; pl.lds = (size_t)best_lds;
    pl.n_runs = (n_pixels + best_g - 1u) / best_g;
    const uint64_t cap = (uint64_t)n_cu * best_cu;
    pl.grid = (uint32_t)(pl.n_runs < cap ? pl.n_runs : cap);
    return true;
}

FwdArgs make_fwd_args(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                      const FwdConst &fc, uint32_t pixel_begin, uint32_t pixel_end, uint32_t spp, const FwdPlan &pl,
                      float *steady, float *transient)
{
    FwdArgs a{};
    a.sc = sc; a.ems_unit = ems_unit; a.cam = cam; a.film = film; a.rc = rc; a.fc = fc;
    a.pixel_begin = pixel_begin; a.pixel_end = pixel_end; a.spp = spp; a.div_spp = fastdiv_make(spp);
    a.G = pl.G; a.n_runs = pl.n_runs; a.stack_rows = pl.stack_rows;
    a.steady = steady; a.transient = transient;
    return a;
}

hipError_t launch_fwd(const SceneDev &sc, const Emitter *ems_unit, const Camera &cam, const Film &film, const RenderConst &rc,
                      const FwdConst &fc, uint32_t pixel_begin, uint32_t pixel_end, uint32_t spp, const FwdPlan &pl,
                      float *steady, float *transient, hipStream_t stream)
{
    if (pixel_begin >= pixel_end || spp == 0u) return hipSuccess;
    const FwdArgs a = make_fwd_args(sc, ems_unit, cam, film, rc, fc, pixel_begin, pixel_end, spp, pl, steady, transient);
    const bool ext = sc.has_rough != 0u;
    if (pl.tier == MTR_FWD_ROWS) return launch_paths<true>(a, pl.scene_lds, ext, (int)pl.grid, pl.lds, stream);
    hipError_t e = launch_fwd_zero(a, stream);
    if (e != hipSuccess) return e;
    return launch_paths<false>(a, pl.scene_lds, ext, (int)pl.grid, pl.lds, stream);
}

} // namespace mtr
