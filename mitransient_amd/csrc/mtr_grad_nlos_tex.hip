// mtr_grad_nlos_tex.hip — mtr_render_grad_tex on the NLOS tier (ABI 20): k_grad_paths_nlos_tex, k_grad_paths_nlos (mtr_grad_nlos.hip)
// with the texel hook of mtr_grad.h (grad_nlos_lane over nlos_bounce with NlosGradTexHook; semantics in DESIGN.md §2) in the two
// tiers of mtr_grad.hip.  A translation unit of its own: the kernels of mtr_grad.hip and mtr_grad_nlos.hip keep their instructions.
// k_grad_reduce of mtr_grad.hip follows it (slab tier: the texel words its third segment), and k_grad_tex_store on the global tier.
// The staging is k_grad_paths_nlos' own (see mtr_grad_nlos.hip).
#include "mtr_grad_args.h"

namespace mtr {

namespace {

// k_grad_paths_nlos<true> with texel gradients (its instantiations are named "nlos,lds,ext,slab" / "nlos,lds,ext,global"; a bitmap
// implies the extended shading code).  TEX = kTexSlab: the texel words (at most kGradTexSlabBytes) extend the f64 LDS slab behind
// the materials' and the laser's words and are stored with the row.  TEX = kTexGlobal: global_atomic_add_f64 into a.tex_acc, zero
// words skipped.  Three workgroups per compute unit, as k_grad_paths_nlos.
template <int TEX>
__global__ void __launch_bounds__(kBlock, kGradNlosPerCu) k_grad_paths_nlos_tex(const GradNlosArgs args)
{
    static_assert(TEX == kTexSlab || TEX == kTexGlobal, "a texel tier");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const GradArgs &a = args.g;
    const int tid = threadIdx.x;
    const uint32_t n_me = 3u * (a.n_mats + a.n_ems);
    const uint32_t slab_n = n_me + (TEX == kTexSlab ? 3u * a.n_texels : 0u);
    uint32_t off = 0;
    double *s_slab = (double *)smem; off += al16(slab_n * 8u);
    int32_t *s_stack = (int32_t *)(smem + off); off += a.stack_rows * kBlock * 4u;
    for (uint32_t i = tid; i < slab_n; i += kBlock) s_slab[i] = 0.0;
    const SceneDev &sc = a.sc;
    SceneView sv;
    sv.n_emitters = sc.n_ems; sv.n_slots = sc.n_slots;
    sv.samp_tris = sc.samp_tris; sv.samp_vn = sc.samp_vn; sv.face_pmf = sc.face_pmf; sv.face_cdf = sc.face_cdf; sv.vnormals = sc.vnormals;
    sv.texels = sc.texels; sv.tex_info = sc.tex_info; sv.uvs = sc.uvs;
    sv.flat_off = 0u;
    WNode *n = (WNode *)(smem + off); off += al16(sc.n_wnodes * sizeof(WNode));
    TriPair *tg = (TriPair *)(smem + off); off += al16(sc.n_slots / 2 * sizeof(TriPair));
    TriShade *ts = (TriShade *)(smem + off); off += al16(sc.n_slots * sizeof(TriShade));
    mtr_material *mm = (mtr_material *)(smem + off); off += al16(sc.n_mats * sizeof(mtr_material));
    cp16(n, sc.wnodes, al16(sc.n_wnodes * sizeof(WNode)), tid);
    cp16(tg, sc.tpairs, al16(sc.n_slots / 2 * sizeof(TriPair)), tid);
    cp16(ts, sc.tshade, al16(sc.n_slots * sizeof(TriShade)), tid);
    cp16(mm, sc.mats, al16(sc.n_mats * sizeof(mtr_material)), tid);
    sv.nodes = nullptr; sv.wnodes = n; sv.wnodes4 = nullptr; sv.wnodes8q = nullptr; sv.tpairs = tg; sv.tshade = ts; sv.mats = mm;
    sv.ems = sc.ems;                                    // (no surface emitter in a NLOS scene: never read)
    sv.node_pairs = true;
    __syncthreads();
    WStack st; st.base = s_stack + tid; st.sp = 0;
    SlabAcc acc{ s_slab, a.n_mats };
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t l = (uint64_t)blockIdx.x * kBlock + tid; l < a.n_lanes; l += stride) {
        const uint32_t pixel = a.pixel_begin + (uint32_t)(l / a.spp_chunk);
        const uint32_t s = a.spp_begin + (uint32_t)(l % a.spp_chunk);
        st.reset();
        // the ~140 dwords of projector / wall / table, film and render constants: from the kernarg segment after every traversal
        NlosConst nc_l = args.nlos; Film film_l = a.film; RenderConst rc_l = a.rc;
        auto reload = [&]() {
            nc_l = kernarg_copy<NlosConst>(offsetof(GradNlosArgs, nlos));
            film_l = kernarg_copy<Film>(offsetof(GradNlosArgs, g) + offsetof(GradArgs, film));
            rc_l = kernarg_copy<RenderConst>(offsetof(GradNlosArgs, g) + offsetof(GradArgs, rc));
        };
        if constexpr (TEX == kTexSlab) grad_nlos_lane<true>(sv, nc_l, film_l, rc_l, a.gc, pixel, s, st, acc, reload, TexelSlab{ s_slab + n_me });
        else grad_nlos_lane<true>(sv, nc_l, film_l, rc_l, a.gc, pixel, s, st, acc, reload, TexelGlobal{ a.tex_acc });
    }
    __syncthreads();
    double *row = a.partial + (size_t)blockIdx.x * slab_n;
    for (uint32_t i = tid; i < slab_n; i += kBlock) row[i] = s_slab[i];
}

} // namespace

hipError_t launch_grad_paths_nlos_tex(const GradArgs &a, const NlosConst &nlos_unit, uint32_t tier, int grid, size_t lds, hipStream_t stream)
{
    if (tier != MTR_GRAD_TEX_SLAB && tier != MTR_GRAD_TEX_GLOBAL) return hipErrorInvalidValue;
    GradNlosArgs n{};
    n.g = a; n.nlos = nlos_unit;
    return tier == MTR_GRAD_TEX_SLAB ? launch_with_lds(k_grad_paths_nlos_tex<kTexSlab>, n, grid, lds, stream)
                                     : launch_with_lds(k_grad_paths_nlos_tex<kTexGlobal>, n, grid, lds, stream);
}

} // namespace mtr
