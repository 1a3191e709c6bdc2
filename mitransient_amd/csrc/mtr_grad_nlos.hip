// mtr_grad_nlos.hip — mtr_render_grad on the NLOS tier (ABI 17): k_grad_paths_nlos, the k_grad_paths of transient_nlos_path
// (mtr_grad.h: grad_nlos_lane over mtr_nlos.h's nlos_bounce; semantics in DESIGN.md §2).  A translation unit of its own: the kernels
// of mtr_grad.hip keep their instructions.  k_grad_reduce (mtr_grad.hip) sums the rows it stores.
// The kernel stages its scene itself, not through stage_scene (mtr_kernels.h): with the helper its instructions move
// (profiles/deriv_harness_asm_diff.txt), and no timing script reaches every form of the NLOS gradient kernels.
#include "mtr_grad_args.h"

namespace mtr {

namespace {

// k_grad_paths of the NLOS tier (its instantiations are named "nlos,lds,plain" / "nlos,lds,ext"): the scene staged in LDS as
// k_grad_paths<true, EXT> stages it, grad_nlos_lane per lane, the laser's words in the slab's emitter words.  Three workgroups per
// compute unit, as k_fused<NLOS>: the loop inlines four walks per bounce.
template <bool EXT>
__global__ void __launch_bounds__(kBlock, kGradNlosPerCu) k_grad_paths_nlos(const GradNlosArgs args)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const GradArgs &a = args.g;
    const int tid = threadIdx.x;
    const uint32_t slab_n = 3u * (a.n_mats + a.n_ems);
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
        grad_nlos_lane<EXT>(sv, nc_l, film_l, rc_l, a.gc, pixel, s, st, acc, reload);
    }
    __syncthreads();
    double *row = a.partial + (size_t)blockIdx.x * slab_n;
    for (uint32_t i = tid; i < slab_n; i += kBlock) row[i] = s_slab[i];
}

} // namespace

hipError_t launch_grad_paths_nlos(const GradArgs &a, const NlosConst &nlos_unit, bool ext, int grid, size_t lds, hipStream_t stream)
{
    GradNlosArgs n{};
    n.g = a; n.nlos = nlos_unit;
    return ext ? launch_with_lds(k_grad_paths_nlos<true>, n, grid, lds, stream) : launch_with_lds(k_grad_paths_nlos<false>, n, grid, lds, stream);
}

} // namespace mtr
