// host_backproject.cpp — TEST-ONLY.  Compiles the product's backprojection arithmetic (mtr_backproject.h: bp_check, bp_args,
// bp_voxel, bp_plan) for the HOST, one voxel after another, for tests/test_backproject.py and tests/test_gpu_backproject.py.
// Never part of libmitransient_amd.so.  Every pointer of the description is a host pointer here.
#include "../mitransient_amd/csrc/mtr_backproject.h"

using namespace mtr;

namespace {
template <uint32_t CAPTURE, bool LINEAR>
void run(const BpArgs &a, float *volume)
{
    for (uint32_t iz = 0; iz < a.nz; ++iz)
        for (uint32_t iy = 0; iy < a.ny; ++iy)
            for (uint32_t ix = 0; ix < a.nx; ++ix)
                volume[((size_t)iz * a.ny + iy) * a.nx + ix] = bp_voxel<CAPTURE, LINEAR>(a, ix, iy, iz, 0u, a.n_pairs);
}
template <uint32_t CAPTURE>
void run(const BpArgs &a, float *volume) { if (a.linear) run<CAPTURE, true>(a, volume); else run<CAPTURE, false>(a, volume); }
}

extern "C" {

// mtr_backproject on the host: 0, or -1 (MTR_ERR_INVALID) with the volume untouched
int hb_backproject(const mtr_backproject_desc *d, const float *capture, float *volume)
{
    if (bp_check(d, capture, volume)) return -1;
    const BpArgs a = bp_args(*d, capture);
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) run<MTR_CAPTURE_CONFOCAL>(a, volume);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) run<MTR_CAPTURE_SINGLE>(a, volume);
    else run<MTR_CAPTURE_EXHAUSTIVE>(a, volume);
    return 0;
}

const char *hb_check(const mtr_backproject_desc *d, const float *capture, const float *volume)
{
    const char *why = bp_check(d, capture, volume);
    return why ? why : "";
}

// bp_plan: out = { n_tiles, n_slabs, slab_len }
int hb_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, int n_cu, uint64_t *out)
{
    BpPlan pl;
    if (!bp_plan(nx, ny, nz, n_pairs, n_cu, pl)) return 0;
    out[0] = pl.n_tiles; out[1] = pl.n_slabs; out[2] = pl.slab_len;
    return 1;
}

}
