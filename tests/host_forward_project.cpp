// host_forward_project.cpp — TEST-ONLY.  Compiles the product's forward-projection arithmetic (mtr_forward_project.h: fp_row,
// fp_taps, fp_plan over mtr_backproject.h) for the HOST, for tests/test_forward_project.py and tests/test_gpu_forward_project.py:
// every cell is the f32 sum of its voxels in ascending linear order.  Never part of libmitransient_amd.so.  Every pointer of the
// description is a host pointer here.
#include "../mitransient_amd/csrc/mtr_forward_project.h"

using namespace mtr;

namespace {
template <uint32_t CAPTURE, bool LINEAR>
void run(const BpArgs &a, const float *volume, float *capture)
{
    for (size_t i = 0; i < (size_t)a.n_pairs * a.T; ++i) capture[i] = 0.0f;
    for (uint32_t iz = 0; iz < a.nz; ++iz)
        for (uint32_t iy = 0; iy < a.ny; ++iy)
            for (uint32_t ix = 0; ix < a.nx; ++ix) {
                const float x = volume[((size_t)iz * a.ny + iy) * a.nx + ix];
                const float vx = bp_centre(a.vmin[0], a.step[0], ix), vy = bp_centre(a.vmin[1], a.step[1], iy), vz = bp_centre(a.vmin[2], a.step[2], iz);
                for (uint64_t p = 0; p < a.n_pairs; ++p) {
                    float *row = capture + (size_t)p * a.T;
                    fp_taps<CAPTURE, LINEAR>(a, fp_row<CAPTURE>(a, p), vx, vy, vz, x, [&](uint32_t b, float val) { row[b] += val; });
                }
            }
}
template <uint32_t CAPTURE>
void run(const BpArgs &a, const float *volume, float *capture) { if (a.linear) run<CAPTURE, true>(a, volume, capture); else run<CAPTURE, false>(a, volume, capture); }
}

extern "C" {

// mtr_forward_project on the host: 0, or -1 (MTR_ERR_INVALID) with the capture untouched
int hf_forward_project(const mtr_backproject_desc *d, const float *volume, float *capture)
{
    if (bp_check(d, capture, volume)) return -1;
    const BpArgs a = bp_args(*d, nullptr);
    FpPlan pl;
    if (!fp_plan(a.nx, a.ny, a.nz, a.n_pairs, a.T, 256, pl)) return -1;
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) run<MTR_CAPTURE_CONFOCAL>(a, volume, capture);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) run<MTR_CAPTURE_SINGLE>(a, volume, capture);
    else run<MTR_CAPTURE_EXHAUSTIVE>(a, volume, capture);
    return 0;
}

// fp_plan: out = { n_windows, n_slabs, slab_len, kFpWindow, kFpPartialCap }
int hf_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, uint32_t T, int n_cu, uint64_t *out)
{
    FpPlan pl;
    if (!fp_plan(nx, ny, nz, n_pairs, T, n_cu, pl)) return 0;
    out[0] = pl.n_windows; out[1] = pl.n_slabs; out[2] = pl.slab_len; out[3] = kFpWindow; out[4] = kFpPartialCap;
    return 1;
}

}
