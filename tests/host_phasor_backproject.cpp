// host_phasor_backproject.cpp — TEST-ONLY.  Compiles the product's phasor-field arithmetic (mtr_phasor_backproject.h: pb_check,
// pb_args, pb_voxel) for the HOST, one voxel after another, for tests/test_phasor_backproject.py and
// tests/test_gpu_phasor_backproject.py.  Never part of libmitransient_amd.so.  Every pointer of the description is a host pointer.
#include "../mitransient_amd/csrc/mtr_phasor_backproject.h"

using namespace mtr;

namespace {
template <uint32_t CAPTURE, bool UNIFORM, bool WEIGHTED>
void run(const PbArgs &a, float *volume)
{
    for (uint32_t iz = 0; iz < a.nz; ++iz)
        for (uint32_t iy = 0; iy < a.ny; ++iy)
            for (uint32_t ix = 0; ix < a.nx; ++ix) {
                float *v = volume + (((size_t)iz * a.ny + iy) * a.nx + ix) * 2u;
                pb_voxel<CAPTURE, UNIFORM, WEIGHTED>(a, ix, iy, iz, 0u, a.n_pairs, v[0], v[1]);
            }
}
template <uint32_t CAPTURE>
void run(const PbArgs &a, float *volume)
{
    if (a.uniform) { if (a.weights) run<CAPTURE, true, true>(a, volume); else run<CAPTURE, true, false>(a, volume); }
    else { if (a.weights) run<CAPTURE, false, true>(a, volume); else run<CAPTURE, false, false>(a, volume); }
}
}

extern "C" {

// mtr_phasor_backproject on the host: 0, or -1 (MTR_ERR_INVALID) with the volume untouched
int hpb_backproject(const mtr_phasor_backproject_desc *d, const float *phasors, float *volume)
{
    if (pb_check(d, phasors, volume)) return -1;
    const PbArgs a = pb_args(*d, phasors);
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) run<MTR_CAPTURE_CONFOCAL>(a, volume);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) run<MTR_CAPTURE_SINGLE>(a, volume);
    else run<MTR_CAPTURE_EXHAUSTIVE>(a, volume);
    return 0;
}

const char *hb_check(const mtr_phasor_backproject_desc *d, const float *phasors, const float *volume)
{
    const char *why = pb_check(d, phasors, volume);
    return why ? why : "";
}

// phasor_term itself: (cos, sin) of the film's term
void hpb_phasor_term(float freq, float tau, float *cs) { phasor_term(freq, tau, cs[0], cs[1]); }

}
