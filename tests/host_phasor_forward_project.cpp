// host_phasor_forward_project.cpp — TEST-ONLY.  Compiles the product's phasor forward-projection arithmetic
// (mtr_phasor_forward_project.h: pf_check, pf_plan, pf_row, pf_voxel, pf_store) for the HOST, one (row, frequency block) after
// another with the voxels in ascending linear order, for tests/test_phasor_forward_project.py and
// tests/test_gpu_phasor_forward_project.py.  Never part of libmitransient_amd.so.  Every pointer of the description is a host pointer.
#include "../mitransient_amd/csrc/mtr_phasor_forward_project.h"

using namespace mtr;

namespace {
template <uint32_t CAPTURE, bool UNIFORM>
void run(const PbArgs &a, const float *volume, float *phasors)
{
    for (uint64_t p = 0; p < a.n_pairs; ++p) {
        const PfRow r = pf_row<CAPTURE>(a, p);
        for (uint32_t k0 = 0; k0 < a.F; k0 += kPbAnchor) {
            const uint32_t nk = a.F - k0 < kPbAnchor ? a.F - k0 : kPbAnchor;
            float fk[kPbAnchor], qr[kPbAnchor] = {}, qi[kPbAnchor] = {};
            for (uint32_t j = 0; j < kPbAnchor; ++j) fk[j] = a.frequencies[k0 + (j < nk ? j : nk - 1u)];
            const float *u = volume;
            for (uint32_t iz = 0; iz < a.nz; ++iz)
                for (uint32_t iy = 0; iy < a.ny; ++iy)
                    for (uint32_t ix = 0; ix < a.nx; ++ix, u += 2) {
                        const float vx = bp_centre(a.vmin[0], a.step[0], ix), vy = bp_centre(a.vmin[1], a.step[1], iy), vz = bp_centre(a.vmin[2], a.step[2], iz);
                        pf_voxel<CAPTURE, UNIFORM, false>(r, a.start_opl, a.freq_step, a.tau_min, a.tau_max, fk, nk, vx, vy, vz, u[0], u[1], qr, qi);
                    }
            for (uint32_t j = 0; j < nk; ++j) pf_store(phasors + ((size_t)p * a.F + k0 + j) * 2u, qr[j], qi[j], a.weights, k0 + j);
        }
    }
}
template <uint32_t CAPTURE>
void run(const PbArgs &a, const float *volume, float *phasors)
{
    if (a.uniform) run<CAPTURE, true>(a, volume, phasors); else run<CAPTURE, false>(a, volume, phasors);
}
}

extern "C" {

// mtr_phasor_forward_project on the host: 0, or -1 (MTR_ERR_INVALID) with the phasors untouched
int hpf_forward_project(const mtr_phasor_backproject_desc *d, const float *volume, float *phasors)
{
    if (pf_check(d, volume, phasors)) return -1;
    const PbArgs a = pb_args(*d, nullptr);
    PfPlan pl;
    if (!pf_plan(a.nx, a.ny, a.nz, a.n_pairs, a.F, 1, pl)) return -1;
    if (a.capture_type == MTR_CAPTURE_CONFOCAL) run<MTR_CAPTURE_CONFOCAL>(a, volume, phasors);
    else if (a.capture_type == MTR_CAPTURE_SINGLE) run<MTR_CAPTURE_SINGLE>(a, volume, phasors);
    else run<MTR_CAPTURE_EXHAUSTIVE>(a, volume, phasors);
    return 0;
}

const char *hpf_check(const mtr_phasor_backproject_desc *d, const float *volume, const float *phasors)
{
    const char *why = pf_check(d, volume, phasors);
    return why ? why : "";
}

// pf_plan; out = { n_blocks, n_slabs, slab_len (low word), slab_len (high word), kPbAnchor }; returns 0 when there is no plan
int hpf_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n_pairs, uint32_t F, int n_cu, uint32_t *out)
{
    PfPlan pl;
    if (!pf_plan(nx, ny, nz, n_pairs, F, n_cu, pl)) return 0;
    out[0] = pl.n_blocks; out[1] = pl.n_slabs; out[2] = (uint32_t)pl.slab_len; out[3] = (uint32_t)(pl.slab_len >> 32); out[4] = kPbAnchor;
    return 1;
}

}
