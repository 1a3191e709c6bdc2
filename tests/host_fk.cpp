// TEST-ONLY host build of mitransient_amd/csrc/mtr_fk.h: the three passes of f-k migration as plain loops over the functions the
// kernels of mtr_fk.hip call, compiled with the numerics contract's flags (tests/test_fk_migration.py: build_host_fk).
#include "../mitransient_amd/csrc/mtr_fk.h"

using namespace mtr;

extern "C" {

int hfk_desc_size(void) { return (int)sizeof(mtr_fk_desc); }

const char *hfk_check(const mtr_fk_desc *d, const void *src, const void *dst) { return fk_check(d, src, dst); }

void hfk_prepare(const mtr_fk_desc *d, const float *capture, const int32_t *shift, float *padded)
{
    const FkArgs a = fk_args(*d);
    const uint32_t rows = 2u * a.H * 2u * a.W, L = 2u * a.Tp;
    for (uint32_t r = 0; r < rows; ++r)
        for (uint32_t k = 0; k < L; ++k) padded[(size_t)r * L + k] = fk_prepare_at(a, capture, shift, r, k);
}

void hfk_stolt(const mtr_fk_desc *d, const float *spectrum, float *resampled)
{
    const FkArgs a = fk_args(*d);
    const size_t in_row = (size_t)a.Tp + 1u, out_row = 2u * (size_t)a.Tp;
    for (uint32_t iy = 0; iy < 2u * a.H; ++iy)
        for (uint32_t ix = 0; ix < 2u * a.W; ++ix) {
            const size_t row = (size_t)iy * (2u * a.W) + ix;
            const float *src = spectrum + row * in_row * 2u;
            float *dst = resampled + row * out_row * 2u;
            const float lateral = fk_lateral(a, iy, ix);
            for (uint32_t oz = 0; oz < out_row; ++oz) {
                uint32_t i0; float w, jac;
                float re = 0.0f, im = 0.0f;
                if (fk_tap(a.Tp, lateral, oz, i0, w, jac)) {
                    re = fk_mix(src[2u * i0], src[2u * i0 + 2u], w, jac);
                    im = fk_mix(src[2u * i0 + 1u], src[2u * i0 + 3u], w, jac);
                }
                dst[2u * oz] = re; dst[2u * oz + 1u] = im;
            }
        }
}

void hfk_finish(const mtr_fk_desc *d, const float *field, float *volume)
{
    const FkArgs a = fk_args(*d);
    const size_t depth = 2u * (size_t)a.Tp;
    for (uint32_t iz = 0; iz < a.nz; ++iz)
        for (uint32_t iy = 0; iy < a.H; ++iy)
            for (uint32_t ix = 0; ix < a.W; ++ix) {
                const float *g = field + (((size_t)iy * (2u * a.W) + ix) * depth + a.z0 + iz) * 2u;
                volume[((size_t)iz * a.H + iy) * a.W + ix] = fk_power(g[0], g[1]);
            }
}

} // extern "C"
