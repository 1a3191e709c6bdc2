// mtr_shadow_hull.h — SHADOW HULL: which top-level rectangles a shadow ray of k_fused's flat walk (mtr_core.h: flat_walk_device)
// need not be tested against, as a block of scalar kernel arguments (ShadowHull), the host arithmetic that fills it
// (shadow_hull_classify, called by classify_scene) and the per-lane guard the kernel evaluates (hull_side).  No HIP include:
// tests/host_shadow_hull.cpp compiles it for the host and sweeps the claim below over 10^7 shadow rays (tests/test_shadow_hull.py).
//
// THE CLAIM.  In a scene with ONE rectangular emitter E (kTrOneRectEmitter) every shadow ray is built by shade_hit as
//     ep on E,   so = offset_point(sp, gn, ep - sp),   sd = ep - so,   S = sqrtf(dot(sd, sd)),   d = sd / S,   tmax = S * (1 - kShadowEps)
// (mtr_core.h: rect_emitter_point, shadow_ray_to — the proof below uses exactly these three facts and the computed origin, nothing
// else of the path).  trav_quad_test decides a rectangle k from the first row Z of its record alone before it looks at the bounds:
//     oz = fma(Z.z, o.z, fma(Z.y, o.y, fma(Z.x, o.x, Z.w))),  dz likewise from d without Z.w,  t = -oz / dz,  a hit needs 0 <= t <= tmax.
// Write u = 2^-24, h(p) = Z . p + Z.w (exact), M = sum |Z_i| B_i + |Z.w| with B the largest |coordinate| a ray origin can have,
// and D = sum |Z_i| L_i with L the scene's extent per axis.  With s = +-1 folded into the row (fma is odd: the folded chain IS s oz):
//     s oz        = s h(so) + E0,                    |E0|  <= 3.01 u M                 (three fmas)
//     s dz S      = s h(ep) - s h(so) + E1,          |E1|  <= 6.1 u D                  (ep - so, 1 / S, * that, three fmas: one rounding each)
//     s h(ep)    >= s h(nearest corner of E) - 2.01 u M                               (ep's two fmas per coordinate)
// HULL RECTANGLE (a wall): s h(corner) >= m for the four corners of E.  A lane with s oz > 0 cannot be told a hit:
//     s dz >= 0:  t = -oz / dz is negative, -inf or +inf.
//     s dz <  0:  |dz| S = s oz - E0 - s h(ep) - E1 <= s oz as soon as m >= 3.01 u M + 6.1 u D + 2.01 u M, and then
//                 t >= (s oz / |dz|)(1 - u) >= S (1 - u) > S fl(1 - kShadowEps)(1 + u) >= tmax.
// The host asks for m >= kHullSafety (8 u M + 7 u D) and the kernel for s oz >= delta = 16 u M instead of > 0.
// E ITSELF: |h(ep)| <= hc + 2.01 u M with hc the largest |h(corner)|, so |dz| S <= s oz + Err, Err = 5.02 u M + 6.1 u D + hc, and
//     t > tmax  <=  s oz (1 - u) > (s oz + Err) fl(1 - eps)(1 + u)  <=  s oz > Err / (eps - 4 u):   delta_E = kHullSafetyE Err / (eps - 4 u),
// millimetres in the Cornell box.  s_E points to the side E shines on; origins behind E are simply not E-safe.
// The first condition on a hull rectangle — every vertex of the scene on the side of E — is not needed for any of this: it is what
// makes hull-safe lanes the rule (a partition inside the room would send every wave down the full stage).  It therefore allows what
// costs nothing: s h(v) >= -max(16 u M, D / kHullPoke).  The Cornell box's tall box stands 0.01 BELOW the floor (translate -0.4, scale
// 0.61), 1/200 of the room's height; nothing of it down there is ever a path vertex, and a rounding-sized allowance alone would
// switch the very scene this was written for off.  A box that reaches a sixty-fourth of the room's extent through a wall switches it off.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MTR_SH_HD __host__ __device__ inline
#else
#define MTR_SH_HD inline
#endif

namespace mtr {

constexpr uint32_t kHullRows = 8;          // (kWide - 1 hull rectangles at most; a multiple of four words keeps the block's loads wide)
// The block: FusedArgs::hull, read with scalar loads at the guard.  Unused rows are (0, 0, 0, 1) with delta 0: safe for every lane.
struct ShadowHull {
    uint32_t count, e_child;               // hull rectangles (0: the feature is off), E's child index under the root
    float e_delta, pad;
    float e_row[4];                        // s_E Z_E
    float delta[kHullRows];
    float row[kHullRows][4];               // s_k Z_k
};
static_assert(sizeof(ShadowHull) == 192, "dword-sized, no padding");

// the guard's arithmetic: trav_quad_test's chain for oz on a sign-folded row
MTR_SH_HD float hull_side(const float r[4], float ox, float oy, float oz) { return fmaf(r[2], oz, fmaf(r[1], oy, fmaf(r[0], ox, r[3]))); }

constexpr double kHullU = 5.9604644775390625e-8;          // 2^-24
constexpr double kHullSafety = 4.0, kHullSafetyE = 2.0, kHullPoke = 64.0;
constexpr double kHullShadowEps = 1500.0 * 5.9604644775390625e-8 * 10.0;      // mtr_core.h: kShadowEps (classify_scene asserts the two agree)
constexpr double kHullOffsetGrow = 1.001;                 // offset_point moves an origin by 8.9e-5 (1 + |p|): B = bound * this + 1e-3

// what classify_scene hands over: the first rows of the root's rectangles, E, and every vertex of the scene
struct HullInput {
    uint32_t n_quads;
    const float (*rows)[4];                // [n_quads] Z rows (TriPair::g[0]) in child order
    uint32_t e_child;
    float ec[3], edu[3], edv[3], en[3];    // E as shade_hit reads it: Emitter::center, du, dv, n
    const float *verts; size_t n_verts;    // xyz of every vertex of every top-level primitive and box (E's and the walls' corners included)
};

// Fills `out` (count 0: off).  Every root rectangle but E must be a hull rectangle, or the feature is off for the scene.
inline bool shadow_hull_classify(const HullInput &in, ShadowHull &out)
{
    out = ShadowHull{};
    for (uint32_t k = 0; k < kHullRows; ++k) out.row[k][3] = 1.0f;
    if (in.n_quads < 2u || in.n_quads > kHullRows || in.e_child >= in.n_quads || !in.n_verts) return false;
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    for (size_t v = 0; v < in.n_verts; ++v)
        for (int a = 0; a < 3; ++a) {
            const double x = in.verts[3 * v + a];
            if (!std::isfinite(x)) return false;
            lo[a] = fmin(lo[a], x); hi[a] = fmax(hi[a], x);
        }
    double corner[4][3], B[3], L[3];
    for (int c = 0; c < 4; ++c)
        for (int a = 0; a < 3; ++a) {
            corner[c][a] = (double)in.ec[a] + ((c & 1) ? 1.0 : -1.0) * (double)in.edu[a] + ((c & 2) ? 1.0 : -1.0) * (double)in.edv[a];
            lo[a] = fmin(lo[a], corner[c][a]); hi[a] = fmax(hi[a], corner[c][a]);
        }
    for (int a = 0; a < 3; ++a) { B[a] = fmax(fabs(lo[a]), fabs(hi[a])) * kHullOffsetGrow + 1e-3; L[a] = (hi[a] - lo[a]) * kHullOffsetGrow + 2e-3; }
    auto plane = [](const float *Z, const double *p) { return (double)Z[0] * p[0] + (double)Z[1] * p[1] + (double)Z[2] * p[2] + (double)Z[3]; };
    auto mag = [&](const float *Z) { return fabs((double)Z[0]) * B[0] + fabs((double)Z[1]) * B[1] + fabs((double)Z[2]) * B[2] + fabs((double)Z[3]); };
    auto ext = [&](const float *Z) { return fabs((double)Z[0]) * L[0] + fabs((double)Z[1]) * L[1] + fabs((double)Z[2]) * L[2]; };
    uint32_t n = 0;
    for (uint32_t k = 0; k < in.n_quads; ++k) {
        const float *Z = in.rows[k];
        const double M = mag(Z), D = ext(Z);
        if (!std::isfinite(M) || !(M > 0.0)) return false;
        if (k == in.e_child) {
            // the side E shines on, and how far E's own corners are from the plane its record describes
            const double front[3] = { (double)in.ec[0] + (double)in.en[0], (double)in.ec[1] + (double)in.en[1], (double)in.ec[2] + (double)in.en[2] };
            const double sf = plane(Z, front);
            if (!(fabs(sf) > 0.5)) return false;                 // (Z is a unit normal and E's centre lies on it: +-1)
            const float s = sf > 0.0 ? 1.0f : -1.0f;
            double hc = 0.0;
            for (int c = 0; c < 4; ++c) hc = fmax(hc, fabs(plane(Z, corner[c])));
            const double err = kHullU * (5.02 * M + 6.1 * D) + hc;
            const double de = kHullSafetyE * err / (kHullShadowEps - 4.0 * kHullU);
            if (!std::isfinite(de) || !(de < 3.0e38)) return false;
            for (int a = 0; a < 4; ++a) out.e_row[a] = s * Z[a];
            out.e_delta = (float)de * 1.000001f;
            out.e_child = k;
            continue;
        }
        double hmin = 1e300, hmax = -1e300;
        for (int c = 0; c < 4; ++c) { const double h = plane(Z, corner[c]); hmin = fmin(hmin, h); hmax = fmax(hmax, h); }
        const float s = hmin > 0.0 ? 1.0f : -1.0f;
        const double m = s > 0.0f ? hmin : -hmax;                // the nearest corner of E, on E's side
        if (!(m >= kHullSafety * kHullU * (8.0 * M + 7.0 * D))) return false;          // E touches or crosses this plane, or lies in it
        const double eta = 16.0 * kHullU * M, poke = fmax(eta, D / kHullPoke);
        for (size_t v = 0; v < in.n_verts; ++v) {
            const double p[3] = { in.verts[3 * v], in.verts[3 * v + 1], in.verts[3 * v + 2] };
            if (!((double)s * plane(Z, p) >= -poke)) return false;                     // something of the scene lies behind this rectangle's plane
        }
        for (int a = 0; a < 4; ++a) out.row[n][a] = s * Z[a];
        out.delta[n] = (float)eta * 1.000001f;
        ++n;
    }
    out.count = n;
    return n != 0u;
}

// amd_shadow_hull_margin: every delta times `margin` (>= 1: only more careful; 0: off)
inline ShadowHull shadow_hull_with_margin(const ShadowHull &h, float margin)
{
    ShadowHull o = h;
    if (!(margin >= 1.0f) || !h.count) { o.count = 0u; return o; }
    for (uint32_t k = 0; k < kHullRows; ++k) o.delta[k] = h.delta[k] * margin;
    o.e_delta = h.e_delta * margin;
    return o;
}

} // namespace mtr
