// TEST-ONLY host build of SHADOW HULL (mitransient_amd/csrc/mtr_shadow_hull.h; mtr_core.h flat_walk_device): the claim that a shadow
// ray built by shade_hit towards the one rectangular emitter E cannot be told a hit by a hull rectangle when its origin is hull-safe,
// nor by E when it is E-safe — checked on the host builds of the very functions the kernel runs: offset_point, rect_emitter_point,
// shadow_ray_to, trav_quad_test, hull_side, and the classification of shadow_hull_classify / classify_scene.
// Built by tests/test_shadow_hull.py as a shared library (hsh_classify: classify_scene on a real scene description; hsh_sweep) and, with
// -DHSH_MAIN, as a stand-alone program that classifies its own rooms and sweeps them (the form a sanitizer build runs).
#include "../mitransient_amd/csrc/mtr_core.h"
#include "../mitransient_amd/csrc/mtr_scene_host.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mtr;

namespace {

struct NullStack { void count(int) {} };

struct Rect { f3 c, du, dv; };
struct Face { Rect r; f3 n; };            // a surface a path vertex can lie on, with its geometric normal

struct Room {
    std::vector<Rect> quads;              // the root's rectangles in child order
    uint32_t e_child = 0;
    f3 en{};                              // E's normal (the side it shines on)
    std::vector<Face> box_faces;
    std::vector<float> verts;             // every vertex: rectangles' corners, boxes' corners
    f3 centre{};
};

f3 rect_point(const Rect &r, float u, float v) { return mk(fmaf(r.du.x, u, fmaf(r.dv.x, v, r.c.x)), fmaf(r.du.y, u, fmaf(r.dv.y, v, r.c.y)), fmaf(r.du.z, u, fmaf(r.dv.z, v, r.c.z))); }
f3 unit(f3 v) { const float l = sqrtf(dot(v, v)); return mk(v.x / l, v.y / l, v.z / l); }

void add_rect_verts(Room &R, const Rect &r)
{
    for (int i = 0; i < 4; ++i) { const f3 p = rect_point(r, (i & 1) ? 1.0f : -1.0f, (i & 2) ? 1.0f : -1.0f); R.verts.push_back(p.x); R.verts.push_back(p.y); R.verts.push_back(p.z); }
}
// a cube [-1, 1]^3 scaled by (sx, sy, sz), turned by `deg` about y, moved to `at`
void add_cube(Room &R, f3 at, float deg, f3 s)
{
    const float a = deg * 0.017453292519943295f, ca = cosf(a), sa = sinf(a);
    const f3 ax[3] = { mk(ca * s.x, 0.0f, -sa * s.x), mk(0.0f, s.y, 0.0f), mk(sa * s.z, 0.0f, ca * s.z) };
    for (int f = 0; f < 6; ++f) {
        const int k = f >> 1; const float sg = (f & 1) ? 1.0f : -1.0f;
        Face F; F.r.c = mk(at.x + sg * ax[k].x, at.y + sg * ax[k].y, at.z + sg * ax[k].z); F.r.du = ax[(k + 1) % 3]; F.r.dv = ax[(k + 2) % 3];
        F.n = unit(mk(sg * ax[k].x, sg * ax[k].y, sg * ax[k].z));
        R.box_faces.push_back(F);
        add_rect_verts(R, F.r);
    }
}

// the Cornell box of mitransient_amd.cornell_box(), times `scale`.  variant: 0 as it is; 1 the light on the red wall; 2 the light in the
// ceiling's plane; 3 the light touching the green wall; 4 a free-standing partition; 5 a cube poking through the floor; 6 seven walls (a gabled front); 7 the room turned about an oblique axis
Room make_room(float scale, int variant)
{
    Room R;
    const float S = scale;
    auto quad = [&](f3 c, f3 du, f3 dv) { Rect r{ mk(c.x * S, c.y * S, c.z * S), mk(du.x * S, du.y * S, du.z * S), mk(dv.x * S, dv.y * S, dv.z * S) }; R.quads.push_back(r); add_rect_verts(R, r); };
    // light: translate(0, .99, .01) rotate(x, 90) scale(.23, .19, .19): du = (.23, 0, 0), dv = (0, 0, .19), normal (0, -1, 0)
    if (variant == 1) { quad(mk(-0.99f, 0.1f, 0.05f), mk(0.0f, 0.0f, 0.23f), mk(0.0f, 0.19f, 0.0f)); R.en = mk(1.0f, 0.0f, 0.0f); }
    else if (variant == 2) { quad(mk(0.0f, 1.0f, 0.01f), mk(0.23f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.19f)); R.en = mk(0.0f, -1.0f, 0.0f); }
    else if (variant == 3) { quad(mk(0.77f, 0.99f, 0.01f), mk(0.23f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.19f)); R.en = mk(0.0f, -1.0f, 0.0f); }
    else { quad(mk(0.0f, 0.99f, 0.01f), mk(0.23f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.19f)); R.en = mk(0.0f, -1.0f, 0.0f); }
    R.e_child = 0;
    quad(mk(0, -1, 0), mk(1, 0, 0), mk(0, 0, -1));      // floor
    quad(mk(0, 1, 0), mk(1, 0, 0), mk(0, 0, 1));        // ceiling
    quad(mk(0, 0, -1), mk(1, 0, 0), mk(0, 1, 0));       // back
    quad(mk(1, 0, 0), mk(0, 0, 1), mk(0, 1, 0));        // green wall
    quad(mk(-1, 0, 0), mk(0, 0, -1), mk(0, 1, 0));      // red wall
    if (variant == 6) {                                 // two panels in front of the open side, meeting in a ridge at z = 1.75: each has the other on its inner side
        quad(mk(0, 0.5f, 1.5f), mk(-1, 0, 0), mk(0, 0.5f, -0.25f));
        quad(mk(0, -0.5f, 1.5f), mk(-1, 0, 0), mk(0, 0.5f, 0.25f));
    }
    if (variant == 4) quad(mk(0.3f, -0.5f, 0.0f), mk(0.0f, 0.0f, 0.4f), mk(0.0f, 0.5f, 0.0f));
    add_cube(R, mk(0.335f * S, -0.7f * S, 0.38f * S), -17.0f, mk(0.3f * S, 0.3f * S, 0.3f * S));
    add_cube(R, mk(-0.33f * S, (variant == 5 ? -0.7f : -0.4f) * S, -0.28f * S), 18.25f, mk(0.3f * S, 0.61f * S, 0.3f * S));
    R.centre = mk(0.0f, 0.0f, 0.0f);
    if (variant == 7) {                                 // the whole room turned about an oblique axis and moved: no row with a zero in it, every rounding of the chains is live
        const double ax[3] = { 0.48, 0.6, 0.64 }, ang = 0.7, c = cos(ang), sn = sin(ang);
        double M[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[i][j] = (i == j ? c : 0.0) + (1.0 - c) * ax[i] * ax[j];
        M[0][1] -= sn * ax[2]; M[0][2] += sn * ax[1]; M[1][0] += sn * ax[2]; M[1][2] -= sn * ax[0]; M[2][0] -= sn * ax[1]; M[2][1] += sn * ax[0];
        auto turn = [&](f3 v) { return mk((float)(M[0][0] * v.x + M[0][1] * v.y + M[0][2] * v.z), (float)(M[1][0] * v.x + M[1][1] * v.y + M[1][2] * v.z), (float)(M[2][0] * v.x + M[2][1] * v.y + M[2][2] * v.z)); };
        const f3 shift = mk(0.37f * S, -0.21f * S, 0.55f * S);
        auto place = [&](Rect &r) { r.c = turn(r.c); r.c = mk(r.c.x + shift.x, r.c.y + shift.y, r.c.z + shift.z); r.du = turn(r.du); r.dv = turn(r.dv); };
        R.verts.clear();
        for (Rect &q : R.quads) { place(q); add_rect_verts(R, q); }
        for (Face &F : R.box_faces) { place(F.r); F.n = unit(turn(F.n)); add_rect_verts(R, F.r); }
        R.en = unit(turn(R.en)); R.centre = shift;
    }
    return R;
}

struct Built {
    Room room;
    std::vector<TriPair> recs, planes;    // the rectangles' records; the same with x and y rows zeroed (the plane alone: |lx|, |ly| <= 1 always)
    float rows[kWide][4];
    Emitter E{};
    ShadowHull hull{};
    bool on = false;
};

Built build(float scale, int variant)
{
    Built B; B.room = make_room(scale, variant);
    const Room &R = B.room;
    for (size_t k = 0; k < R.quads.size() && k < kWide; ++k) {
        const Rect &q = R.quads[k];
        const float c[3] = { q.c.x, q.c.y, q.c.z }, du[3] = { q.du.x, q.du.y, q.du.z }, dv[3] = { q.dv.x, q.dv.y, q.dv.z };
        float rx[4], ry[4], rz[4];
        rect_to_object(c, du, dv, rx, ry, rz);
        TriPair tp{};
        tp.g[0] = q4{ rz[0], rz[1], rz[2], rz[3] }; tp.g[1] = q4{ rx[0], rx[1], rx[2], rx[3] }; tp.g[2] = q4{ ry[0], ry[1], ry[2], ry[3] };
        tp.g[3] = q4{ 0, 0, 0, 0 }; tp.g[4] = q4{ 0, 0, bitsf((uint32_t)k), 0 };
        B.recs.push_back(tp);
        tp.g[1] = tp.g[2] = q4{ 0, 0, 0, 0 };
        B.planes.push_back(tp);
        for (int a = 0; a < 4; ++a) B.rows[k][a] = rz[a];
    }
    const Rect &e = R.quads[R.e_child];
    B.E.kind = kEmRect;
    B.E.center[0] = e.c.x; B.E.center[1] = e.c.y; B.E.center[2] = e.c.z;
    B.E.du[0] = e.du.x; B.E.du[1] = e.du.y; B.E.du[2] = e.du.z; B.E.dv[0] = e.dv.x; B.E.dv[1] = e.dv.y; B.E.dv[2] = e.dv.z;
    B.E.n[0] = R.en.x; B.E.n[1] = R.en.y; B.E.n[2] = R.en.z;
    HullInput in{};
    in.n_quads = (uint32_t)R.quads.size(); in.rows = B.rows; in.e_child = R.e_child;
    for (int a = 0; a < 3; ++a) { in.ec[a] = B.E.center[a]; in.edu[a] = B.E.du[a]; in.edv[a] = B.E.dv[a]; in.en[a] = B.E.n[a]; }
    in.verts = R.verts.data(); in.n_verts = R.verts.size() / 3;
    B.on = R.quads.size() <= kWide && shadow_hull_classify(in, B.hull);
    return B;
}

struct TestRng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; uint32_t x = (uint32_t)(((s >> 18u) ^ s) >> 27u); const uint32_t r = (uint32_t)(s >> 59u); return (x >> r) | (x << ((32u - r) & 31u)); }
    float u01() { return (float)(next() >> 8) * 5.9604644775390625e-8f; }        // [0, 1)
    float s11() { return fmaf(u01(), 2.0f, -1.0f); }
    uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)next() * n) >> 32); }
};

float step_towards(float x, float target, uint32_t ulps) { for (uint32_t i = 0; i < ulps; ++i) x = nextafterf(x, target); return x; }
f3 rect_normal(const Rect &r) { return unit(cross(r.du, r.dv)); }

} // namespace

extern "C" {

struct hsh_stats {
    uint64_t pairs, violations_hull, violations_e;
    uint64_t uniform_wall, uniform_wall_hull_safe, uniform_wall_e_safe;      // uniform origins on the walls that cast a shadow ray (shade_hit: the emitter faces them)
    uint64_t adversarial, adversarial_hull_risky, adversarial_e_risky;
    uint64_t hull_plane_hits, e_hits;                  // hits the tests DID report (for risky lanes): the sweep is not vacuous
    uint64_t wall_origins_safe_at_128;                 // uniform wall origins that are NOT hull-risky with every delta times 128
    float e_delta, hull_delta_max;
    uint32_t count, on;
};

// classify_scene on a scene description (what the library's mtr_scene_create computes and mtr_scene_shadow_hull reports)
int hsh_classify(const mtr_scene_desc *d, ShadowHull *out)
{
    HostScene hs;
    if (derive_scene(*d, hs) != nullptr) return 1;
    *out = hs.hull;
    return 0;
}

// (origin, endpoint) pairs over the room (scale, variant), every one asserted; returns 0 when no claim was violated
int hsh_sweep(float scale, int variant, uint64_t n_pairs, uint64_t seed, hsh_stats *o)
{
    *o = hsh_stats{};
    const Built B = build(scale, variant);
    o->on = B.on ? 1u : 0u; o->count = B.hull.count; o->e_delta = B.hull.e_delta;
    for (uint32_t k = 0; k < kHullRows; ++k) o->hull_delta_max = fmaxf(o->hull_delta_max, B.hull.delta[k]);
    if (!B.on) return 2;
    const Room &R = B.room;
    const ShadowHull h128 = shadow_hull_with_margin(B.hull, 128.0f);
    const uint32_t nq = (uint32_t)R.quads.size(), e = R.e_child;
    const f3 en = R.en;
    TestRng rng{ seed * 2u + 1u };
    NullStack st; SceneView sc{};
    for (uint64_t i = 0; i < n_pairs; ++i) {
        // ---- the surface point sp and its geometric normal
        f3 sp, gn; bool uniform_wall = false, adversarial = false;
        const uint32_t kind = rng.below(10);
        if (kind < 4u) {                      // uniform on a wall
            uint32_t k = rng.below(nq - 1u); if (k >= e) ++k;
            sp = rect_point(R.quads[k], rng.s11(), rng.s11()); gn = rect_normal(R.quads[k]); uniform_wall = true;
        } else if (kind < 6u) {               // uniform on a box face or on E
            if (rng.below(8) == 0u) { sp = rect_point(R.quads[e], rng.s11(), rng.s11()); gn = en; }
            else { const Face &F = R.box_faces[rng.below((uint32_t)R.box_faces.size())]; sp = rect_point(F.r, rng.s11(), rng.s11()); gn = F.n; }
        } else {
            adversarial = true;
            const uint32_t ulps = rng.below(65);
            if (kind < 8u) {                  // 0 .. 64 ulps from a wall's edge or corner (where it meets its neighbours), or from E's
                const uint32_t k = rng.below(4) == 0u ? e : [&] { uint32_t w = rng.below(nq - 1u); return w >= e ? w + 1u : w; }();
                const uint32_t which = rng.below(3);
                const float u = which != 1u ? (rng.below(2) ? 1.0f : -1.0f) : rng.s11(), v = which != 0u ? (rng.below(2) ? 1.0f : -1.0f) : rng.s11();
                sp = rect_point(R.quads[k], u, v); gn = k == e ? en : rect_normal(R.quads[k]);
                const f3 to = k == e ? R.quads[e].c : R.centre;
                if (rng.below(2)) sp = mk(step_towards(sp.x, to.x, ulps), step_towards(sp.y, to.y, ulps), step_towards(sp.z, to.z, ulps));
                else {                        // ... along the edge's own normal direction in the wall alone
                    const f3 dir = which == 1u ? R.quads[k].dv : R.quads[k].du;
                    const float ax = fabsf(dir.x), ay = fabsf(dir.y), az = fabsf(dir.z);
                    if (ax >= ay && ax >= az) sp.x = step_towards(sp.x, to.x, ulps); else if (ay >= az) sp.y = step_towards(sp.y, to.y, ulps); else sp.z = step_towards(sp.z, to.z, ulps);
                }
            } else {                          // the strip of a wall around E's plane, both sides: +-3 delta_E, and 64 and 4096 times narrower (where E's test does report hits)
                uint32_t k = rng.below(nq - 1u); if (k >= e) ++k;
                const Rect &w = R.quads[k];
                sp = rect_point(w, rng.s11(), rng.s11()); gn = rect_normal(w);
                if (fabsf(dot(gn, en)) < 0.1f) {
                    const float he = hull_side(B.hull.e_row, sp.x, sp.y, sp.z), tau = rng.s11() * 3.0f * B.hull.e_delta * (kind == 8u ? 1.0f : (ulps & 1u) ? 0.015625f : 0.000244140625f);
                    const f3 q = mk(fmaf(en.x, tau - he, sp.x), fmaf(en.y, tau - he, sp.y), fmaf(en.z, tau - he, sp.z));
                    const q4 X = B.recs[k].g[1], Y = B.recs[k].g[2];
                    const float lx = fmaf(X.z, q.z, fmaf(X.y, q.y, fmaf(X.x, q.x, X.w))), ly = fmaf(Y.z, q.z, fmaf(Y.y, q.y, fmaf(Y.x, q.x, Y.w)));
                    if (fabsf(lx) <= 1.0f && fabsf(ly) <= 1.0f) sp = q;
                }
            }
        }
        // ---- the point on E: uniform, or on its edges and corners
        float u1 = rng.u01(), u2 = rng.u01();
        if (rng.below(5) == 0u) {
            const float ends[2] = { 0.0f, 0.99999994f };
            const uint32_t which = rng.below(3);
            if (which != 1u) u1 = ends[rng.below(2)];
            if (which != 0u) u2 = ends[rng.below(2)];
        }
        const f3 ep = rect_emitter_point(B.E, u1, u2);
        const Ray ray = shadow_ray_to(sp, gn, ep);
        // (shade_hit casts the ray only when the emitter faces the point: dp < 0 on the normalised direction; a ceiling point behind E never does)
        const f3 dd0 = ep - sp;
        const bool casts = dot(dd0 / sqrtf(dot(dd0, dd0)), en) < 0.0f;
        // ---- the guards, as flat_walk_device evaluates them
        bool risky_h = false, risky_h128 = false;
        for (uint32_t k = 0; k < kHullRows; ++k) {
            const float g = hull_side(B.hull.row[k], ray.o.x, ray.o.y, ray.o.z);
            risky_h |= !(g >= B.hull.delta[k]); risky_h128 |= !(g >= h128.delta[k]);
        }
        const bool risky_e = !(hull_side(B.hull.e_row, ray.o.x, ray.o.y, ray.o.z) >= B.hull.e_delta);
        // ---- what the rectangle tests say
        const RayByValue rv{ ray.o, ray.d, ray.tmax };
        bool hull_hit = false, e_hit = false;
        for (uint32_t k = 0; k < nq; ++k)
            for (int form = 0; form < 2; ++form) {
                Trav tr; tr.h.t = kInf; tr.h.u = 0.0f; tr.h.v = 0.0f; tr.h.prim = -1; tr.best_orig = 0xffffffffu;
                RecByValue rec; rec.tp = form ? B.planes[k] : B.recs[k]; rec.first = k;
                const bool hit = trav_quad_test(tr, sc, st, true, rv, rec);
                if (k == e) e_hit |= hit; else hull_hit |= hit;
            }
        ++o->pairs;
        if (!risky_h && hull_hit) ++o->violations_hull;
        if (!risky_e && e_hit) ++o->violations_e;
        if (hull_hit) ++o->hull_plane_hits;
        if (e_hit) ++o->e_hits;
        if (uniform_wall && casts) { ++o->uniform_wall; o->uniform_wall_hull_safe += risky_h ? 0u : 1u; o->uniform_wall_e_safe += risky_e ? 0u : 1u; o->wall_origins_safe_at_128 += risky_h128 ? 0u : 1u; }
        if (adversarial) { ++o->adversarial; o->adversarial_hull_risky += risky_h ? 1u : 0u; o->adversarial_e_risky += risky_e ? 1u : 0u; }
    }
    return (o->violations_hull || o->violations_e) ? 1 : 0;
}

// the rooms of make_room classified through shadow_hull_classify: (on, hull rectangles)
int hsh_room_class(float scale, int variant, uint32_t *count)
{
    const Built B = build(scale, variant);
    *count = B.hull.count;
    return B.on ? 1 : 0;
}

} // extern "C"

#ifdef HSH_MAIN
int main(int argc, char **argv)
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    int bad = 0;
    // classification: the Cornell box and its scaled copies are on with five hull rectangles, the light on a side wall too, seven walls
    // with seven; the light in the ceiling's plane, touching a wall, a partition in the room, a cube through the floor: off
    const struct { float scale; int variant; int on; uint32_t count; } cls[] = {
        { 1.0f, 0, 1, 5 }, { 100.0f, 0, 1, 5 }, { 0.01f, 0, 1, 5 }, { 1.0f, 1, 1, 5 }, { 1.0f, 6, 1, 7 }, { 1.0f, 7, 1, 5 }, { 100.0f, 7, 1, 5 },
        { 1.0f, 2, 0, 0 }, { 1.0f, 3, 0, 0 }, { 1.0f, 4, 0, 0 }, { 1.0f, 5, 0, 0 } };
    for (const auto &c : cls) {
        uint32_t count = 0;
        const int on = hsh_room_class(c.scale, c.variant, &count);
        if (on != c.on || count != c.count) { printf("classification of room (%g, %d): on %d count %u, expected %d %u\n", c.scale, c.variant, on, count, c.on, c.count); ++bad; }
    }
    const struct { float scale; int variant; uint64_t share; } runs[] = { { 1.0f, 0, 3 }, { 100.0f, 0, 1 }, { 0.01f, 0, 1 }, { 1.0f, 1, 1 }, { 1.0f, 6, 1 }, { 1.0f, 7, 2 }, { 100.0f, 7, 1 } };
    for (const auto &r : runs) {
        hsh_stats s;
        const int rc = hsh_sweep(r.scale, r.variant, n * r.share / 10u, 12345u + (uint64_t)r.variant, &s);
        printf("room (%g, %d): %llu pairs, violations hull %llu E %llu; uniform wall origins %llu: hull-safe %.6f E-safe %.6f; adversarial %llu: hull-risky %llu E-risky %llu; "
               "hits reported: walls' planes %llu E %llu; delta_E %.4g, largest delta %.4g; wall origins not hull-risky at margin 128: %llu\n",
               (double)r.scale, r.variant, (unsigned long long)s.pairs, (unsigned long long)s.violations_hull, (unsigned long long)s.violations_e,
               (unsigned long long)s.uniform_wall, (double)s.uniform_wall_hull_safe / (double)(s.uniform_wall ? s.uniform_wall : 1), (double)s.uniform_wall_e_safe / (double)(s.uniform_wall ? s.uniform_wall : 1),
               (unsigned long long)s.adversarial, (unsigned long long)s.adversarial_hull_risky, (unsigned long long)s.adversarial_e_risky,
               (unsigned long long)s.hull_plane_hits, (unsigned long long)s.e_hits, (double)s.e_delta, (double)s.hull_delta_max, (unsigned long long)s.wall_origins_safe_at_128);
        if (rc != 0) ++bad;
        if (s.uniform_wall && ((double)s.uniform_wall_hull_safe < 0.999 * (double)s.uniform_wall || (double)s.uniform_wall_e_safe < 0.98 * (double)s.uniform_wall)) ++bad;
        if (s.pairs >= 100000u && (!s.adversarial_hull_risky || !s.adversarial_e_risky)) ++bad;
        if (r.scale == 1.0f && r.variant == 0 && s.wall_origins_safe_at_128) ++bad;
    }
    printf("%s\n", bad ? "failed" : "ok");
    return bad ? 1 : 0;
}
#endif
