// mtr_scene_host.h — host-side scene ingestion: mtr_scene_desc -> device-layout arrays
// (BVH2 node packets, leaf-ordered triangles with flat shading frames, emitters with derived
// normal / inverse area).  Pure C++, no HIP: the API layer uploads the result; the test host
// harness runs the same arrays through mtr_core.h on the CPU.
#pragma once
#include <vector>
#include "mtr_core.h"
#include "mtr_bvh.h"
#include "mtr_nlos.h"

namespace mtr {

struct HostScene {
    std::vector<Node> nodes;
    std::vector<WNode> wnodes;                 // 8-wide collapse of `nodes` (small scenes only: walked in LDS)
    std::vector<QNode8> wnodes8q;              // quantised 8-wide collapse (large scenes only)
    std::vector<QNode4> wnodes4;               // quantised 4-wide collapse of `nodes` (walked in HBM by the wavefront kernels)
    bool has_wide = false;                     // wnodes is valid (possibly empty: a scene without triangles)
    std::vector<TriPair> tpairs;               // [n_slots / 2]
    std::vector<TriShade> tshade;              // [n_slots]
    std::vector<uint32_t> slot_orig;           // [n_slots] original triangle index (pad slots: the triangle they repeat)
    std::vector<mtr_material> mats;
    std::vector<Emitter> ems;
    std::vector<q4> samp_tris;                 // mesh emitters only (empty otherwise): see SceneView
    std::vector<q4> samp_vn;                   // ... their vertex normals (empty unless a mesh emitter has them): mesh_sample_position
    std::vector<q4> vnormals;                  // [3 * n_slots] vertex normals, when a triangle is smooth-shaded (empty otherwise)
    // bitmap textures (empty without): texels as RGBA f32 of all textures, (first texel, width, height, 0) per texture, and
    // the corner texture coordinates by slot, two quads each
    std::vector<q4> texels; std::vector<q4> tex_info; std::vector<q4> uvs;
    std::vector<float> face_pmf, face_cdf;
    uint32_t bvh_depth = 0, n_leaves = 0;
    uint32_t wide_levels = 0, wide4_levels = 0, wide8q_levels = 0;        // levels of the collapsed trees (= their traversal stack bound)
    Camera cam{};
    Film film{};
    // classify_scene's verdict on the tables above.  The host picks kernels by it, and a specialised kernel LACKS the code a trait rules out
    uint32_t traits = 0;                       // kTr* (mtr_core.h)
    bool needs_ext = false;                    // the extended shading code: a lobe, a smooth-shaded triangle, a bitmap (SceneDev::has_rough)
    bool polar_ok = false;                     // every material and emitter has a polarized form (mtr_polar.h)
    bool grey_scene = false;                   // kTrGrey without the NLOS laser (traits_with_laser decides with it)
    bool has_sphere = false;                   // an analytic sphere among the shapes: none of the traits tr_spheres (mtr_core.h) names
    FlatTop flat{};                            // traits & kTrFlatTop: the top level as scalar kernel arguments
    ShadowHull hull{};                         // SHADOW HULL (mtr_shadow_hull.h): which rectangles a shadow ray is spared; count 0: none
};

inline bool bsdf_is_lobe(uint32_t type) { return bsdf_is_rough(type) || type == MTR_BSDF_THINDIELECTRIC; }     // what only the extended shading code evaluates
// the colour-dependent trait (kTrGrey, the scene's part): three equal channels in every colour, no bitmap
bool colours_are_grey(const mtr_material *mats, uint32_t n_mats, const Emitter *ems, uint32_t n_ems, bool textured);
// ... as the scene's own part of kTrGrey: a scene with an analytic sphere never has it, whatever its colours (mtr_core.h tr_spheres: the
// one-plane NLOS kernels hold no sphere code) — a grey NLOS scene with a hidden ball renders with three-plane rows.  The one place that
// rule lives: classify_scene and the colour updates of the API layer all decide through it
inline bool scene_is_grey(bool has_sphere, const mtr_material *mats, uint32_t n_mats, const Emitter *ems, uint32_t n_ems, bool textured)
{
    return !has_sphere && colours_are_grey(mats, n_mats, ems, n_ems, textured);
}
// world -> object rows of an analytic rectangle (centre c, half-edges du, dv): x and y along the edges, z the unit normal — the
// rows of its intersection record (TriPair::g[1], g[2], g[0])
void rect_to_object(const float c[3], const float du[3], const float dv[3], float rx[4], float ry[4], float rz[4]);
// fills traits, needs_ext, polar_ok, grey_scene and flat from the tables (derive_scene ends with it)
void classify_scene(const mtr_scene_desc &d, HostScene &s);
// ... its last step: fills hull from the traits, the flat top level and the emitter
void classify_shadow_hull(const mtr_scene_desc &d, HostScene &s);
// kTrGrey of the NLOS tier: the scene's colours and the laser's irradiance
uint32_t traits_with_laser(uint32_t traits, bool grey_scene, const float laser_irradiance[3]);

// the tint slots of mtr_scene_tint_layout (ABI 19): materials in table order, `specular_reflectance` of a conductor, roughconductor,
// dielectric, thindielectric or roughdielectric, then `specular_transmittance` of the three dielectric types.  slots (may be null):
// two words per material, the slot of its reflectance and of its transmittance or -1.  Returns the number of slots.
uint32_t tint_slot_table(const mtr_material *mats, uint32_t n_mats, int32_t *slots);

// NLOS tier tables (TransientNLOSPath.prepare, transientnlospath.py:251-292): shape / face distributions,
// rectangle normals, triangles in ORIGINAL order for Mesh::sample_position, projector constants
struct HostNlos {
    std::vector<NlosShape> shapes;
    std::vector<float> shape_pmf, shape_cdf, face_pmf, face_cdf;
    std::vector<q4> hg_tris;
    std::vector<q4> hg_vn;                     // vertex normals of hidden meshes that have them (empty otherwise): mesh_sample_position
    NlosConst k{};            // pointers left null: the caller points them at its copies
};
const char *derive_nlos(const mtr_scene_desc &d, HostNlos &out);

Film film_from_desc(const mtr_film_desc &d);
// returns nullptr on success or a static error string
const char *derive_scene(const mtr_scene_desc &d, HostScene &out);
RenderConst make_render_const(const mtr_render_params &p, const Film &f, uint32_t n_emitters);

} // namespace mtr
