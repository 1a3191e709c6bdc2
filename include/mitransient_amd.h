/*
 * mitransient_amd.h — C-ABI of the MI355X-native transient path tracer.
 *
 * This is the drop-in boundary for ONE path of diegoroyo/mitransient: the
 * `transient_path` integrator + `transient_hdr_film` time-binning
 * (reference: mitransient/integrators/common.py:122-213,
 *  mitransient/integrators/transientpath.py:88-326,
 *  mitransient/films/transient_hdr_film.py:210-276,
 *  mitransient/render/transient_image_block.py:56-151).
 *
 * The reference has no FFI of its own: its Python plugins call into Mitsuba 3
 * (C++) / Dr.Jit through pybind11 objects.  The entry points below are what a
 * ctypes binding placed at those Python call sites would bind (see
 * INTEGRATION.md for the stub); each one cites the reference interface it
 * replaces.
 *
 * Conventions: opaque handles; plain pointers and sizes; no C++/torch types;
 * every function returns 0 on success or a negative mtr_status; the message of
 * the last failure on a context is available through mtr_last_error().
 * Pointers documented "device" must be HIP device pointers on the context's
 * GPU; all launches go to the hipStream_t handed to mtr_ctx_set_stream()
 * (default: the NULL stream).  A context is not re-entrant; use one per
 * thread/stream.
 */
#ifndef MITRANSIENT_AMD_H
#define MITRANSIENT_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_ABI_VERSION 24

typedef enum mtr_status {
    MTR_OK = 0,
    MTR_ERR_INVALID = -1,     /* bad argument / unsupported property            */
    MTR_ERR_NO_DEVICE = -2,   /* no HIP device: there is NO CPU fallback        */
    MTR_ERR_HIP = -3,         /* a HIP runtime call failed                      */
    MTR_ERR_OOM = -4,
    MTR_ERR_UNSUPPORTED = -5
} mtr_status;

/* ---- materials: BSDF subset of the north-star path --------------------- */
enum { MTR_BSDF_DIFFUSE = 0, MTR_BSDF_CONDUCTOR = 1, MTR_BSDF_DIELECTRIC = 2,
       MTR_BSDF_NULL = 3 /* no BSDF: absorbs */,
       MTR_BSDF_ROUGHCONDUCTOR = 4, /* microfacet conductor, isotropic alpha, visible-normal sampling (mitsuba `roughconductor`,
                                       distribution = ggx | beckmann (MTR_MAT_BECKMANN), sample_visible = true): a smooth lobe,
                                       takes part in emitter sampling */
       MTR_BSDF_ROUGHPLASTIC = 5,   /* microfacet dielectric coat over a diffuse base (mitsuba `roughplastic`) */
       MTR_BSDF_ROUGHDIELECTRIC = 6, /* rough refractive interface (mitsuba `roughdielectric`, ABI 11): int_ior / ext_ior, c = specular
                                       reflectance, c2 = specular transmittance, alpha (MTR_MAT_ANISOTROPIC: alpha_v in b[0]);
                                       transmissive, never under MTR_MAT_TWOSIDED */
       MTR_BSDF_THINDIELECTRIC = 7, /* thin dielectric slab (mitsuba `thindielectric`, ABI 11): two delta lobes, no refraction, eta stays 1;
                                       int_ior / ext_ior, c / c2 = specular reflectance / transmittance */
       MTR_BSDF_PLASTIC = 8         /* smooth dielectric coat over a diffuse base (mitsuba `plastic`, ABI 11): a = diffuse_reflectance,
                                       c = specular_reflectance, int_ior / ext_ior, MTR_MAT_NONLINEAR, internal_reflectance =
                                       fresnel_diffuse_reflectance(1 / eta), specular_sampling_weight                              */ };
enum { MTR_MAT_TWOSIDED = 1u,
       MTR_MAT_NONLINEAR = 2u, /* roughplastic `nonlinear`: diffuse / (1 - diffuse * internal_reflectance) per channel */
       MTR_MAT_BECKMANN = 4u,  /* rough lobes (ABI 11): the Beckmann distribution — mitsuba's default `distribution` — instead of GGX */
       MTR_MAT_ANISOTROPIC = 8u /* roughconductor (ABI 11): `alpha` is alpha_u (along the shading frame's tangent, dp/du) and c2[0]
                                   holds alpha_v (a field conductors do not use otherwise)                                    */ };
#define MTR_ROUGH_TRANSMITTANCE_RES 64

typedef struct mtr_material {
    uint32_t type;        /* MTR_BSDF_*                                          */
    uint32_t flags;       /* MTR_MAT_*                                           */
    float    a[3];        /* diffuse: reflectance rgb | (rough)conductor: eta rgb | roughplastic: diffuse_reflectance rgb */
    float    b[3];        /* (rough)conductor: k rgb | roughdielectric with MTR_MAT_ANISOTROPIC: b[0] = alpha_v */
    float    c[3];        /* conductor/dielectric/rough*: specular_reflectance rgb */
    float    int_ior;     /* dielectric, roughplastic                            */
    float    ext_ior;     /* dielectric, roughplastic                            */
    float    c2[3];       /* dielectric: specular_transmittance rgb | roughconductor with MTR_MAT_ANISOTROPIC: c2[0] = alpha_v */
    /* rough lobes (ABI 8) */
    float    alpha;       /* roughness of the lobe (alpha_u = alpha_v unless MTR_MAT_ANISOTROPIC) */
    float    internal_reflectance;   /* roughplastic: mean rough reflectance of the coat seen from inside          */
    float    specular_sampling_weight; /* roughplastic: s_mean / (d_mean + s_mean)                                 */
    uint32_t albedo_texture;  /* 1 + index into mtr_scene_desc.textures of a bitmap that replaces `a` (diffuse reflectance,
                                 roughplastic diffuse_reflectance) at the hit's texture coordinate; 0 = the constant `a` */
    /* roughplastic: transmittance of the rough coat for cos(theta) = max(1e-6, k / 63), k = 0 .. 63 — mitsuba computes
     * this table when the plugin is built (RoughPlastic::parameters_changed: eval_transmittance by Gauss-Legendre
     * quadrature over visible normals); the caller does the same (mitransient_amd/scene.py: rough_plastic_tables) and the
     * library only interpolates it */
    float    external_transmittance[MTR_ROUGH_TRANSMITTANCE_RES];
} mtr_material;

/* `bitmap` texture (mitsuba: filter_type = bilinear, wrap_mode = repeat, to_uv = identity): linear RGB */
typedef struct mtr_texture {
    uint32_t width, height;
    const float *rgb;      /* host, height * width * 3 floats, row 0 first (v = 0), already linear (sRGB decoded by the caller) */
} mtr_texture;

/* ---- emitters: `area` emitter attached to a `rectangle` (analytic sampling), to a triangle mesh or (ABI 23) to an analytic
 *      `sphere`; (ABI 22) mitsuba's `point` and `spot` emitters, which no ray can hit and no triangle references ---- */
enum { MTR_EMITTER_AREA = 0,   /* `area` / `angulararea` on a shape: every caller up to ABI 21 */
       MTR_EMITTER_POINT = 1,  /* mitsuba `point`: position = center, intensity = radiance; sample_direction has ds.pdf = 1, ds.delta,
                                  weight intensity / dist^2 */
       MTR_EMITTER_SPOT = 2    /* mitsuba `spot`: the same from center along `axis`, times the falloff of the angle to the axis: 1 inside
                                  beam_width, linear in the angle down to 0 at cutoff_angle (cutoff / cos_cutoff / cos_beam /
                                  inv_transition below, the curve `angulararea` copied from it) */,
       MTR_EMITTER_SPHERE = 3  /* (ABI 23) an `area` emitter on an analytic sphere (mtr_shape.kind = MTR_SHAPE_SPHERE, whose one carrier
                                  triangle references it): center, radius, flip_normals (the emitting side is the inside).
                                  mitsuba's Sphere::sample_direction [upstream-unverified]: from outside the cone the sphere subtends
                                  is sampled, pdf 1 / (2 pi (1 - cos theta_max)); from inside the surface uniformly, pdf
                                  dist^2 / (4 pi r^2 |cos|).  du, dv, is_mesh, first_tri, n_tris and angular are ignored */ };
typedef struct mtr_emitter {
    float center[3];      /* rectangle: to_world * (0,0,0); point / spot: the position */
    float du[3];          /* rectangle: to_world * (1,0,0) - center  (half edge) */
    float dv[3];          /* rectangle: to_world * (0,1,0) - center  (half edge) */
    float radiance[3];
    uint32_t is_mesh;     /* 1: the emitter is the triangle range below (obj / cube shapes) */
    uint32_t first_tri, n_tris;
    uint32_t flip_normals; /* rectangle (ABI 9): the shape's `flip_normals` — the emitting side is -normalize(du x dv);
                              sample positions are unchanged (mitsuba negates the normal, not the parameterisation).
                              A mesh emitter's flip is the winding of its triangles. */
    /* ABI 13: mitransient's `angulararea` emitter (mitransient/emitters/angulararea.py) on the same shapes.  All zero: a plain `area`
       emitter.  The constants are the f32 values AngularAreaLight.__init__ derives (:55-72), computed by the caller. */
    uint32_t angular;      /* 1: radiance is scaled by the falloff of the angle to the shading normal (_fallof_curve, :74-82)      */
    float cutoff;          /* deg2rad(cutoff_angle) (:58-59), default 10 degrees                                                   */
    float cos_cutoff;      /* cos(cutoff) (:68)                                                                                     */
    float cos_beam;        /* cos(deg2rad(beam_width)) (:60-61, :69), beam_width defaults to cutoff_angle                          */
    float inv_transition;  /* 1 / (cutoff - beam), +inf when they are equal (:62-66)                                               */
    /* ABI 22 */
    uint32_t kind;         /* MTR_EMITTER_*.  Point and spot: du, dv, is_mesh, first_tri, n_tris, flip_normals and angular are ignored,
                              `radiance` holds the intensity; a spot's four falloff constants are read (finite, cutoff >= beam; inv_transition +inf when equal)     */
    float axis[3];         /* spot: the unit world-space direction of the beam (to_world's +z axis); to_world is rigid                   */
    /* ABI 23 */
    float radius;          /* MTR_EMITTER_SPHERE: the world radius (> 0), about `center`                                                */
} mtr_emitter;

/* ---- sensor: `perspective` (utils.py:92-105 of the reference) ----------- */
typedef struct mtr_camera {
    float sample_to_camera[16]; /* row-major 4x4 projective, film sample [0,1]^2 -> camera near plane */
    float to_world[16];         /* row-major 4x4 camera -> world (rigid)         */
    float near_clip, far_clip;
} mtr_camera;

/* ---- film: `transient_hdr_film` (transient_hdr_film.py:114-121) --------- */
typedef struct mtr_film_desc {
    uint32_t width, height;               /* full film size (tensor is H x W x T x 4)  */
    uint32_t crop_width, crop_height;     /* sampled window                            */
    uint32_t crop_offset_x, crop_offset_y;
    uint32_t temporal_bins;               /* T  (default 2048)                         */
    float    start_opl;                   /* default 0                                 */
    float    bin_width_opl;               /* default 0.003                             */
    /* `exhaustive_scan` (transient_hdr_film.py:119-121, transient_image_block.py:63-66,134-140): both > 0 makes
     * the tensor H x W x laser_scan_height x laser_scan_width x T x 4 with the reference's flat index
     * ((((y*W + x)*laser_scan_width + laser_x)*laser_scan_height + laser_y)*T + t)*4; 0/0 = plain H x W x T x 4 */
    uint32_t laser_scan_width, laser_scan_height;
    /* `phasor_hdr_film` (mitransient/films/phasor_hdr_film.py:125-139, render/phasor_image_block.py:42-67): n_frequencies > 0
     * makes the tensor H x W x (2F + 1) — per frequency the real and imaginary part of sum(value * exp(i * phase)),
     * phase = fmod(-2 pi f (opl - start_opl), 2 pi), then the weight channel — instead of time bins; every finite optical
     * path length counts (temporal_bins / bin_width_opl only choose the frequencies, on the host).  Monochromatic: the
     * value is channel 0 of the contribution.  frequencies: host pointer, read during the call that takes the desc.
     * (ABI 21) Both integrators render into it: transient_path, and the NLOS tier with a Single or Confocal capture (an
     * Exhaustive capture needs the exhaustive_scan rows a phasor film does not have: MTR_ERR_UNSUPPORTED). */
    uint32_t n_frequencies;
    const float *frequencies;
} mtr_film_desc;

/* ---- NLOS tier: `transient_nlos_path` + `nlos_capture_meter` + `projector` ---------------
 * (reference: mitransient/integrators/transientnlospath.py:200-249 properties, :251-383 prepare;
 *  mitransient/sensors/nloscapturemeter.py:93-202; mitsuba's `projector` emitter)            */
enum { MTR_CAPTURE_SINGLE = 1, MTR_CAPTURE_CONFOCAL = 2,
       MTR_CAPTURE_EXHAUSTIVE = 3 /* every scanned point x every illuminated point: needs an exhaustive_scan film */ };
enum { MTR_NLOS_LASER_SAMPLING = 1u,          /* nlos_laser_sampling                              */
       MTR_NLOS_HG_SAMPLING = 2u,             /* nlos_hidden_geometry_sampling                    */
       MTR_NLOS_HG_RROULETTE = 4u,            /* nlos_hidden_geometry_sampling_do_rroulette       */
       MTR_NLOS_HG_INCLUDES_WALL = 8u,        /* nlos_hidden_geometry_sampling_includes_relay_wall*/
       MTR_NLOS_ACCOUNT_FIRST_LAST = 16u,     /* account_first_and_last_bounces                   */
       MTR_NLOS_DISCARD_DIRECT = 32u,         /* discard_direct_paths                             */
       MTR_NLOS_FORCE_EQUAL_GRIDS = 64u       /* force_equal_illumination_scanning (Exhaustive)   */ };

enum { MTR_RECT_ANALYTIC = 1u, MTR_RECT_FLIP_NORMALS = 2u };     /* mtr_shape.is_rectangle */
enum { MTR_SHAPE_DEFAULT = 0u,          /* mtr_shape.kind (ABI 23): what is_rectangle says — an analytic rectangle or a triangle mesh */
       MTR_SHAPE_SPHERE = 1u,           /* mitsuba's analytic `sphere` */
       MTR_SHAPE_FLIP_NORMALS = 0x100u  /* ... with `flip_normals` (a bit beside the kind): both normals are -normalize(p - center) */ };
typedef struct mtr_shape {          /* one scene shape = a contiguous triangle range */
    uint32_t first_tri, n_tris;
    uint32_t is_rectangle;          /* analytic `rectangle`: the shape is ONE primitive — mitsuba's Rectangle::ray_intersect
                                       (ray to object space, t = -o.z/d.z, |x|,|y| <= 1), one shading frame, sample_position by
                                       to_world.  Its two triangles (0,1,2) (0,2,3) of the corners (-1,-1) (1,-1) (1,1) (-1,1)
                                       only CARRY the material / emitter / index of the primitive (hits report the first one).
                                       Bit MTR_RECT_FLIP_NORMALS (ABI 9): the shape's `flip_normals` — geometric and shading
                                       normal are -normalize(du x dv) (and t = n x s follows); the local parameterisation,
                                       hence prim_uv and sample_position, is unchanged. */
    float    center[3], du[3], dv[3];   /* rectangle only: to_world*(0,0,0), half edges to_world*(1,0,0) - center, to_world*(0,1,0) - center */
    uint32_t has_to_world;          /* meshes: to_world below is the shape's object -> world transform (cube: of [-1,1]^3; obj / ply:
                                       of the file's coordinates).  Only an acceleration hint (oriented bounds); 0 = unknown */
    float    to_world[12];          /* row-major 3 x 4 affine */
    /* ABI 23 */
    uint32_t kind;                  /* MTR_SHAPE_*.  MTR_SHAPE_SPHERE: the shape is ONE primitive — mitsuba's Sphere [upstream-unverified]:
                                       |o + t d - center|^2 = radius^2, roots from the point of closest approach; no hit for a ray wholly
                                       inside; the far root when the origin is inside; n = normalize(p - center), p re-projected to
                                       center + radius n; dp_du = to_world (-local.y, local.x, 0), coordinate_system(n) at the poles; no uv.
                                       is_rectangle is 0, `center` and `radius` are the world sphere, to_world (has_to_world = 1; a rotation
                                       times a uniform scale, then the translation) orients the tangent.  It owns ONE carrier triangle, which
                                       only carries material / emitter / index: it is never intersected and never sampled. */
    float    radius;                /* sphere only: |to_world (1,0,0) - center| > 0 */
} mtr_shape;

#define MTR_NLOS_NO_RELAY 0xffffffffu
typedef struct mtr_nlos_desc {
    float    sensor_origin[3];      /* nlos_capture_meter.sensor_origin (nloscapturemeter.py:103-105)     */
    uint32_t relay_shape;           /* index into shapes[]: the rectangle the nlos_capture_meter is attached to;
                                       MTR_NLOS_NO_RELAY: the sensor is the scene's `perspective` camera
                                       (mtr_scene_desc.camera), as in examples/transient-nlos/nlos-z-simple.xml      */
    float    laser_to_world[16];    /* projector world transform, row-major (after nlos.focus_emitter_*)   */
    float    laser_fov;             /* degrees, along x                                                    */
    float    laser_irradiance[3];   /* constant `irradiance` texture                                       */
    float    laser_scale;           /* `scale` (default 1)                                                 */
    uint32_t capture_type;          /* MTR_CAPTURE_*                                                       */
    uint32_t flags;                 /* MTR_NLOS_*                                                          */
    int32_t  filter_depth;          /* -1 = off (filter_bounces + 1 when that was given)                   */
    float    illumination_scan_fov; /* Exhaustive without FORCE_EQUAL_GRIDS: fov (degrees) of the laser grid scan
                                       (transientnlospath.py:346-376); the grid is film.laser_scan_width x _height */
    uint32_t n_shapes;
    const mtr_shape *shapes;        /* host; every triangle of the scene belongs to exactly one shape      */
    /* `is_confocal` capture meter (nloscapturemeter.py:111-119, :142): a 1 x 1 film whose every sensor ray goes to
     * nlos_capture_meter.laser_target (set by mitransient.nlos.focus_emitter_*) instead of the pixel-centre grid */
    uint32_t sensor_is_confocal;
    float    sensor_target[3];
} mtr_nlos_desc;

typedef struct mtr_scene_desc {
    uint32_t        n_tris;
    const float    *tri_verts;     /* host, n_tris*9 floats: p0 p1 p2, world space      */
    const uint32_t *tri_material;  /* host, n_tris: index into materials                */
    const int32_t  *tri_emitter;   /* host, n_tris: index into emitters or -1           */
    uint32_t        n_materials;
    const mtr_material *materials; /* host                                              */
    uint32_t        n_emitters;
    const mtr_emitter  *emitters;  /* host                                              */
    mtr_camera      camera;         /* with nlos != NULL: used only when nlos->relay_shape == MTR_NLOS_NO_RELAY */
    mtr_film_desc   film;
    const mtr_nlos_desc *nlos;      /* NULL: `perspective` sensor + `transient_path`; else the NLOS tier */
    /* Shape table (host; optional): shapes tile the triangle array in order.  Needed for analytic rectangles
     * (mtr_shape.is_rectangle); without it every triangle is a plain mesh triangle.  With nlos != NULL it must be the
     * same table as nlos->shapes. */
    uint32_t        n_shapes;
    const mtr_shape *shapes;
    /* Per-corner texture coordinates (host, n_tris*6 floats: uv0 uv1 uv2; optional).  They only fix the tangent of the
     * shading frame, as in mitsuba's Mesh::compute_surface_interaction: dp_du from the UV parameterisation when it is
     * not degenerate, coordinate_system(n) otherwise (and for every triangle when this is NULL); then
     * SurfaceInteraction::initialize_sh_frame: s = normalize(dp_du - n * dot(n, dp_du)), t = n x s. */
    const float    *tri_uv;
    /* Per-corner SHADING normals (host, n_tris*9 floats: n0 n1 n2, unit length, world space; optional; ABI 8).  A triangle
     * whose nine floats are all zero — and every triangle when this is NULL — is flat-shaded (face_normals = true, cube,
     * rectangle).  Otherwise, as in mitsuba's Mesh::compute_surface_interaction: sh_frame.n = normalize(b0 n0 + b1 n1 +
     * b2 n2), the tangent from dp_du by initialize_sh_frame; the geometric normal (si.n) keeps the ray offsets.  Meshes that are
     * SAMPLED (area emitters, NLOS hidden geometry) interpolate the same normals in Mesh::sample_position. */
    const float    *tri_normals;
    /* Bitmap textures referenced by mtr_material.albedo_texture (host; optional).  The lookup uses tri_uv exactly as given:
     * uv = fmadd(uv2, b2, fmadd(uv1, b1, uv0 b0)) (a rectangle: (prim_uv + 1) / 2); mitsuba's OBJ loader flips v
     * (flip_tex_coords), the caller passes the flipped coordinates. */
    uint32_t        n_textures;
    const mtr_texture *textures;
} mtr_scene_desc;

/* ---- integrator: `transient_path` properties (common.py:22-30) ---------- */
enum { MTR_FLAG_CAMERA_UNWARP = 1u,        /* common.py:25, transientpath.py:133-138 */
       MTR_FLAG_DISCARD_DIRECT_LIGHT = 2u, /* common.py:27, transientpath.py:173-176 */
       MTR_FLAG_FILM_ZERO = 4u,            /* caller guarantees that the film rows of the rendered pixels are
                                              all-zero on entry (first pass after TransientImageBlock.clear):
                                              the row flush may store instead of read-modify-write            */
       MTR_FLAG_KEEP_COUNTERS = 16u,       /* do not reset the context's device counters at the start of this call: a render
                                              issued as several asynchronous calls (row bands on alternating streams) sums
                                              its counters on the device; read them once with mtr_counters_read()        */
       MTR_FLAG_DETERMINISTIC = 32u,       /* fused kernel: accumulate the LDS rows (and the steady sums) in signed 2^-42 fixed
                                              point with 64-bit integer atomics instead of f32 atomics: sums no longer depend
                                              on the order in which lanes add, so two runs give the same bits (the wavefront
                                              organisation's scatter kernel always works this way).  Twice the LDS per row.  */
       MTR_FLAG_DEVELOPED_ROWS = 64u,      /* single-pass film lifecycle (ABI 9): `transient_hwt4` of mtr_render is the DEVELOPED tensor
                                              (H, W, T, 3) — for every pixel of [pixel_begin, pixel_end) the whole row is STORED,
                                              zeros included — so the call replaces mtr_film_clear + mtr_render +
                                              mtr_film_develop of the transient tensor (the weight channel of the reference's
                                              raw block stays 0: develop divides by 1, the developed values ARE the raw sums).
                                              The row holds the samples of THIS call only: use it when one call renders all
                                              samples of its pixels.  Honoured by the fused organisation with LDS rows
                                              (mtr_render_plan reports it); MTR_ERR_UNSUPPORTED otherwise.               */
       MTR_FLAG_PCG_INITSEQ_PLUS_LANE = 8u /* sampler seeding variant: PCG32 initseq = TEA.v1 + lane instead of TEA.v1.
                                              drjit's PCG32::seed(size, initstate, initseq) adds arange(size) to initseq;
                                              mitsuba's independent sampler passes size = 1 after the TEA scramble in the
                                              versions we know [upstream-unverified, SURVEY A.9].  Kept so that ONE real
                                              reference render decides the question without a code change
                                              (tests/test_reference_golden.py).                                */,
       MTR_FLAG_POLARIZED = 256u,          /* (ABI 14) the *_mono_polarized variants: polarized transport (mitransient's transient_path with
                                              mi.is_polarized, transientpath.py:140-318).  The path throughput is a Mueller matrix
                                              (beta_init, utils.py:9-21; beta = beta * bsdf_weight, :233; BSDF values and weights through
                                              si.to_world_mueller, :210, :222-226; Russian roulette on M00, :244-253) and every
                                              emitter a depolarizer, so a contribution is column 0 of the Mueller value.  Channel 0 of
                                              every colour is used (the monochromatic variant).  OUTPUT CONTRACT:
                                              `transient_hwt4` (H, W, T, 4) receives (S0, S1, S2, S3) per bin — value[0..3, 0, 0] of
                                              the splat (transient_image_block.py:93-95; channels "0123W" of transient_hdr_film.py:176-177
                                              without the weight, which is 0 for every transient splat): the developed tensor IS the raw
                                              one, mtr_film_develop must not be applied to it.  `steady_hw4` receives (S0, S1, S2, weight)
                                              per pixel; the steady image is S0 / weight (unpolarized_spectrum(L), integrators/
                                              common.py:108-112), which mtr_film_develop computes in channel 0.
                                              Scenes: diffuse, conductor, roughconductor, dielectric (also two-sided) and `area`
                                              emitters; anything else, the NLOS tier and a phasor film are MTR_ERR_UNSUPPORTED.
                                              Wavefront organisation only: MTR_MODE_AUTO resolves to MTR_MODE_WAVEFRONT,
                                              MTR_MODE_FUSED is MTR_ERR_UNSUPPORTED, and so are MTR_FLAG_DEVELOPED_ROWS and band words. */
       MTR_FLAG_PCG_TEA64 = 128u           /* a third reading of the same call site (round 5; a new flag bit, no ABI change): m_rng.seed(1, sample_tea_64(seed, idx),
                                              sample_tea_64(idx, seed)) — 64-bit state and stream words, each the two TEA
                                              outputs glued together (v0 + (v1 << 32)) — instead of the two halves of one
                                              sample_tea_32(seed, idx) [upstream-unverified].  Wins over PLUS_LANE if both are set. */ };
/* SHADOW HULL MARGIN (round 15; bits 16..31 of `flags`, zero in every earlier caller: no ABI change).  In a room of rectangles with one
   rectangular light the fused kernel spares a shadow ray the rectangle tests it provably cannot pass (mtr_scene_shadow_hull says whether
   the scene is one); a lane is spared only when its ray origin lies a guard distance inside the walls' planes and in front of the light.
   The field v multiplies those distances by v + 1 (0: as derived; larger: only more careful, the same picture bit for bit);
   MTR_SHADOW_HULL_OFF switches the feature off for the call. */
#define MTR_SHADOW_HULL_SHIFT 16u
#define MTR_SHADOW_HULL_OFF   0xffffu

/* which kernel organisation executes the path */
enum { MTR_MODE_AUTO = 0,
       MTR_MODE_FUSED = 1,      /* one persistent launch per tile; per-pixel LDS time histogram */
       MTR_MODE_WAVEFRONT = 2,  /* per-bounce launches over SoA path queues in HBM + splat
                                   records + the stand-alone time-bin scatter-add kernel        */
       MTR_MODE_SAMPLES = 3     /* (ABI 24) a pixel's samples spread over workgroups: work item = (pixel, slab of the call's samples),
                                   one LDS row per workgroup, the slabs' rows summed by a second kernel in slab order.  For films of
                                   one or a few pixels with very many samples (a `radiancemeter`, a SPAD array), which the two
                                   organisations above — a whole pixel per workgroup — leave on a handful of workgroups.  On request
                                   only: MTR_MODE_AUTO never resolves to it.  transient_path into a plain transient_hdr_film with f32
                                   rows; honours sample and pixel sub-ranges, spp_scale, crop windows, MTR_FLAG_CAMERA_UNWARP,
                                   _DISCARD_DIRECT_LIGHT, _FILM_ZERO, _KEEP_COUNTERS and the seeding flags.  MTR_ERR_UNSUPPORTED,
                                   before any launch and with both tensors untouched: the NLOS tier, a phasor film, an
                                   exhaustive_scan film, MTR_FLAG_POLARIZED, MTR_FLAG_DETERMINISTIC, MTR_FLAG_DEVELOPED_ROWS, band
                                   words, and a time-bin row that with the traversal stack (and the scene, when even the HBM walk
                                   leaves no room) exceeds 160 KiB of LDS.  The splat log is not written.  The slabs' rows live in a
                                   context-owned workspace ((pixels, slabs, 3 T + 4) f32; above 256 MiB released by the call,
                                   otherwise by mtr_ctx_trim).                                                              */ };

typedef struct mtr_render_params {
    uint32_t spp_total;     /* samples per pixel of the WHOLE render: sample_scale = 1/spp_total
                               (common.py:173-175) and lane = pixel*spp_total + s             */
    uint32_t spp_begin;     /* this call renders samples s in [spp_begin, spp_end) ...         */
    uint32_t spp_end;
    uint32_t pixel_begin;   /* ... of crop-window pixels [pixel_begin, pixel_end) (row-major)  */
    uint32_t pixel_end;
    uint32_t seed;          /* mi.render(seed=) + sampler base seed (common.py:52)             */
    int32_t  max_depth;     /* -1 = unbounded                                                   */
    int32_t  rr_depth;
    uint32_t flags;         /* MTR_FLAG_*                                                       */
    uint32_t mode;          /* MTR_MODE_*                                                       */
    uint32_t spp_scale;     /* 0, or the sample count of the WHOLE multi-pass render (common.py:56-85: above 2^32 lanes
                               the reference renders passes of their own sampler each — lanes of a pass are indexed with
                               spp_total = the PASS's samples — while sample_scale stays 1/total_spp, :173-175)       */
    uint32_t reserve_cus;   /* (ABI 10) fused organisation: leave this many compute units WITHOUT a resident workgroup of the
                               persistent path kernel (grid = (CUs - reserve_cus) x workgroups per CU; at least one CU is
                               used).  The kernel otherwise owns every CU's LDS for the whole launch, so kernels of other
                               streams — RCCL's reduce-scatter of the previous row band — could only start between two
                               launches.  0 = use every CU (one GPU; the measured cost of 8 / 16 is in DESIGN.md section 7) */
    /* BAND COMPLETION WORDS (round 5; the struct's former reserved words: no ABI change).  n_bands > 0, fused organisation only
       (MTR_ERR_UNSUPPORTED otherwise: ask mtr_render_plan first): the pixel range is split into n_bands equal contiguous bands
       (the last takes the remainder) and, when every pixel of band b has been flushed to the film, the kernel stores band_epoch to
       band_done[b] with a system-scope release — rows and steady sums of the band are then visible to whatever waits for that
       word (hipStreamWaitValue32 on another stream: a multi-GPU caller starts band b's film reduction while the SAME launch still
       renders band b + 1, instead of issuing one launch per band).  The caller owns band_done (device memory, n_bands words) and
       picks an epoch the words do not hold yet.                                                                        */
    uint32_t n_bands;
    uint32_t band_epoch;
    uint64_t band_done;     /* device pointer (uint32_t *), or 0 */
} mtr_render_params;

/* in-kernel counters */
typedef struct mtr_counters {
    uint64_t paths;
    uint64_t rays_closest;
    uint64_t rays_shadow;
    uint64_t splats_issued;   /* in-range, non-zero time-bin contributions                      */
    uint64_t bounces;         /* loop iterations executed                                       */
    uint64_t splats_overflow; /* wavefront mode: records that took the global-atomic fallback   */
    uint64_t reserved[2];
} mtr_counters;

/* one time-resolved contribution, as consumed by the stand-alone scatter-add */
typedef struct mtr_splat_soa {
    const uint32_t *pixel;   /* device, n: y*W + x (film coordinates)                          */
    const float    *opl;     /* device, n: optical path length                                 */
    const float    *r, *g, *b; /* device, n: value already multiplied by sample_scale          */
    uint64_t        n;
    const uint32_t *laser;   /* device, n, or NULL (= 0): laser_x*laser_scan_height + laser_y of an
                                exhaustive_scan film (add_transient_data's laser_x / laser_y)    */
} mtr_splat_soa;

/* per-kernel timing of the last mtr_render (HIP events on the context stream) */
typedef struct mtr_kernel_times {
    float    total_ms;        /* whole mtr_render call on the stream                            */
    float    trace_ms;        /* fused: the path kernel | wavefront: sum of bounce kernels      */
    float    scatter_ms;      /* wavefront: sum of time-bin scatter-add launches (0 if fused)   */
    uint32_t trace_launches;
    uint32_t scatter_launches;
    float    wf_trace_ms;     /* wavefront (ABI 9): sum of the k_wf_trace launches alone (closest-hit and any-hit runs) */
    uint32_t wf_trace_kernel_launches; /* ... and their number                                   */
    float    wf_shade_ms;     /* wavefront (ABI 10): sum of the k_wf_shade launches (HBM-bound for scenes in HBM) */
} mtr_kernel_times;

typedef struct mtr_ctx   mtr_ctx;
typedef struct mtr_scene mtr_scene;

/* ------------------------------------------------------------------------ */
int  mtr_abi_version(void);

/* Context = one GPU + one stream.  device_ordinal >= 0 is required: this
 * library has no CPU path (MTR_ERR_NO_DEVICE when HIP sees no device). */
int  mtr_ctx_create(int device_ordinal, mtr_ctx **out);
void mtr_ctx_destroy(mtr_ctx *);
int  mtr_ctx_set_stream(mtr_ctx *, void *hip_stream);
const char *mtr_last_error(const mtr_ctx *);   /* never NULL; ctx may be NULL for creation errors */

/* Replaces mi.load_dict(scene_dict) for the supported subset (reference
 * call site: README.md:159, utils.py:78-220).  Copies the arrays, builds the
 * BVH2 on the host and uploads it. */
int  mtr_scene_create(mtr_ctx *, const mtr_scene_desc *, mtr_scene **out);
void mtr_scene_destroy(mtr_scene *);
/* transient_hdr_film traverse()/parameters_changed (transient_hdr_film.py:295-311):
 * change T / start / width between renders. */
int  mtr_scene_set_film(mtr_scene *, const mtr_film_desc *);
/* (ABI 24) Replace the sensor: the next render's camera rays come from `camera`; nothing else is rebuilt (a scanned
 * `radiancemeter` is a loop over this call and mtr_render).  Renders already enqueued keep the camera they were launched with.
 * MTR_ERR_UNSUPPORTED for a scene with the NLOS tier, whose tables are derived from the sensor (mtr_scene_set_nlos). */
int  mtr_scene_set_camera(mtr_scene *, const mtr_camera *);
/* NLOS tier: (re)derive the laser / relay-wall / hidden-geometry tables and the scanned points
 * (TransientNLOSPath.prepare, transientnlospath.py:251-383) after mitransient.nlos.focus_emitter_*
 * (nlos.py:5-70) or an integrator property changed.  The shape table must match the scene's triangles. */
int  mtr_scene_set_nlos(mtr_scene *, const mtr_nlos_desc *);
/* BVH statistics for tests: nodes, max depth, leaf count. */
int  mtr_scene_bvh_info(const mtr_scene *, uint32_t *n_nodes, uint32_t *max_depth, uint32_t *n_leaves);
/* Which specialised kernels the scene's tables select (for tests and tools; no counterpart in the reference, whose tracing
 * JIT specialises on the scene implicitly): MTR_TRAIT_* bits. */
#define MTR_TRAIT_DIFFUSE          1u   /* every material plain one-sided diffuse */
#define MTR_TRAIT_ONE_RECT_EMITTER 2u   /* exactly one emitter, an analytic rectangle (`area`, not `angulararea`, no point / spot emitter) */
#define MTR_TRAIT_LEAF_PAIR        4u   /* no leaf of the LDS-staged tree beyond one triangle pair */
#define MTR_TRAIT_FLAT_TOP         8u   /* top level = rectangles, triangle leaves and box nodes: the fused kernel does not walk a tree */
#define MTR_TRAIT_FLAT_LEAVES     16u   /* ... and there are triangle leaves among them */
#define MTR_TRAIT_NO_LOBES        32u   /* extended shading (interpolated normals, bitmaps) without any microfacet lobe / plastic / thin dielectric */
#define MTR_TRAIT_GREY            64u   /* every colour (materials, emitters, the NLOS laser) has three equal channels, no bitmaps: r == g == b in every contribution */
int  mtr_scene_traits(const mtr_scene *, uint32_t *traits);
/* SHADOW HULL (round 15; a new entry point, nothing a caller of ABI 24 uses moves): is the scene a room of rectangles with one
 * rectangular light in the sense of MTR_SHADOW_HULL_SHIFT above?  *n_hull_rectangles receives the number of rectangles a safe shadow
 * ray is spared (the walls: every top-level rectangle but the light), 0 when the scene is no such room.  Reported here and not as a
 * bit of mtr_scene_traits: that word selects kernels and is compared for equality. */
int  mtr_scene_shadow_hull(const mtr_scene *, uint32_t *n_hull_rectangles);
/* (ABI 15) mi.traverse(scene) parameters changed (params.update()): new constant colours for the scene's tables, without
 * rebuilding anything else — material_a (host, n_materials x 3) replaces every mtr_material.a, emitter_radiance (host,
 * n_emitters x 3) every mtr_emitter.radiance; the traits that depend on colours are decided again.  Synchronises the context's
 * stream.  MTR_ERR_UNSUPPORTED for a scene with the NLOS tier (recreate it). */
int  mtr_scene_set_colors(mtr_scene *, const float *material_a, const float *emitter_radiance);
/* (ABI 16) ... and new texels for one bitmap (params["<bsdf>.reflectance.data"], Mitsuba's BitmapTexture parameter `data`):
 * rgb (host, height x width x 3 floats, row 0 first, linear RGB, the size the texture was created with) replaces texture
 * `index` of mtr_scene_desc.textures on the device, and `a` of every material that references it becomes the new mean colour
 * (summed in f64, rounded to f32 once), so that the scene is the one a fresh mtr_scene_create with these texels gives; a caller
 * that computes the stand-in its own way (the Python layer: an f32 mean) follows with mtr_scene_set_colors.
 * Nothing else is rebuilt.  Synchronises the context's stream.  MTR_ERR_INVALID for an unknown index, MTR_ERR_UNSUPPORTED for a
 * scene with the NLOS tier. */
int  mtr_scene_set_texture(mtr_scene *, uint32_t index, const float *rgb);
/* (ABI 16) Where texture `index` lies in the texel array of mtr_render_grad_tex: its first texel (textures follow each other in
 * scene order, row 0 first) and its size.  Any output may be NULL; index == n_textures answers first_texel = the number of texels
 * of the whole scene (width = height = 0). */
int  mtr_scene_texture_layout(const mtr_scene *, uint32_t index, uint32_t *first_texel, uint32_t *width, uint32_t *height);

/* (ABI 19) The tint slots of mtr_render_grad_tint / mtr_render_fwd_tint (the reference: `specular_reflectance.value` and
 * `specular_transmittance.value` of a BSDF are ordinary parameters of mi.traverse, common.py:215-409): one slot per constant tint
 * the shading code multiplies a lobe by — materials in table order, `specular_reflectance` (which 0, mtr_material.c) of
 * MTR_BSDF_CONDUCTOR, ROUGHCONDUCTOR, DIELECTRIC, THINDIELECTRIC and ROUGHDIELECTRIC, then `specular_transmittance` (which 1,
 * mtr_material.c2) of the three dielectric types.  PLASTIC and ROUGHPLASTIC have none: their tint enters lobe sampling.
 * *n_slots receives the count (0 for a scene with the NLOS tier); slot_material / slot_which (host, n_slots words each, or NULL)
 * the material index and 0 | 1 of every slot.  A caller maps the tints it exposes as parameters to slots and ignores the others. */
int  mtr_scene_tint_layout(const mtr_scene *, uint32_t *n_slots, uint32_t *slot_material, uint32_t *slot_which);
/* (ABI 19) params.update() of a tint: material_c / material_c2 (host, n_materials x 3 each) replace mtr_material.c / .c2 of every
 * material that has the slot (other materials keep theirs: c2 of an anisotropic roughconductor holds alpha_v); the traits that
 * depend on colours are decided again, nothing else is rebuilt.  Synchronises the context's stream.  MTR_ERR_UNSUPPORTED for a
 * scene with the NLOS tier. */
int  mtr_scene_set_tints(mtr_scene *, const float *material_c, const float *material_c2);

/* TransientImageBlock.clear (transient_image_block.py:56-70): zero the
 * (H,W,T,4) f32 accumulator and the (H,W,4) steady accumulator. */
int  mtr_film_clear(mtr_ctx *, const mtr_film_desc *, float *transient_hwt4 /*device, may be NULL*/,
                    float *steady_hw4 /*device, may be NULL*/);

/* TransientADIntegrator.render pass (common.py:157-210) + TransientPath.sample
 * (transientpath.py:88-326) + add_transient_data/put_/accum
 * (transient_hdr_film.py:250-276, transient_image_block.py:103-151):
 * ADDS the contributions of the requested lanes into
 *   transient_hwt4 : device f32 (H, W, T, 4)  channels R,G,B,W (W stays 0)
 *   steady_hw4     : device f32 (H, W, 4)     sum of L over samples, and the sample count in .w
 * counters/times may be NULL.  Asynchronous on the context stream unless
 * counters or times are requested (then it synchronises the stream).
 * A phasor film (mtr_film_desc.n_frequencies > 0): transient_hwt4 is device f32 (H, W, 2F + 1) instead.
 * (ABI 21) ... also for a scene with the NLOS tier, Single or Confocal capture (up to ABI 20: MTR_ERR_UNSUPPORTED).  Under
 * MTR_MODE_AUTO such a render runs the fused kernel — (Re, Im) rows in LDS — when the scene has plain shading, the 2F floats
 * of a row fit LDS beside the staged scene and F <= 16 (measured: DESIGN.md section 6), and the wavefront organisation ((opl,
 * value) records) otherwise; MTR_MODE_FUSED runs any F whose rows fit and is MTR_ERR_UNSUPPORTED with extended shading or
 * rows that do not fit.  MTR_ERR_UNSUPPORTED, before any launch and with both tensors
 * untouched: an Exhaustive capture with a phasor film, and MTR_FLAG_POLARIZED on the NLOS tier or with a phasor film. */
int  mtr_render(mtr_scene *, const mtr_render_params *,
                float *transient_hwt4, float *steady_hw4,
                mtr_counters *counters_out /*host*/, mtr_kernel_times *times_out /*host*/);

/* Which kernel organisation mtr_render would run for these parameters on this scene (MTR_MODE_AUTO resolved exactly as
 * mtr_render resolves it; MTR_MODE_FUSED or MTR_MODE_WAVEFRONT in *mode_out; (ABI 24) MTR_MODE_SAMPLES for MTR_MODE_SAMPLES, or
 * its refusal).  A caller that overlaps several mtr_render
 * calls of ONE scene on different streams needs this: only the fused organisation keeps its per-launch state apart
 * (rotating work tickets); the wavefront organisation has one workspace per scene and must stay on one stream. */
int  mtr_render_plan(mtr_scene *, const mtr_render_params *, uint32_t *mode_out,
                     uint32_t *developed_rows_ok /* may be NULL: 1 when MTR_FLAG_DEVELOPED_ROWS would be honoured */);
/* (ABI 24) What MTR_MODE_SAMPLES would run for these parameters (params.mode is not read): samples per slab, slabs per pixel
 * (the last one ragged; never more slabs than samples), whether the scene is staged in LDS (0: walked in HBM) and whether the
 * extended shading code runs — together the instantiation of the path kernel.  Any pointer may be NULL.  Refuses what
 * mtr_render refuses in that mode. */
int  mtr_render_samples_plan(mtr_scene *, const mtr_render_params *, uint32_t *slab_len, uint32_t *n_slabs,
                             uint32_t *scene_in_lds, uint32_t *extended);

/* (ABI 15) Reverse-mode gradients of transient_path: TransientADIntegrator.render_backward (common.py:325-409) with
 * TransientPath.sample's backward pass (transientpath.py:88-326, :284-299).  For the lanes of `params` (the same lanes, seeds
 * and passes mtr_render would run) the gradient of  sum g_s . steady + sum g_t . transient  of the seeded estimator is STORED to
 *   grad_materials : device f32 (n_materials, 3)  d loss / d reflectance of every plain `diffuse` material (constant `a`;
 *                                                  other materials receive 0, and so do bitmap-textured ones: their
 *                                                  gradient is per texel, mtr_render_grad_tex)
 *   grad_emitters  : device f32 (n_emitters, 3)   d loss / d radiance of every `area` / `angulararea` emitter, (ABI 22) d loss /
 *                                                 d intensity of every `point` / `spot` emitter
 * with the upstream gradients of the DEVELOPED tensors
 *   grad_steady_hw3     : device f32 (H, W, 3)
 *   grad_transient_hwt3 : device f32 (H, W, T, 3)
 * Sampling is detached (Russian-roulette probabilities, BSDF and emitter sampling are constants); a contribution's transient
 * weight is read at its own time bin (film_bin of its optical path length), which departs from the reference's single read at the
 * vertex distance — DESIGN.md §2.  A render split into passes (pixel / sample ranges, spp_scale) has the sum of its passes'
 * gradients.  Only an RGB transient_hdr_film: a phasor film, an exhaustive_scan film and MTR_FLAG_POLARIZED are
 * MTR_ERR_UNSUPPORTED.  params.mode, n_bands and the film flags are ignored.  Synchronises the stream.
 * (ABI 17) A scene with a NLOS description (transient_nlos_path, Single or Confocal capture; Exhaustive: MTR_ERR_UNSUPPORTED) is
 * differentiated as well: grad_materials as above (hidden geometry and relay wall), and grad_emitters is (1, 3) and must not be
 * NULL: d loss / d irradiance of the projector (mtr_nlos_desc.laser_irradiance), the scene's one emitter.  The scene's tables must
 * fit LDS (every NLOS scene mtr_render runs in the fused organisation does), else MTR_ERR_UNSUPPORTED. */
int  mtr_render_grad(mtr_scene *, const mtr_render_params *params,
                     const float *grad_steady_hw3, const float *grad_transient_hwt3,
                     float *grad_materials, float *grad_emitters);

/* (ABI 16) mtr_render_grad plus the gradients of bitmap texels (the reference: a BitmapTexture's `data` is an ordinary
 * differentiable parameter of TransientADIntegrator.render_backward, common.py:325-409):
 *   grad_texels : device f32 (n_texels, 3)  d loss / d texel of every texture, textures in scene order, row 0 first
 *                                           (mtr_scene_texture_layout gives a texture's first texel); NULL: exactly mtr_render_grad
 * At a vertex on a `diffuse` material (also two-sided) with albedo_texture != 0 the remaining sum divided per channel by the
 * interpolated colour goes to the four taps of the bilinear lookup with the lookup's own weights; taps that wrap onto one texel
 * add up; a channel whose interpolated colour is exactly 0 gets nothing (0, never NaN).  Gradients are per TEXTURE: materials that
 * share a bitmap sum into it.  Only `diffuse` vertices contribute: a bitmap that a roughplastic references as well receives its
 * diffuse materials' part alone and is no parameter (the Python layer gives it no key).  grad_materials of textured materials stay 0.
 * The sums are f64 in one of two tiers (mtr_render_grad_tex_tier): in the workgroups' LDS slabs when all texel words fit beside
 * the material / emitter words (bitwise reproducible), by f64 global atomics otherwise (the f32 result can differ in its last
 * bit from run to run: arrival order).
 * (ABI 20) A NLOS scene (Single or Confocal capture, as mtr_render_grad) has texel gradients as well, in the same two tiers:
 * the bitmap-textured `diffuse` vertices of a term — those whose sampling weight is in its throughput, the vertex the term is
 * emitted at and, under laser sampling, the laser spot — receive as above, the laser spot the term itself over its interpolated
 * colour.  Hidden geometry and relay wall alike; grad_emitters is (1, 3) as for mtr_render_grad.  (Up to ABI 19 a non-NULL
 * grad_texels on a NLOS scene was MTR_ERR_UNSUPPORTED.)  mtr_scene_set_texture stays refused on a NLOS scene: create the scene
 * again (a bitmap enters the scene's classification). */
int  mtr_render_grad_tex(mtr_scene *, const mtr_render_params *params,
                         const float *grad_steady_hw3, const float *grad_transient_hwt3,
                         float *grad_materials, float *grad_emitters, float *grad_texels);
/* (ABI 16) Which tier mtr_render_grad_tex runs for this scene (for tests and tools): a function of the scene alone. */
#define MTR_GRAD_TEX_NONE   0u   /* no bitmap: grad_texels is not touched */
#define MTR_GRAD_TEX_SLAB   1u   /* texel words in the f64 LDS slab, summed by the reduction pass */
#define MTR_GRAD_TEX_GLOBAL 2u   /* f64 global atomics into a device buffer, converted to f32 by a small pass */
int  mtr_render_grad_tex_tier(const mtr_scene *, uint32_t *tier);

/* (ABI 18) Forward-mode derivatives of transient_path: TransientADIntegrator.render_forward (common.py:215-323), the transpose of
 * mtr_render_grad_tex.  For the lanes of `params` the tangent of the DEVELOPED film of the seeded estimator is STORED to
 *   steady_hw3     : device f32 (H, W, 3)     the crop window at the top-left corner, as grad_steady_hw3
 *   transient_hwt3 : device f32 (H, W, T, 3)
 * for the tangents
 *   tan_materials : device f32 (n_materials, 3)  of the reflectance of every plain `diffuse` material (others: not read)
 *   tan_emitters  : device f32 (n_emitters, 3)   of the radiance of every `area` / `angulararea` emitter
 *   tan_texels    : device f32 (n_texels, 3)     of every texel, in the layout of mtr_scene_texture_layout; NULL: none
 * Sampling is detached as in mtr_render_grad, so that  sum g . (J v) = sum (J^T g) . v  holds between the two entry points.  A path
 * is walked once; its log-derivative (f64) gains  da / a  per channel at every `diffuse` vertex whose BSDF factor enters later
 * terms (a channel whose albedo is exactly 0 adds nothing: 0, never NaN), and a term c_unit (.) L_e has the tangent
 * c_unit (.) (L_e (.) D + dL_e), rounded to f32 once and splatted like the term itself.
 * A pixel range renders those pixels' rows and leaves every other pixel of the outputs untouched.  Synchronises the stream.
 * MTR_ERR_UNSUPPORTED (nothing is written): a sample sub-range or a pass of a split render (spp_scale), a NLOS scene, a phasor or
 * exhaustive_scan film, MTR_FLAG_POLARIZED. */
int  mtr_render_fwd(mtr_scene *, const mtr_render_params *params,
                    const float *tan_materials, const float *tan_emitters, const float *tan_texels /* or NULL */,
                    float *steady_hw3, float *transient_hwt3);
/* (ABI 18) Which tier mtr_render_fwd runs (for tests and tools): a function of the scene and its film alone. */
#define MTR_FWD_ROWS   1u   /* a pixel's tangent row lives in LDS and is stored once, developed: no global atomics */
#define MTR_FWD_GLOBAL 2u   /* the row does not fit LDS beside the scene and the stack: f32 global atomics onto zeroed outputs */
int  mtr_render_fwd_tier(const mtr_scene *, const mtr_render_params *params, uint32_t *tier);

/* (ABI 19) mtr_render_grad_tex plus the gradients of the specular tints (TransientADIntegrator.render_backward, common.py:325-409,
 * over `specular_reflectance.value` / `specular_transmittance.value`):
 *   grad_tints : device f32 (n_slots, 3)  d loss / d tint of every slot of mtr_scene_tint_layout; NULL: exactly mtr_render_grad_tex
 * A term is multilinear in the tints (no sampling decision reads one), so  d c / d s = c k_s(c) / s  per channel, k_s(c) the vertices
 * at which s is a factor of c: the continued path carries the tint of the lobe that was SAMPLED at the vertex (reflection when the
 * new ray leaves on the side it arrived on), the vertex's emitter-sampling term (rough lobes) the tint of the lobe EVALUATED for
 * the shadow direction — on a roughdielectric the two can differ at one vertex.  A tint channel that is exactly 0 receives 0.
 * Russian-roulette probabilities are constants.  The sums are f64 in the workgroups' LDS slabs (3 more words per slot), reduced
 * without global atomics.  With grad_texels as well the texel gradients come from a launch of their own.  Everything
 * mtr_render_grad refuses is refused; a non-NULL grad_tints on a NLOS scene is MTR_ERR_UNSUPPORTED with nothing written. */
int  mtr_render_grad_tint(mtr_scene *, const mtr_render_params *params,
                          const float *grad_steady_hw3, const float *grad_transient_hwt3,
                          float *grad_materials, float *grad_emitters, float *grad_texels /* or NULL */, float *grad_tints /* or NULL */);
/* (ABI 19) mtr_render_fwd plus the tangents of the specular tints (common.py:215-323), the transpose of mtr_render_grad_tint:
 *   tan_tints : device f32 (n_slots, 3)  of every slot of mtr_scene_tint_layout; NULL: exactly mtr_render_fwd
 * At a vertex on a tinted material the emitter-sampling term uses the log-derivative plus  ds / s  of the evaluated lobe's tint, the
 * continued path plus that of the sampled lobe's.  Same tiers (mtr_render_fwd_tier), same refusals. */
int  mtr_render_fwd_tint(mtr_scene *, const mtr_render_params *params,
                         const float *tan_materials, const float *tan_emitters, const float *tan_texels /* or NULL */,
                         const float *tan_tints /* or NULL */, float *steady_hw3, float *transient_hwt3);

/* Zero the context's device counters on the context stream (then issue every mtr_render of the render with
 * MTR_FLAG_KEEP_COUNTERS and read the sums once with mtr_counters_read). */
int  mtr_counters_reset(mtr_ctx *);

/* The context's device counters as they stand (summed over every mtr_render since the last one without
 * MTR_FLAG_KEEP_COUNTERS).  The caller has synchronised the streams those renders ran on. */
int  mtr_counters_read(mtr_ctx *, mtr_counters *out /*host*/);

/* TransientHDRFilm.develop / develop_transient_ (transient_hdr_film.py:210-248)
 * and steady.develop (common.py:206,212):  raw (H,W,T,4) -> (H,W,T,3) with the
 * weight division (w==0 -> 1), steady (H,W,4) -> (H,W,3) = sum / count. */
int  mtr_film_develop(mtr_ctx *, const mtr_film_desc *,
                      const float *transient_hwt4, float *transient_hwt3 /*device, may be NULL*/,
                      const float *steady_hw4, float *steady_hw3 /*device, may be NULL*/);

/* The time-bin scatter-add alone: add_transient_data + put_ + accum
 * (transient_hdr_film.py:263-276, transient_image_block.py:131-149) over n
 * splats.  variant 0 = global f32 atomics (the contract form: one atomic per channel wherever the contribution lands).
 * variant 1 = LDS-privatised rows, one workgroup per pixel: input whose `pixel` is non-decreasing (the order of the
 * reference's own lanes, pixel * spp + s) is consumed as it is; any other order is first partitioned by pixel on the
 * device (ABI 10; two scatter passes over 16-byte records — needs 32 bytes of device workspace per contribution for the
 * duration of the call and synchronises the stream once; films whose pixel index and row position do not fit one 32-bit key
 * fall back to variant 0 on the device).  OR MTR_SPLAT_FILM_ZERO into `variant` when the film is all-zero on entry: the row
 * flush then stores whole rows instead of read-modify-write. */
#define MTR_SPLAT_FILM_ZERO 0x100
int  mtr_splat_add(mtr_ctx *, const mtr_splat_soa *, const mtr_film_desc *, int variant,
                   float *transient_hwt4 /*device*/, float *elapsed_ms /*host, may be NULL*/);

/* Backprojection of a NLOS capture into a voxel volume (additive, ABI 24: a new entry point and a new struct; no struct that
 * exists changes and nothing a caller of ABI 24 uses moves, so MTR_ABI_VERSION stays 24).
 *   capture   n_sensor relay-wall points P_s (film order [y][x]), n_laser illuminated points P_l, temporal_bins bins of
 *             bin_width_opl from start_opl.  MTR_CAPTURE_CONFOCAL (n_laser = n_sensor): pairs (s, s), capture (S, T);
 *             MTR_CAPTURE_SINGLE (n_laser = 1): pairs (s, 0), capture (S, T); MTR_CAPTURE_EXHAUSTIVE: every (s, l), capture
 *             (S, L, T) — the exhaustive_scan film's order [y][x][laser_x][laser_y][t] with l = laser_x * Ly + laser_y.
 *   value     voxel centre v = volume_min + (i + 0.5) (volume_max - volume_min) / n; path length
 *             d = |P_s - v| + |v - P_l| + sensor_offset[s] + laser_offset[l] (the sensor -> wall and laser -> wall legs of a
 *             capture rendered with account_first_and_last_bounces, zeros otherwise); u = (d - start_opl) / bin_width_opl;
 *             NEAREST reads bin floor(u) (the bin a rendered contribution of that length was splatted into), LINEAR
 *             interpolates between the bin centres on either side; a tap outside [0, T) contributes 0.  volume (nz, ny, nx)
 *             f32 is STORED: the sum over the voxel's pairs in ascending (s, l) order — a fixed order, the same bits every call.
 * All pointers are device pointers (f32, contiguous).  Runs on the context's stream and does not synchronise it, except to grow
 * the context's workspace when few voxels meet many pairs (mtr_ctx_trim releases it).  MTR_ERR_INVALID before any launch, the
 * volume untouched: a zero size, n_laser != n_sensor on Confocal, n_laser != 1 on Single, bin_width_opl <= 0, a NULL pointer, an
 * empty box (volume_max <= volume_min on an axis), an unknown capture type or interpolation. */
enum { MTR_BACKPROJECT_NEAREST = 0, MTR_BACKPROJECT_LINEAR = 1 };
typedef struct mtr_backproject_desc {
    uint32_t capture_type;          /* MTR_CAPTURE_*                                  */
    uint32_t interpolation;         /* MTR_BACKPROJECT_*                              */
    uint32_t n_sensor, n_laser;     /* S, L                                           */
    uint32_t temporal_bins;         /* T                                              */
    float    start_opl, bin_width_opl;
    float    volume_min[3], volume_max[3];
    uint32_t nx, ny, nz;
    const float *sensor_points;     /* (S, 3) device                                  */
    const float *laser_points;      /* (L, 3) device                                  */
    const float *sensor_offset;     /* (S) device                                     */
    const float *laser_offset;      /* (L) device                                     */
} mtr_backproject_desc;
int  mtr_backproject(mtr_ctx *, const mtr_backproject_desc *, const float *capture_dev, float *volume_dev);

/* The transpose of mtr_backproject: a voxel volume scattered into a NLOS capture — the three-bounce forward model of a hidden
 * volume, and the gradient of a backprojection (additive, ABI 24: a new entry point on mtr_backproject's struct;
 * MTR_ABI_VERSION stays 24).
 *   value     with mtr_backproject's path length d and lookup of (voxel v, row p): NEAREST adds volume[v] to
 *             capture[p, floor(u)], LINEAR adds (1 - w) volume[v] and w volume[v] to the two bins it interpolates between, each
 *             only inside [0, T).  The weight of (v, p, bin) is bit-identical to the one mtr_backproject reads with: with the
 *             same description the two calls are exact transposes, up to the order of their f32 sums.
 *   capture   (rows, T) f32 in mtr_backproject's row order is STORED: every cell is written, a cell nothing reaches is 0.
 *             Voxels that are exactly 0 are skipped (a NaN is not).  The sum of a cell is taken with float atomics in LDS,
 *             whose order is not fixed: the same call gives the same capture to rounding, NOT to bits.
 * All pointers are device pointers (f32, contiguous).  Runs on the context's stream and does not synchronise it, except to grow
 * the context's workspace when few rows meet many voxels (mtr_ctx_trim releases it).  MTR_ERR_INVALID before any launch, the
 * capture untouched: whatever mtr_backproject refuses, more than 2^31 - 1 voxels, rows or (row, 16384-bin window) pairs. */
int  mtr_forward_project(mtr_ctx *, const mtr_backproject_desc *, const float *volume_dev, float *capture_dev);

/* Phasor-field reconstruction: the phasors of a NLOS capture propagated back into a complex voxel volume (additive, ABI 24: a new
 * entry point and a new struct; MTR_ABI_VERSION stays 24).
 *   capture   mtr_backproject's geometry: n_sensor points P_s, n_laser points P_l, the two offset arrays, pairs in ascending (s, l)
 *             order for MTR_CAPTURE_CONFOCAL / _SINGLE / _EXHAUSTIVE.  phasors (n_pairs, n_freq, 2) f32 — the developed tensor of a
 *             phasor_hdr_film viewed as rows: P[p, k] = sum of value * exp(-i 2 pi f_k (opl - start_opl)).
 *   value     d = |P_s - v| + |v - P_l| + sensor_offset[s] + laser_offset[l] for the voxel centre v, tau = d - start_opl;
 *             V(v) = sum over p of [tau_min <= tau <= tau_max] sum over k of (w_k P[p, k]) exp(+i 2 pi f_k tau), pairs ascending
 *             and k ascending inside a pair, one complex f32 accumulator per voxel.  volume (nz, ny, nx, 2) f32 is STORED; the same
 *             call gives the same bits.  A NaN or infinite tau fails the window test: with the bounds -FLT_MAX .. FLT_MAX a voxel
 *             so far away that d overflows contributes exactly 0.
 *   exp       freq_step == 0: every exp(+i 2 pi f_k tau) is the conjugate of the film's own term (its range reduction and
 *             polynomials).  freq_step > 0 is the caller's promise that frequencies[k] = frequencies[0] + k freq_step: the term is
 *             evaluated so at every 16th k and rotated by exp(+i 2 pi freq_step tau) in between.
 *   weights   NULL means ones; otherwise w_k P is formed first.
 * All pointers are device pointers (f32, contiguous; phasors and volume 8-byte aligned, or MTR_ERR_INVALID).  Runs on the
 * context's stream and does not synchronise it, except to grow the context's workspace (weights given, or few voxels meeting many pairs; mtr_ctx_trim releases it).  MTR_ERR_INVALID before any
 * launch, the volume untouched: a zero size (n_freq included), a NULL pointer other than weights, n_laser != n_sensor on Confocal,
 * n_laser != 1 on Single, an empty box, a start_opl that is not finite, tau_min > tau_max or either a NaN, freq_step < 0 or a NaN,
 * an unknown capture type. */
typedef struct mtr_phasor_backproject_desc {
    uint32_t capture_type;          /* MTR_CAPTURE_*                                  */
    uint32_t n_sensor, n_laser;     /* S, L                                           */
    uint32_t n_freq;                /* F                                              */
    float    start_opl, freq_step;
    float    tau_min, tau_max;      /* the window, in path length from start_opl      */
    float    volume_min[3], volume_max[3];
    uint32_t nx, ny, nz;
    const float *sensor_points;     /* (S, 3) device                                  */
    const float *laser_points;      /* (L, 3) device                                  */
    const float *sensor_offset;     /* (S) device                                     */
    const float *laser_offset;      /* (L) device                                     */
    const float *frequencies;       /* (F) device                                     */
    const float *weights;           /* (F) device, or NULL                            */
} mtr_phasor_backproject_desc;
int  mtr_phasor_backproject(mtr_ctx *, const mtr_phasor_backproject_desc *, const float *phasors_dev, float *volume_dev);

/* The conjugate transpose of mtr_phasor_backproject: a complex voxel volume turned into the phasors it would produce — the forward
 * model of a phasor-field reconstruction, and the gradient of one (additive, ABI 24: a new entry point on
 * mtr_phasor_backproject's struct; MTR_ABI_VERSION stays 24).
 *   value     with mtr_phasor_backproject's tau, window test M(v, p) and factor z(v, p, k) of (voxel v, row p, frequency k):
 *             Q[p, k] = w_k sum over v of M(v, p) U(v) conj(z(v, p, k)).  z is evaluated by the same functions, at the same
 *             anchors (every 16th k of a uniform table, rotations in between): with the same description the two calls are exact
 *             conjugate transposes, up to the order of their f32 sums.  For a real non-negative U this is the film's convention,
 *             sum of value * exp(-i 2 pi f_k (opl - start_opl)): the phasors of a volume of scatterers, without cosines and 1/r^2.
 *   volume    (nz, ny, nx, 2) f32, read.  A voxel outside the window of a row does not reach it, whatever it holds.
 *   phasors   (n_pairs, n_freq, 2) f32 in mtr_phasor_backproject's row order is STORED: every element is written, an element
 *             nothing reaches is 0.  The sums have a fixed order (no float atomics): the same call gives the same bits.
 *   weights   NULL means ones; otherwise w_k multiplies the finished sum, two f32 products per element.
 * All pointers are device pointers (f32, contiguous; volume and phasors 8-byte aligned, or MTR_ERR_INVALID).  Runs on the
 * context's stream and does not synchronise it, except to grow the context's workspace when few rows meet many voxels
 * (mtr_ctx_trim releases it).  MTR_ERR_INVALID before any launch, the phasors untouched: whatever mtr_phasor_backproject
 * refuses, more than 2^31 - 1 voxels, rows or (row, block of 16 frequencies) pairs. */
int  mtr_phasor_forward_project(mtr_ctx *, const mtr_phasor_backproject_desc *, const float *volume_dev, float *phasors_dev);

/* f-k migration of a confocal capture of a planar wall (Lindell et al. 2019): the three passes around the caller's two FFTs
 * (additive, ABI 24: three new entry points and a new struct; MTR_ABI_VERSION stays 24).  With T' = depth_bins, q = bin_factor:
 *   mtr_fk_prepare  capture (H, W, T) f32 and shift (H, W) int32 -> padded (2H, 2W, 2T') f32, EVERY element stored (no memset
 *                   is needed before it).  In the low corner padded[y, x, k] = sqrt(max(S, 0)) ((k + 1/2) / T') with
 *                   S = sum over j = kq .. kq + q - 1 of capture[y, x, j - shift[y, x]], terms outside [0, T) dropped, added in
 *                   f32 in increasing j; zero elsewhere.
 *   mtr_fk_stolt    spectrum (2H, 2W, T' + 1) complex64 — the real-to-complex transform of `padded` over its three axes, depth
 *                   last — -> resampled (2H, 2W, 2T') complex64, EVERY element stored.  With signed FFT indices my in [-H, H),
 *                   mx in [-W, W), mz in [-T', T') and ky = my / H, kx = mx / W, kz = mz / T': for kz > 0,
 *                   k' = sqrt((ax kx)^2 + (ay ky)^2 + kz^2), p = k' T', i0 = floor(p), w = p - i0 and
 *                   resampled = ((1 - w) spectrum[iy, ix, i0] + w spectrum[iy, ix, i0 + 1]) (kz / k') when i0 + 1 <= T';
 *                   zero otherwise, and for kz <= 0.  ax, ay: the depth spacing over the scan spacing along x and y.
 *   mtr_fk_finish   field (2H, 2W, 2T') complex64 — the inverse complex transform of `resampled` — -> volume (nz, H, W) f32,
 *                   volume[iz, iy, ix] = |field[iy, ix, z_begin + iz]|^2.
 * f32 arithmetic in a fixed order and no sums across threads: the same call gives the same bits.  All pointers are device
 * pointers (contiguous, 16-byte aligned, or MTR_ERR_INVALID).  Each runs on the context's stream and does not synchronise it.
 * MTR_ERR_INVALID before any launch, the output untouched: a NULL pointer, height or width below 2 or above 32767, a zero size,
 * bin_factor 0, z_begin + nz > depth_bins, ax or ay not positive and finite. */
typedef struct mtr_fk_desc {
    uint32_t height, width;         /* H, W: the scan grid                            */
    uint32_t temporal_bins;         /* T                                              */
    uint32_t bin_factor;            /* q                                              */
    uint32_t depth_bins;            /* T'                                             */
    uint32_t z_begin, nz;           /* the depth rows mtr_fk_finish keeps             */
    float    ax, ay;
} mtr_fk_desc;
int  mtr_fk_prepare(mtr_ctx *, const mtr_fk_desc *, const float *capture_dev, const int32_t *shift_dev, float *padded_dev);
int  mtr_fk_stolt(mtr_ctx *, const mtr_fk_desc *, const float *spectrum_dev, float *resampled_dev);
int  mtr_fk_finish(mtr_ctx *, const mtr_fk_desc *, const float *field_dev, float *volume_dev);

/* Release the device workspaces the context keeps between calls (ABI 10: the partition workspace of mtr_splat_add on
 * unsorted input — 32 bytes per contribution; a workspace above 256 MiB is released by the call itself, a smaller one
 * stays with the context; ABI 24: the slabs' rows of MTR_MODE_SAMPLES, under the same rule).  Synchronises the context's stream. */
int  mtr_ctx_trim(mtr_ctx *);

/* Debug/test aid: per-lane splat log of one render (records of 8 x u32:
 * lane, depth|kind<<16, pixel, bin, r,g,b bits, opl bits), capacity in records.
 * Pass NULL to disable. The count is written to *n_records_device (u64). */
int  mtr_debug_set_splat_log(mtr_scene *, uint32_t *log_device, uint64_t capacity, uint64_t *n_records_device);

#ifdef __cplusplus
}
#endif
#endif /* MITRANSIENT_AMD_H */
