"""Scenes with an `angulararea` emitter (mitransient/emitters/angulararea.py) and the comparison against the CPU oracle's
restatement of it (oracle/mtr_oracle.c, f64 falloff), shared by tests/test_angular_oracle.py (the host build of mtr_core.h) and
tests/test_gpu_angular_emitter.py (k_fused and the k_wf_* kernels).

The bar: rel-L2 <= 1e-5 on the transient and the steady film, and every counter equal up to the oracle's near total — the number
of falloff evaluations that sat at a threshold (oracle.render(..., near=True)), where an f32 falloff may take the other side of
`falloff > 0` and issue (or not) one shadow ray and one splat.  Pixels with a near evaluation are left out of the image comparison.
"""
import copy
import os

import numpy as np

from angular_quadrature import SCENES
from conftest import rel_l2

TOL = 1e-5
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")


def _mi():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    return mi


def _angular(cutoff=None, beam=None, radiance=None):
    e = {"type": "angulararea"}
    if cutoff is not None:
        e["cutoff_angle"] = cutoff
    if beam is not None:
        e["beam_width"] = beam
    if radiance is not None:
        e["radiance"] = radiance
    return e


def notebook(view=1, res=24, spp=16, **integ):
    """the tutorial's angular_1light.xml (an obj light with vertex normals over an obj floor); view 2: the notebook's cell 6"""
    from angular_quadrature import load_notebook_scene
    scene = load_notebook_scene("angular", view, res=res, spp=spp)
    for k, v in integ.items():
        setattr(scene.integrator(), k, v)
    return scene


def cornell(cutoff=60, beam=30, res=24, bins=64, emitter=None, shape="rectangle", flip=False, second_area_light=False,
            rough_floor=False, film=None, **integ):
    """cornell_box() with its luminaire as an angulararea emitter.  shape="cube": a small cube below the ceiling instead (a mesh
    emitter of six faces); flip: the rectangle turned to face the ceiling and flipped back (`flip_normals`)."""
    import mitransient_amd as mitr
    from mitransient_amd.transform import ScalarTransform4f as T
    mi = _mi()
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=res, height=res, temporal_bins=bins, start_opl=3.0, bin_width_opl=8.0 / bins)
    d["sensor"]["film"].update(film or {})
    d["integrator"].update(integ)
    rad = d["light"]["emitter"].get("radiance", 1.0)
    d["light"]["emitter"] = emitter if emitter is not None else _angular(cutoff, beam, rad)
    if shape == "cube":
        d["light"].update(type="cube", to_world=T().translate([0.0, 0.6, 0.0]).scale(0.12))
    if flip:
        d["light"]["to_world"] = T().translate([0, 0.99, 0.01]).rotate([1, 0, 0], -90).scale([0.23, 0.19, 0.19])
        d["light"]["flip_normals"] = True
    if second_area_light:
        d["light2"] = {"type": "rectangle", "to_world": T().translate([-0.98, 0.0, 0.3]).rotate([0, 1, 0], 90).scale(0.15),
                       "bsdf": {"type": "ref", "id": "white"},
                       "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [4.0, 9.0, 2.0]}}}
    if rough_floor:
        d["floor"]["bsdf"] = {"type": "roughconductor", "distribution": "ggx", "alpha": 0.25,
                              "eta": [0.2, 0.9, 1.1], "k": [3.9, 2.4, 2.2]}
    return mi.load_dict(d)


def write_bent_light(path, normals=True, n=4):
    """the tutorial light's rectangle (y = 10, x in [-3, 3], z in [-1, 1], facing -y) as an n x n grid; normals=True: vertex
    normals bent outwards by up to ~27 degrees (shading normals that differ from the face normal), False: no `vn` at all"""
    lines = []
    xs, zs = np.linspace(-3, 3, n + 1), np.linspace(-1, 1, n + 1)
    for z in zs:
        for x in xs:
            lines.append(f"v {x:.6f} 10.0 {z:.6f}")
    if normals:
        for z in zs:
            for x in xs:
                v = np.array([0.12 * x, -1.0, 0.3 * z])
                v /= np.linalg.norm(v)
                lines.append(f"vn {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}")
    for j in range(n):
        for i in range(n):
            a, b = j * (n + 1) + i + 1, j * (n + 1) + i + 2
            c, e = a + n + 1, b + n + 1
            for tri in ((a, e, c), (a, b, e)):         # wound so that the face normal is -y
                lines.append("f " + " ".join(f"{k}//{k}" if normals else f"{k}" for k in tri))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return str(path)


def mesh_light(obj_path, res=24, spp=16, cutoff=35, beam=20, **integ):
    """the tutorial scene's camera and floor, lit by the obj at obj_path as an angulararea emitter"""
    from mitransient_amd.transform import ScalarTransform4f as T
    mi = _mi()
    d = {
        "type": "scene",
        "integrator": dict({"type": "transient_path", "max_depth": 8}, **integ),
        "sensor": {"type": "perspective", "fov_axis": "smaller", "near_clip": 10.0, "far_clip": 2800.0, "fov": 39.3077,
                   "to_world": T().look_at([30, 8, 0], [-10, 0, 0], [0, 1, 0]),
                   "sampler": {"type": "independent", "sample_count": spp},
                   "film": {"type": "transient_hdr_film", "width": res, "height": res, "temporal_bins": 200, "start_opl": 0.0,
                            "bin_width_opl": 0.5, "rfilter": {"type": "box"}}},
        "gray": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.85, 0.85, 0.85]}},
        "black": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.0, 0.0, 0.0]}},
        "light": {"type": "obj", "filename": obj_path, "bsdf": {"type": "ref", "id": "black"},
                  "emitter": _angular(cutoff, beam, {"type": "rgb", "value": [18.387, 10.9873, 2.75357]})},
        "floor": {"type": "obj", "filename": os.path.join(SCENES, "meshes", "floor50.obj"), "bsdf": {"type": "ref", "id": "gray"}},
    }
    return mi.load_dict(d)


def staircase(res=24, spp=8):
    """staircase_like(tiles=6) (a scene walked in HBM) lit by an angulararea cube hanging from the ceiling"""
    from mitransient_amd.scenes import staircase_like
    from mitransient_amd.transform import ScalarTransform4f as T
    mi = _mi()
    d = staircase_like(n_steps=12, balusters=2, tiles=6, width=res, height=res, temporal_bins=64, spp=spp)
    d["light"] = {"type": "cube", "to_world": T().translate([0.0, 3.6, 0.5]).scale(0.25), "bsdf": {"type": "ref", "id": "wall"},
                  "emitter": _angular(40, 15, {"type": "rgb", "value": [30.0, 30.0, 30.0]})}
    return mi.load_dict(d)


def phasor(res=12, **film):
    """tests/test_phasor.py::phasor_cornell with the luminaire as an angulararea emitter (60 / 30 degrees); mono variant"""
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_mono")
    d = mitr.cornell_box()
    fd = {"type": "phasor_hdr_film", "width": res, "height": res, "wl_mean": 2.0, "wl_sigma": 1.0, "temporal_bins": 400,
          "bin_width_opl": 0.05, "start_opl": 3.0, "rfilter": {"type": "box"}}
    fd.update(film)
    d["sensor"]["film"] = fd
    d["light"]["emitter"] = _angular(60, 30, d["light"]["emitter"].get("radiance", 1.0))
    return mi.load_dict(d)


def as_area(sd):
    """a copy of the flattened scene with every emitter's `angular` forced to 0: what a render that ignored it would see"""
    sd2 = copy.copy(sd)
    sd2.emitters = type(sd.emitters).from_buffer_copy(sd.emitters)
    for i in range(sd2.n_emitters):
        sd2.emitters[i].angular = 0
    return sd2


def oracle_render(scene, seed, spp, sd=None, **p):
    """the oracle's film (developed), raw counters, near map (H, W) and near total"""
    from oracle import oracle as _o
    sd = sd if sd is not None else scene.data()
    params = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp, **p)
    t4, s4, c, (near, n_near) = _o.render(sd, params, use_bvh=True, near=True)
    t3, s3 = _o.develop(sd.film, t4, s4)
    return np.array(s3), np.array(t3), c, near, n_near


def _masked(a, keep):
    a = np.asarray(a, np.float64)
    k = keep.reshape(keep.shape + (1,) * (a.ndim - 2))
    return np.where(k, a, 0.0)


def assert_matches_oracle(s, t, c, ref, what=""):
    """(s, t, c): a steady (H', W', C) / transient (H, W, T, C) / counters render of the product; ref: oracle_render(...).  The
    near pixels are left out of the image comparison; each counter may differ by at most the near total.  Returns the near total."""
    rs, rt, rc, near, n_near = ref
    H, W = near.shape
    keep = ~near
    assert near.mean() <= 0.05, (what, int(near.sum()))
    assert np.count_nonzero(rt) > 20, what
    e_t = rel_l2(_masked(t, keep), _masked(rt, keep))
    hs, ws = rs.shape[:2]                                   # the steady image holds only the crop window
    e_s = rel_l2(_masked(s, keep[:hs, :ws]), _masked(rs, keep[:hs, :ws]))
    assert e_t <= TOL and e_s <= TOL, (what, e_t, e_s, n_near)
    for k in COUNTERS:
        assert abs(int(c[k]) - int(rc[k])) <= n_near, (what, k, c[k], rc[k], n_near)
    return n_near


def assert_cone_clips(scene, seed=0, spp=8, wide=False):
    """the cone clips the image: with max_depth 2 (emission and one emitter-sampling bounce), some pixels are lit, and some that the
    same emitter lights as a plain `area` light stay dark.  wide (cutoff >= 90 degrees: every front direction is in the cone):
    instead, the falloff and the extra 1 / dist^2 make the render differ from the area light's."""
    from oracle import oracle as _o
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)
    p.max_depth = 2
    _, ang, _ = _o.render(sd, p, use_bvh=True)
    _, area, _ = _o.render(as_area(sd), p, use_bvh=True)
    lit_ang = ang[..., :3].sum(-1) > 0
    lit_area = area[..., :3].sum(-1) > 0
    assert lit_ang.sum() > 0
    if wide:
        assert rel_l2(ang[..., :3], area[..., :3]) > 1e-2
    else:
        assert (lit_area & ~lit_ang).sum() > 0


def hh_render_developed(host_harness, scene, seed, spp, **p):
    from conftest import hh_render
    from oracle import oracle as _o
    sd = scene.data()
    params = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp, **p)
    t4, s4, c = hh_render(host_harness, sd, params)
    t3, s3 = _o.develop(sd.film, t4, s4)
    return np.array(s3), np.array(t3), c


# (id, builder(tmp_path) -> scene, seed, spp, wide): the scenes every comparison runs on
def _nb_bent(tmp, **kw):
    return mesh_light(write_bent_light(os.path.join(tmp, "bent.obj"), normals=True), **kw)


def _nb_flat(tmp, **kw):
    return mesh_light(write_bent_light(os.path.join(tmp, "flat.obj"), normals=False), **kw)


SCENE_CASES = {
    "notebook_view1": (lambda tmp: notebook(1), 3, 16, False),
    "notebook_view2": (lambda tmp: notebook(2), 3, 16, False),
    "obj_bent_vertex_normals": (lambda tmp: _nb_bent(tmp), 4, 16, False),
    "obj_without_vertex_normals": (lambda tmp: _nb_flat(tmp), 4, 16, False),
    "cornell_60_30": (lambda tmp: cornell(60, 30), 1, 16, False),
    "cornell_flip_normals": (lambda tmp: cornell(60, 30, flip=True), 1, 16, False),
    "step_35_35": (lambda tmp: cornell(35, 35), 5, 16, False),
    "defaults_10": (lambda tmp: cornell(emitter=_angular(radiance={"type": "rgb", "value": [18.0, 14.0, 7.0]})), 6, 16, False),
    "wide_90_0": (lambda tmp: cornell(90, 0), 7, 16, True),
    "wide_180_120": (lambda tmp: cornell(180, 120), 7, 16, True),
    "narrow_2_1": (lambda tmp: cornell(2, 1, res=32), 8, 32, False),
    "cube_40_20": (lambda tmp: cornell(40, 20, shape="cube"), 9, 16, False),
    "area_and_angular": (lambda tmp: cornell(60, 30, second_area_light=True), 2, 16, False),
    "ggx_rough_receiver": (lambda tmp: cornell(45, 25, rough_floor=True), 10, 16, False),
    "max_depth_1": (lambda tmp: cornell(90, 0, res=48, max_depth=1), 11, 16, True),     # the luminaire seen at ~75 degrees
    "max_depth_2": (lambda tmp: cornell(45, 25, max_depth=2), 11, 16, False),
    "discard_direct_light": (lambda tmp: cornell(45, 25, discard_direct_light=True), 12, 16, False),
    "camera_unwarp": (lambda tmp: cornell(45, 25, camera_unwarp=True, film={"start_opl": 0.0}), 13, 16, False),
}
