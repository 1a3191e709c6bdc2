"""The scenes whose classification (mtr_scene_host.cpp classify_scene: trait word, extended shading, polarized form) is pinned:
test_scene_class.py holds the words as literals and checks the host build against them, test_gpu_scene_class.py checks
that the library reports the same word.  Every builder takes a pathlib directory for the files it writes."""
import os

from conftest import ROOT, make_cornell, make_nlos, make_nlos_z


def _mi():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    return mi


def _cornell_dict(width=32, height=32, bins=64):
    import mitransient_amd as mitr
    _mi()
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=width, height=height, temporal_bins=bins, start_opl=3.5, bin_width_opl=6.0 / bins)
    return d


def _obj(tmp, name, text):
    path = os.path.join(str(tmp), name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def cornell_c3(tmp):
    import mitransient_amd as mitr
    return _mi().load_dict(mitr.cornell_box())


def mirror_box(tmp):
    """tools/mirror_box.py: the small box a conductor — a flat top level under the general shading code"""
    d = _cornell_dict()
    d["mirror"] = {"type": "conductor", "eta": {"type": "rgb", "value": [1.65, 0.88, 0.52]}, "k": {"type": "rgb", "value": [9.2, 6.3, 4.8]}}
    d["small-box"]["bsdf"] = {"type": "ref", "id": "mirror"}
    return _mi().load_dict(d)


def two_emitters(tmp):
    from mitransient_amd.transform import ScalarTransform4f as T
    d = _cornell_dict()
    d["far-light"] = {"type": "rectangle", "to_world": T().translate([50.0, 50.0, 50.0]).scale([0.01, 0.01, 0.01]),
                      "bsdf": {"type": "ref", "id": "white"},
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [0.0, 0.0, 0.0]}}}
    return _mi().load_dict(d)


def angular(tmp):
    import angular_cases
    return angular_cases.cornell()


def mesh_boxes(tmp):
    """tools/size_sweep.py: both boxes as 2 x 2-tessellated meshes of 48 triangles — a third level, no flat top"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import size_sweep
    saved, size_sweep.TMP = size_sweep.TMP, str(tmp)
    try:
        return _mi().load_dict(size_sweep.cornell(2, 48, 48, 96))
    finally:
        size_sweep.TMP = saved


def top_level_triangles(tmp):
    """a two-triangle mesh beside rectangles and a box node: triangle leaves at the top level (kTrFlatLeaves)"""
    d = _cornell_dict()
    d.pop("small-box")
    kite = _obj(tmp, "kite.obj", "v 0.2 -0.9 0.6\nv 0.7 -0.9 0.2\nv 0.5 -0.2 0.4\nv 0.1 -0.3 0.1\nf 1 2 3\nf 1 3 4\n")
    d["kite"] = {"type": "obj", "filename": kite, "face_normals": True,
                 "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.4, 0.5, 0.6]}}}}
    return _mi().load_dict(d)


def far_triangle(tmp):
    """one loose triangle behind the back wall: its leaf is not a pair, the scene is walked through its tree"""
    d = _cornell_dict()
    tri = _obj(tmp, "far_triangle.obj", "v -0.1 -0.1 -30\nv 0.1 -0.1 -30\nv 0 0.1 -30\nf 1 2 3\n")
    d["far-triangle"] = {"type": "obj", "filename": tri, "face_normals": True, "bsdf": {"type": "ref", "id": "white"}}
    return _mi().load_dict(d)


def five_cubes(tmp):
    """one box node more than the flat top level takes (kFlatMaxBoxes)"""
    from mitransient_amd.transform import ScalarTransform4f as T
    d = _cornell_dict()
    for i in range(3):
        d[f"extra-box-{i}"] = {"type": "cube", "to_world": T().translate([-0.6 + 0.6 * i, 0.5, -0.6]).rotate([0, 1, 0], 15.0 * i).scale(0.12),
                               "bsdf": {"type": "ref", "id": "white"}}
    return _mi().load_dict(d)


def _rough(distribution):
    def build(tmp):
        from test_rough_bsdf import _rough_cornell
        return _mi().load_dict(_rough_cornell(distribution))
    return build


def _textured(bsdf_type):
    def build(tmp):
        from test_textures import textured_scene
        return textured_scene(tmp, bsdf_type, width=24, height=24)
    return build


def _staircase(**kw):
    def build(tmp):
        from mitransient_amd.scenes import staircase
        return staircase(width=45, height=80, spp=4, **kw)
    return build


def grey_cornell_dict():
    d = _cornell_dict()
    for name, v in zip(("white", "red", "green"), (0.7, 0.4, 0.5)):
        d[name]["reflectance"] = {"type": "rgb", "value": [v, v, v]}
    d["light"]["emitter"]["radiance"] = {"type": "rgb", "value": [12.0, 12.0, 12.0]}
    return d


def grey_cornell(tmp, colour=None):
    """the Cornell box with three equal channels in every reflectance and in the light; colour: then the red wall takes it through
    params.update() (mtr_scene_set_colors on a scene that is on the device already)"""
    scene = _mi().load_dict(grey_cornell_dict())
    if colour is not None:
        recolour(scene, colour)
    return scene


def recolour(scene, colour):
    p = _mi().traverse(scene)
    p["red.reflectance.value"] = list(colour)
    p.update()


CASES = {
    "cornell-config1": lambda tmp: make_cornell(),
    "cornell-config2": lambda tmp: make_cornell(width=512, height=512, bins=1024),
    "cornell-config3": cornell_c3,
    "nlos-z-config4": lambda tmp: make_nlos_z(tmp),
    "nlos-grey-quad": lambda tmp: make_nlos(),
    "nlos-coloured-laser": lambda tmp: make_nlos(laser_rgb=(1.0, 0.6, 0.3)),
    "nlos-coloured-hidden": lambda tmp: make_nlos(hidden_bsdf={"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.9, 0.5, 0.2]}}),
    "staircase-config5": _staircase(),
    "staircase-rough": _staircase(materials="rough"),
    "staircase-rough-normals": _staircase(materials="rough", vertex_normals=True),
    "staircase-rough-normals-textures": _staircase(materials="rough", vertex_normals=True, textures=True),
    "mirror-box": mirror_box,
    "cornell-angulararea": angular,
    "cornell-two-emitters": two_emitters,
    "cornell-mesh-boxes": mesh_boxes,
    "top-level-triangles": top_level_triangles,
    "far-triangle": far_triangle,
    "five-cubes": five_cubes,
    "rough-ggx": _rough("ggx"),
    "rough-beckmann-by-default": _rough(None),
    "rough-anisotropic": _rough("aniso"),
    "rough-roughdielectric": _rough("glass"),
    "rough-plastic-thindielectric": _rough("plastic"),
    "textured-diffuse": _textured("diffuse"),
    "textured-roughplastic": _textured("roughplastic"),
    "grey-cornell": grey_cornell,
    "grey-cornell-one-wall-coloured": lambda tmp: grey_cornell(tmp, (0.6, 0.2, 0.1)),
}


def host_class(host_harness, scene):
    """(traits, needs the extended shading code, has a polarized form, [n_quads, n_boxes, node0, prim_mask, wide_levels]) of the
    host build"""
    import ctypes as C
    d = scene.data().desc()
    t, ext, pol = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    flat = (C.c_uint32 * 5)()
    assert host_harness.hh_scene_class(C.byref(d), C.byref(t), C.byref(ext), C.byref(pol), flat) == 0
    return int(t.value), int(ext.value), int(pol.value), [int(x) for x in flat]


def planned_mode(scene, spp=8):
    """the organisation MTR_MODE_AUTO resolves to (mtr_render_plan): "fused" | "wavefront" """
    import ctypes as C
    from mitransient_amd import _cabi
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    sensor = scene.sensors()[0]
    params = scene.integrator().render_params(sensor.film(), 0, spp)
    params.mode = _cabi.MTR_MODE_AUTO
    mode = C.c_uint32(0)
    ctx.check(ctx.lib.mtr_render_plan(scene.gpu_handle(ctx, sensor), C.byref(params), C.byref(mode), None), "mtr_render_plan")
    return {_cabi.MTR_MODE_FUSED: "fused", _cabi.MTR_MODE_WAVEFRONT: "wavefront"}[int(mode.value)]
