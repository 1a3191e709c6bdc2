"""Scenes with mitsuba's analytic `sphere`, shared by tests/test_sphere.py (host build) and tests/test_gpu_sphere.py (MI355X)."""
import math

import numpy as np

import delta_cases as DC
import delta_quadrature as DQ

L_BALL = (2.0, 3.0, 4.0)
RHO = (0.8, 0.5, 0.2)


def T():
    return DC._T()()


def integ(max_depth, **kw):
    return dict({"type": "transient_path", "max_depth": max_depth, "rr_depth": 100}, **kw)


# ---- 1. seeing a ball: an emitting unit sphere at the origin, the camera 4 away; a 6 x 4 window across the silhouette, one inside it
SEEN_C, SEEN_R = (0.0, 0.0, 0.0), 1.0
WINDOW_EDGE = {"width": 1024, "height": 768, "crop_width": 6, "crop_height": 4, "crop_offset_x": 873, "crop_offset_y": 382}
WINDOW_IN = dict(WINDOW_EDGE, crop_offset_x=600, crop_offset_y=300)


def seen_scene(window, spp=64, film=None, flip=False, **kw):
    """flip: the camera sits inside a `flip_normals` sphere of radius 5 instead and reads the far root"""
    f = dict(window, **(film or {}))
    ball = {"type": "sphere", "emitter": {"type": "area", "radiance": DC.rgb(*L_BALL)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}}
    if flip:
        ball.update(radius=5.0, center=[0.5, 0.0, 0.25], flip_normals=True)
    return DC._mi().load_dict({"type": "scene", "integrator": integ(1, **kw),
                               "sensor": DC._sensor(f, spp, origin=(0.0, -4.0, 0.0), target=(0.0, 0.0, 0.0)), "ball": ball})


# ---- 2. a sphere light over the delta-emitter tests' floor
def light_centre(D, tilt=25.0, azimuth=80.0):
    x0 = DC.window_centre()
    t, a = math.radians(tilt), math.radians(azimuth)
    return x0 + D * np.array([math.sin(t) * math.cos(a), math.sin(t) * math.sin(a), math.cos(t)])


def light_scene(ratio, D=2.0, film=None, spp=64, max_depth=2, **kw):
    """a diffuse floor and a sphere light of radius ratio * D, D from the floor point behind the window's centre: (scene, c, r)"""
    c, r = light_centre(D), ratio * D
    d = DC.floor_dict({"type": "sphere", "center": [float(v) for v in c], "radius": r,
                       "emitter": {"type": "area", "radiance": DC.rgb(*L_BALL)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}},
                      film, max_depth=max_depth, spp=spp, **kw)
    return DC._mi().load_dict(d), c, r


# ---- 3. a furnace: a `flip_normals` emitting sphere around the camera and a diffuse ball
def furnace_scene(max_depth, spp=256, res=(8, 6), film=None):
    f = dict({"width": res[0], "height": res[1]}, **(film or {}))
    return DC._mi().load_dict({
        "type": "scene", "integrator": integ(max_depth),
        "sensor": DC._sensor(f, spp, origin=(0.0, -3.0, 0.0), target=(0.0, 0.0, 0.0), fov=60.0),
        "room": {"type": "sphere", "radius": 5.0, "center": [0.3, 0.2, -0.1], "flip_normals": True,
                 "emitter": {"type": "area", "radiance": DC.rgb(*L_BALL)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}},
        "ball": {"type": "sphere", "radius": 1.0, "bsdf": {"type": "diffuse", "reflectance": DC.rgb(*RHO)}}})


FURNACE_ROOM = ((0.3, 0.2, -0.1), 5.0)

# ---- 4. a ball lens: glass ball between the camera and an emitting rectangle that faces it
LENS_R, LENS_ETA = 0.5, 1.5
LENS_PLANE = DQ.Plane((0.0, 3.0, 0.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.0, 0.0, 0.0))        # normal -y


def lens_scene(film=None, spp=256):
    f = dict({"width": 33, "height": 33, "crop_width": 1, "crop_height": 1, "crop_offset_x": 16, "crop_offset_y": 16}, **(film or {}))
    return DC._mi().load_dict({
        "type": "scene", "integrator": integ(3),
        "sensor": DC._sensor(f, spp, origin=(0.0, -4.0, 0.0), target=(0.0, 0.0, 0.0), fov=2.0),
        "lens": {"type": "sphere", "radius": LENS_R, "bsdf": {"type": "dielectric", "int_ior": LENS_ETA, "ext_ior": 1.0}},
        # the rectangle's x -> x, its y -> z, its normal +z -> -y
        "panel": {"type": "rectangle", "to_world": DC._T()([[2, 0, 0, 0], [0, 0, -2, 3], [0, 2, 0, 0], [0, 0, 0, 1]]),
                  "emitter": {"type": "area", "radiance": DC.rgb(1.0, 1.0, 1.0)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}}})


# ---- 5. a hidden ball behind the relay wall
HIDDEN = {"type": "sphere", "center": [0, 0, 1], "radius": 0.35}


def hidden_scene(hg=True, spp=256, **kw):
    from conftest import make_nlos
    args = dict(sx=4, sy=4, capture="single", hidden=dict(HIDDEN), spp=spp, max_depth=3, rr_depth=100,
                nlos_hidden_geometry_sampling=hg)
    args.update(kw)
    return make_nlos(**args)


# ---- 6. the frame: an anisotropic rough conductor
def aniso_scene(au, av, turn=0.0, spp=64, res=(12, 9)):
    ball = {"type": "sphere", "radius": 0.6, "center": [0.0, 0.0, 0.6], "to_world": T().rotate([0, 0, 1], turn),
            "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha_u": au, "alpha_v": av,
                     "eta": DC.rgb(0.2, 0.9, 1.1), "k": DC.rgb(3.9, 2.4, 2.2)}}
    return DC._mi().load_dict({
        "type": "scene", "integrator": integ(2),
        "sensor": DC._sensor({"width": res[0], "height": res[1]}, spp, origin=(0.0, -3.0, 1.6), target=(0.0, 0.0, 0.6), fov=30.0),
        "ball": ball,
        "lamp": {"type": "rectangle", "to_world": T().translate([0.4, -0.3, 2.5]).rotate([1, 0, 0], 180.0).scale(0.5),
                 "emitter": {"type": "area", "radiance": DC.rgb(6.0, 6.0, 6.0)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}}})


# ---- 7 / GPU: balls in the Cornell box's room
def room_dict(balls=("diffuse", "glass", "light"), res=(8, 6), bins=16, spp=5, max_depth=4, boxes=False, rect_light=True, **kw):
    d = DC.cornell_dict(area=rect_light, point=False, spot=False, boxes=boxes, res=res, spp=spp, max_depth=max_depth, **kw)
    d["sensor"]["film"].update(temporal_bins=bins, bin_width_opl=8.0 / bins)
    add_balls(d, balls)
    return d


def add_balls(d, balls):
    if "diffuse" in balls:
        d["ball"] = {"type": "sphere", "center": [-0.45, -0.65, -0.2], "radius": 0.35, "bsdf": {"type": "diffuse", "reflectance": DC.rgb(0.3, 0.6, 0.8)}}
    if "glass" in balls:
        d["glass"] = {"type": "sphere", "center": [0.45, -0.7, 0.3], "radius": 0.3, "bsdf": {"type": "dielectric", "int_ior": 1.5}}
    if "light" in balls:
        d["bulb"] = {"type": "sphere", "center": [0.1, 0.55, -0.3], "radius": 0.12,
                     "emitter": {"type": "area", "radiance": DC.rgb(9.0, 7.0, 4.0)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}}
    if "metal" in balls:
        d["metal"] = {"type": "sphere", "center": [0.0, -0.6, 0.0], "radius": 0.4,
                      "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": 0.2, "eta": 0.47, "k": 2.4}}
    return d


def room_scene(**kw):
    return DC._mi().load_dict(room_dict(**kw))
