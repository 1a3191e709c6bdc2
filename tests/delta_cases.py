"""Scenes lit by mitsuba's `point` / `spot` emitters, shared by tests/test_delta_emitters.py (host build) and
tests/test_gpu_delta_emitters.py (MI355X), with the Planes that tests/delta_quadrature.py integrates over."""
import math
import os

import numpy as np

import delta_quadrature as DQ

FLOOR_ALBEDO = (0.8, 0.5, 0.2)
POINT_POS = (0.3, -0.2, 1.1)
POINT_I = (3.0, 5.0, 7.0)


def _T():
    from mitransient_amd.transform import ScalarTransform4f
    return ScalarTransform4f


def _mi():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    return mi


def _sensor(film, spp=64, origin=(0.0, -3.0, 2.5), target=(0.0, 0.0, 0.0), fov=40.0):
    f = {"type": "transient_hdr_film", "rfilter": {"type": "box"}, "temporal_bins": 1, "start_opl": 0.0, "bin_width_opl": 100.0}
    f.update(film)
    return {"type": "perspective", "fov": fov, "fov_axis": "x", "near_clip": 0.1, "far_clip": 100.0,
            "to_world": _T()().look_at(origin=list(origin), target=list(target), up=[0, 0, 1]),
            "sampler": {"type": "independent", "sample_count": spp}, "film": f}


def rgb(*v):
    return {"type": "rgb", "value": list(v)}


FLOOR = DQ.Plane((0, 0, 0), (2, 0, 0), (0, 2, 0), FLOOR_ALBEDO)
WINDOW = {"width": 1024, "height": 768, "crop_width": 6, "crop_height": 4, "crop_offset_x": 600, "crop_offset_y": 300}


def floor_dict(light, film=None, max_depth=2, spp=64, **integ):
    """C2 / C3: one diffuse floor rectangle (z = 0, 4 x 4), a delta emitter above it, a 1024 x 768 film cropped to a 6 x 4 window
    off the image centre"""
    d = {"type": "scene",
         "integrator": dict({"type": "transient_path", "max_depth": max_depth, "rr_depth": 100}, **integ),
         "sensor": _sensor(dict(WINDOW, **(film or {})), spp),
         "floor": {"type": "rectangle", "to_world": _T()().scale(2.0), "bsdf": {"type": "diffuse", "reflectance": rgb(*FLOOR_ALBEDO)}}}
    d["lamp"] = light
    return d


def point_light(pos=POINT_POS, intensity=POINT_I):
    return {"type": "point", "position": list(pos), "intensity": rgb(*intensity)}


def window_centre(film=None):
    """the floor point behind the centre of the crop window"""
    scene = _mi().load_dict(floor_dict(point_light(), film))
    _, _, d, org = DQ.camera_rays(scene, 1)
    h, w = d.shape[:2]
    o, v = org[h // 2, w // 2, 0], d[h // 2, w // 2, 0]
    return o + v * FLOOR.hit(o[None], v[None])[0]


def spot_light(x0, offset=(1.2, 0.3, 3.6), tilt=25.0, edge=20.0, cutoff=20.0, beam=12.0, intensity=(6.0, 4.0, 9.0)):
    """a spot `offset` away from the floor point x0, tilted `tilt` degrees from straight down, turned about the vertical so that x0
    lies `edge` degrees off its axis: with edge = cutoff the cone's edge passes through x0"""
    p = np.asarray(x0, np.float64) + np.asarray(offset, np.float64)
    v = (np.asarray(x0) - p) / np.linalg.norm(np.asarray(x0) - p)
    st, ct = math.sin(math.radians(tilt)), math.cos(math.radians(tilt))
    f = lambda phi: np.array([st * math.cos(phi), st * math.sin(phi), -ct]) @ v - math.cos(math.radians(edge))     # noqa: E731
    phis = np.linspace(0.0, 2.0 * math.pi, 721)
    vals = np.array([f(x) for x in phis])
    k = int(np.nonzero(np.sign(vals[:-1]) != np.sign(vals[1:]))[0][0])
    lo, hi = phis[k], phis[k + 1]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if np.sign(f(mid)) == np.sign(f(lo)) else (lo, mid)
    a = np.array([st * math.cos(lo), st * math.sin(lo), -ct])
    return {"type": "spot", "to_world": _T()().look_at(origin=list(p), target=list(p + a), up=[0, 1, 0]),
            "cutoff_angle": cutoff, "beam_width": beam, "intensity": rgb(*intensity)}


def floor_scene(kind, film=None, **kw):
    mi = _mi()
    light = point_light() if kind == "point" else spot_light(window_centre(film))
    return mi.load_dict(floor_dict(light, film, **kw))


# ---- C4: a floor and a perpendicular wall (a gap between them keeps the one-bounce kernel bounded)
WALL = DQ.Plane((-1.2, 0.0, 1.2), (0, 1, 0), (0, 0, 1), (0.3, 0.7, 0.6))          # x = -1.2, normal +x
FLOOR1 = DQ.Plane((0, 0, 0), (1, 0, 0), (0, 1, 0), FLOOR_ALBEDO)


def corner_scene(spp=16, res=(16, 12), max_depth=3):
    d = {"type": "scene", "integrator": {"type": "transient_path", "max_depth": max_depth, "rr_depth": 100},
         "sensor": _sensor({"width": res[0], "height": res[1]}, spp, origin=(2.2, -2.4, 2.6), target=(-0.1, 0.0, 0.0), fov=10.0),
         "floor": {"type": "rectangle", "bsdf": {"type": "diffuse", "reflectance": rgb(*FLOOR_ALBEDO)}},
         # the rectangle's x -> y, its y -> z, its normal +z -> +x
         "wall": {"type": "rectangle", "to_world": _T()([[0, 0, 1, -1.2], [1, 0, 0, 0], [0, 1, 0, 1.2], [0, 0, 0, 1]]),
                  "bsdf": {"type": "diffuse", "reflectance": rgb(0.3, 0.7, 0.6)}},
         "lamp": point_light((0.2, 0.3, 0.9), (2.0, 3.0, 1.5))}
    return _mi().load_dict(d)


# ---- C5 / G1: the Cornell box's room (no boxes: the room is convex up to the luminaire, which delta_quadrature takes as an occluder)
def cornell_dict(area=True, point=True, spot=True, boxes=False, res=(16, 16), spp=16, max_depth=2, **integ):
    import mitransient_amd as mitr
    src = mitr.cornell_box()
    d = {}
    for k, v in src.items():                       # dictionary order: spot, light (area), point -> emitters 0, 1, 2
        if k == "light":
            if spot:
                d["beam"] = {"type": "spot", "to_world": _T()().look_at(origin=[0.5, 0.6, 0.6], target=[-0.2, -1.0, -0.2], up=[0, 1, 0]),
                             "cutoff_angle": 35.0, "beam_width": 20.0, "intensity": rgb(2.0, 3.0, 4.0)}
            if area:
                d[k] = v
            if point:
                d["lamp"] = {"type": "point", "position": [-0.45, 0.2, 0.35], "intensity": rgb(1.5, 1.0, 0.5)}
        elif k in ("small-box", "large-box") and not boxes:
            continue
        else:
            d[k] = v
    d["sensor"]["film"].update(width=res[0], height=res[1], temporal_bins=16, start_opl=3.0, bin_width_opl=8.0 / 16)
    d["sensor"]["sampler"]["sample_count"] = spp
    d["integrator"].update(max_depth=max_depth, rr_depth=100, **integ)
    return d


def cornell_scene(**kw):
    return _mi().load_dict(cornell_dict(**kw))


WHITE, GREEN, RED = (0.885809, 0.698859, 0.666422), (0.105421, 0.37798, 0.076425), (0.570068, 0.0430135, 0.0443706)
CORNELL_PLANES = [DQ.Plane((0, -1, 0), (1, 0, 0), (0, 0, -1), WHITE),            # floor, normal +y
                  DQ.Plane((0, 1, 0), (1, 0, 0), (0, 0, 1), WHITE),              # ceiling, normal -y
                  DQ.Plane((0, 0, -1), (1, 0, 0), (0, 1, 0), WHITE),             # back, normal +z
                  DQ.Plane((1, 0, 0), (0, 0, 1), (0, 1, 0), GREEN),              # normal -x
                  DQ.Plane((-1, 0, 0), (0, 0, -1), (0, 1, 0), RED),              # normal +x
                  DQ.Plane((0.0, 0.99, 0.01), (0.23, 0, 0), (0, 0, 0.19), WHITE)]  # the luminaire, normal -y
LUMINAIRE = CORNELL_PLANES[5]


# ---- host build
def develop_window(sd, t4, s4):
    """(steady (ch, cw, 3), transient (ch, cw, T, 3)) of the crop window: the accumulators are full-size with the window at their
    top-left corner; rgb over weight, as the film develops them"""
    f = sd.film
    ch, cw = int(f.crop_height), int(f.crop_width)
    t = np.array(t4[:ch, :cw], np.float64)
    s = np.array(s4[:ch, :cw], np.float64)
    tw, sw = t[..., 3:], s[..., 3:]
    return s[..., :3] / np.where(sw == 0, 1.0, sw), t[..., :3] / np.where(tw == 0, 1.0, tw)


def host_render(host_harness, scene, spp, seed=0):
    from conftest import hh_render
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)
    t4, s4, c = hh_render(host_harness, sd, p)
    s, t = develop_window(sd, t4, s4)
    return s, t, c


def obj_file(tmp, tilt=0.15):
    """a 2 x 2 quad of 8 triangles with vertex normals that lean away from the face normal (smooth shading), around z = 0.4"""
    lines = []
    for j in range(3):
        for i in range(3):
            lines.append(f"v {i - 1.0} {j - 1.0} 0.0")
    for j in range(3):
        for i in range(3):
            n = np.array([tilt * (i - 1.0), tilt * (j - 1.0), 1.0])
            n /= np.linalg.norm(n)
            lines.append(f"vn {float(n[0])!r} {float(n[1])!r} {float(n[2])!r}")
    for j in range(2):
        for i in range(2):
            a, b, c, d = j * 3 + i + 1, j * 3 + i + 2, (j + 1) * 3 + i + 2, (j + 1) * 3 + i + 1
            lines += [f"f {a}//{a} {b}//{b} {c}//{c}", f"f {a}//{a} {c}//{c} {d}//{d}"]
    path = os.path.join(str(tmp), "quad.obj")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return path
