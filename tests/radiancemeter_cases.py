"""Scenes of the `radiancemeter` sensor and of the sample-parallel render mode, shared by test_radiancemeter.py (CPU: oracle and
host harness) and test_gpu_samples_mode.py (MI355X).

CLOSED FORM.  A radiancemeter at O looks along P - O at the point P of a diffuse unit rectangle in the z = 0 plane (normal +z,
reflectance a), lit by a `point` emitter of intensity I at L; max_depth = 2.  Every sample is the same path: the camera ray hits P
at t_cam = |P - O|, the emitter-sampling term of that vertex arrives with optical path length t_cam + d, d = |L - P|, and carries
a / pi . cos(theta) . I / d^2, cos(theta) = (L - P).z / d; the sampled continuation leaves the half space of the rectangle and
misses.  The developed transient holds that value in bin floor((t_cam + d - start) / width) and exactly 0 in every other bin; the
steady value is the same.  closed_form() computes all of it in f64 and places the arrival in the middle of bin 20.
The CPU oracle knows nothing of delta emitters (tests/test_delta_emitters.py): on the CPU the scene is rendered by the host build
of the product's own arithmetic (tests/host_harness.cpp), which the Cornell-box cases pin to the oracle bit for bit.
"""
import math

import numpy as np

ALBEDO = (0.8, 0.5, 0.3)
INTENSITY = (30.0, 20.0, 10.0)
P_HIT = np.array([0.2, -0.1, 0.0])
O_METER = np.array([0.8, 0.5, 1.5])
L_POINT = np.array([-0.6, 0.4, 1.2])
BIN_WIDTH = 0.1
ARRIVAL_BIN = 20
CLOSED_BINS = 64
CLOSED_TOL = 1e-5         # relative: the term is a few dozen f32 operations (ray, hit point, distances, cosine, the products)


def _mi():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    return mi


def rgb(*v):
    return {"type": "rgb", "value": list(v)}


def closed_form(origin=O_METER):
    """f64: (optical path length of the arrival, RGB value, start_opl that puts the arrival of the meter AT O_METER mid-bin)"""
    t_cam = float(np.linalg.norm(P_HIT - origin))
    d = float(np.linalg.norm(L_POINT - P_HIT))
    cos_t = float((L_POINT - P_HIT)[2]) / d
    value = np.array([a / math.pi * cos_t * i / (d * d) for a, i in zip(ALBEDO, INTENSITY)])
    t0 = float(np.linalg.norm(P_HIT - O_METER))
    start = t0 + d - (ARRIVAL_BIN + 0.5) * BIN_WIDTH
    return t_cam + d, value, start


def closed_form_dict(form="origin", spp=8, origin=O_METER, **integ):
    """the closed-form scene; form "origin": origin + direction, "to_world": the same pose as a look-at"""
    from mitransient_amd.transform import ScalarTransform4f as T
    _, _, start = closed_form()
    sensor = {"type": "radiancemeter", "sampler": {"type": "independent", "sample_count": spp},
              "film": {"type": "transient_hdr_film", "width": 1, "height": 1, "temporal_bins": CLOSED_BINS,
                       "bin_width_opl": BIN_WIDTH, "start_opl": start, "rfilter": {"type": "box"}}}
    if form == "origin":
        sensor.update(origin=[float(x) for x in origin], direction=[float(x) for x in (P_HIT - origin)])
    else:
        sensor["to_world"] = T().look_at(origin=list(origin), target=list(P_HIT), up=[0, 1, 0])
    idict = {"type": "transient_path", "max_depth": 2, "temporal_filter": "box"}
    idict.update(integ)
    return {"type": "scene", "integrator": idict, "sensor": sensor,
            "wall": {"type": "rectangle", "bsdf": {"type": "diffuse", "reflectance": rgb(*ALBEDO)}},
            "lamp": {"type": "point", "position": [float(x) for x in L_POINT], "intensity": rgb(*INTENSITY)}}


def closed_form_scene(**kw):
    return _mi().load_dict(closed_form_dict(**kw))


# a rotated pose inside the Cornell box (no axis-aligned component) and an axis-aligned one
METER_ORIGIN = [0.25, 0.125, 3.0]
METER_DIRECTION = [-0.3, -0.45, -1.0]
AXIS_ORIGIN = [0.25, -0.5, 3.0]
AXIS_DIRECTION = [0.0, 0.0, -1.0]


def meter_sensor(bins=64, spp=16, form="origin", origin=METER_ORIGIN, direction=METER_DIRECTION, start=3.0, window=8.0):
    from mitransient_amd.transform import ScalarTransform4f as T
    from mitransient_amd.sensors import coordinate_system
    s = {"type": "radiancemeter", "sampler": {"type": "independent", "sample_count": spp},
         "film": {"type": "transient_hdr_film", "width": 1, "height": 1, "temporal_bins": bins, "bin_width_opl": window / bins,
                  "start_opl": start, "rfilter": {"type": "box"}}}
    if form == "origin":
        s.update(origin=list(origin), direction=list(direction))
    else:
        o, v = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
        up, _ = coordinate_system(v / np.linalg.norm(v))
        s["to_world"] = T().look_at(origin=o, target=o + v, up=up)
    return s


def cornell_meter_dict(bins=64, spp=16, form="origin", **integ):
    """the Cornell box (area light, both boxes) seen by a radiancemeter: 1 x 1 film"""
    import mitransient_amd as mitr
    _mi()
    d = mitr.cornell_box()
    d["sensor"] = meter_sensor(bins=bins, spp=spp, form=form)
    d["integrator"].update(integ)
    return d


def cornell_meter(**kw):
    return _mi().load_dict(cornell_meter_dict(**kw))


def oracle_developed(oracle, scene, spp, seed=0, spp_range=None, pixel_range=None):
    """(steady, transient, counters) of the CPU oracle, developed"""
    sd = scene.data()
    film = scene.sensors()[0].film()
    s0, s1 = (0, spp) if spp_range is None else spp_range
    p0, p1 = (0, None) if pixel_range is None else pixel_range
    params = scene.integrator().render_params(film, seed, spp, s0, s1, p0, p1)
    t4, s4, cnt = oracle.render(sd, params, use_bvh=True)
    t3, s3 = oracle.develop(sd.film, t4, s4)
    return np.array(s3), np.array(t3), cnt


def host_developed(host_harness, scene, spp, seed=0, spp_range=None, pixel_range=None):
    """(steady, transient, counters) of the host build of the product's arithmetic (tests/host_harness.cpp), developed"""
    from conftest import hh_render
    from oracle import oracle as _o
    sd = scene.data()
    s0, s1 = (0, spp) if spp_range is None else spp_range
    p0, p1 = (0, None) if pixel_range is None else pixel_range
    params = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp, s0, s1, p0, p1)
    t4, s4, cnt = hh_render(host_harness, sd, params)
    t3, s3 = _o.develop(sd.film, t4, s4)
    return np.array(s3), np.array(t3), cnt
