"""mitsuba's `radiancemeter` sensor on the CPU: the flattened camera record against the oracle's camera_ray, the host build of the
product's arithmetic against the oracle, a closed-form single-path measurement, and the plugin's surface (refusals, XML, traverse).
The cases are radiancemeter_cases.py's; test_gpu_samples_mode.py runs them on the MI355X."""
import os

import numpy as np
import pytest

import radiancemeter_cases as RC
from conftest import hh_render

JITTERS = [(0.0, 0.0), (0.5, 0.5), (0.99999994, 0.0), (0.0, 0.99999994), (0.25, 0.75), (0.99999994, 0.99999994)]


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


# ---------------------------------------------------------------- mapping
@pytest.mark.parametrize("form", ["origin", "to_world"])
def test_axis_aligned_meter_is_origin_and_direction_bit_for_bit(oracle, form):
    d = RC.cornell_meter_dict(form=form)
    d["sensor"] = RC.meter_sensor(form=form, origin=RC.AXIS_ORIGIN, direction=RC.AXIS_DIRECTION)
    sd = RC._mi().load_dict(d).data()
    assert sd.camera.near_clip == 0.0 and sd.camera.far_clip == np.finfo(np.float32).max
    for j1, j2 in JITTERS:
        o, v, tmax = oracle.camera_ray(sd, 0, 0, np.float32(j1), np.float32(j2))
        assert np.array_equal(o, np.asarray(RC.AXIS_ORIGIN, np.float32))
        assert np.array_equal(v, np.asarray(RC.AXIS_DIRECTION, np.float32))
        assert np.isfinite(tmax) and tmax == np.finfo(np.float32).max


@pytest.mark.parametrize("form", ["origin", "to_world"])
def test_rotated_meter_is_origin_and_unit_direction_within_2_ulp(oracle, form):
    sd = RC.cornell_meter(form=form).data()
    want = np.asarray(RC.METER_DIRECTION, np.float64)
    want = (want / np.linalg.norm(want)).astype(np.float32)
    rays = [oracle.camera_ray(sd, 0, 0, np.float32(j1), np.float32(j2)) for j1, j2 in JITTERS]
    for o, v, tmax in rays:
        assert np.array_equal(o, np.asarray(RC.METER_ORIGIN, np.float32))
        assert _ulps(v, want) <= 2
        assert np.isfinite(tmax)
        assert np.array_equal(v, rays[0][1])                 # the jitter is drawn and has no effect


def test_both_property_forms_flatten_to_one_camera():
    a, b = RC.cornell_meter(form="origin").data().camera, RC.cornell_meter(form="to_world").data().camera
    assert list(a.sample_to_camera) == list(b.sample_to_camera) == [0.0] * 11 + [1.0, 0.0, 0.0, 0.0, 1.0]
    assert list(a.to_world) == list(b.to_world)


@pytest.mark.parametrize("flags", [{}, {"camera_unwarp": True}, {"discard_direct_light": True}])
def test_host_harness_is_the_oracle_bit_for_bit(oracle, host_harness, flags):
    scene = RC.cornell_meter(spp=64, **flags)
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), 3, 64)
    t_o, s_o, c_o = oracle.render(sd, p, use_bvh=True)
    t_h, s_h, c_h = hh_render(host_harness, sd, p)
    assert np.count_nonzero(t_o) > 10
    assert np.array_equal(t_o, t_h) and np.array_equal(s_o, s_h)
    for k in ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces"):
        assert c_o[k] == c_h[k], k
    assert c_o["paths"] == 64


def test_escaped_rays_end_as_for_a_perspective_sensor(oracle):
    """a meter that looks out of the open front of the box: every path is one bounce, nothing is added, tmax stays finite"""
    d = RC.cornell_meter_dict(spp=8)
    d["sensor"] = RC.meter_sensor(spp=8, origin=[0.0, 0.0, 3.0], direction=[0.0, 0.0, 1.0])
    scene = RC._mi().load_dict(d)
    s, t, c = RC.oracle_developed(oracle, scene, 8)
    assert not t.any() and not s.any() and np.isfinite(t).all()
    assert c["paths"] == 8 and c["bounces"] == 8 and c["rays_closest"] == 8 and c["rays_shadow"] == 0 and c["splats_issued"] == 0


# ---------------------------------------------------------------- closed form
@pytest.mark.parametrize("form", ["origin", "to_world"])
def test_closed_form_single_path(host_harness, form):
    scene = RC.closed_form_scene(form=form, spp=8)
    s, t, c = RC.host_developed(host_harness, scene, 8, seed=5)
    opl, value, start = RC.closed_form()
    assert int(np.floor((opl - start) / RC.BIN_WIDTH)) == RC.ARRIVAL_BIN
    assert t.shape == (1, 1, RC.CLOSED_BINS, 3) and s.shape == (1, 1, 3)
    print("closed form", value, "host build", t[0, 0, RC.ARRIVAL_BIN], "steady", s[0, 0])
    assert np.abs(t[0, 0, RC.ARRIVAL_BIN].astype(np.float64) - value).max() <= RC.CLOSED_TOL * value.max()
    assert np.abs(t[0, 0, RC.ARRIVAL_BIN].astype(np.float64) / value - 1.0).max() <= RC.CLOSED_TOL
    assert np.abs(s[0, 0].astype(np.float64) / value - 1.0).max() <= RC.CLOSED_TOL
    rest = np.delete(t[0, 0], RC.ARRIVAL_BIN, axis=0)
    assert not rest.any()                                    # every other bin is exactly 0
    assert c["paths"] == 8 and c["rays_shadow"] == 8 and c["splats_issued"] == 8


# ---------------------------------------------------------------- refusals and surface
def test_film_must_be_one_pixel():
    d = RC.cornell_meter_dict()
    d["sensor"]["film"]["width"] = 2
    with pytest.raises(ValueError, match="only supports films of size 1x1"):
        RC._mi().load_dict(d)


def test_to_world_and_origin_together_are_refused():
    from mitransient_amd.transform import ScalarTransform4f as T
    d = RC.cornell_meter_dict()
    d["sensor"]["to_world"] = T().translate([0, 0, 3])
    with pytest.raises(ValueError, match="can be specified at the same time"):
        RC._mi().load_dict(d)
    d = RC.cornell_meter_dict()
    del d["sensor"]["direction"]
    with pytest.raises(ValueError, match="both values must be set"):
        RC._mi().load_dict(d)


def test_unknown_sensor_message_lists_the_radiancemeter():
    d = RC.cornell_meter_dict()
    with pytest.raises(ValueError, match="supported sensors: perspective, radiancemeter, nlos_capture_meter"):
        RC._mi()._make_sensor(dict(d["sensor"], type="orthographic"))


def test_nlos_integrator_refuses_the_meter():
    mi = RC._mi()
    d = RC.cornell_meter_dict()
    d["integrator"] = {"type": "transient_nlos_path", "max_depth": 4}
    with pytest.raises(ValueError, match="radiancemeter cannot capture a NLOS scene"):
        mi.load_dict(d)


@pytest.mark.parametrize("variant", ["llvm_ad_mono_polarized", "cuda_ad_mono_polarized"])
def test_polarized_variants_refuse_the_meter_before_any_gpu_work(variant):
    import mitransient_amd.mi as mi
    try:
        mi.set_variant(variant)
        scene = mi.load_dict(RC.closed_form_dict())
        with pytest.raises(ValueError, match="unpolarized variants only"):
            scene.data()
        with pytest.raises(ValueError, match="unpolarized variants only"):
            scene.integrator().render(scene, spp=4)
    finally:
        mi.set_variant("llvm_ad_rgb")


def test_stand_alone_and_nested_plugin():
    mi = RC._mi()
    from mitransient_amd.sensors import RadianceMeter
    meter = mi.load_dict(RC.meter_sensor())
    assert isinstance(meter, RadianceMeter) and tuple(meter.film().size()) == (1, 1) and meter.sampler().sample_count() == 16
    d = RC.cornell_meter_dict()
    d["sensor"] = meter                                       # an object loaded on its own keeps its identity in the scene
    scene = mi.load_dict(d)
    assert scene.sensors()[0] is meter
    assert list(scene.data().camera.to_world) == list(RC.cornell_meter().data().camera.to_world)


XML = """<scene version="3.0.0">
  <integrator type="transient_path"><integer name="max_depth" value="2"/><string name="temporal_filter" value="box"/></integrator>
  <sensor type="radiancemeter">
    {pose}
    <sampler type="independent"><integer name="sample_count" value="8"/></sampler>
    <film type="transient_hdr_film"><integer name="width" value="1"/><integer name="height" value="1"/>
      <integer name="temporal_bins" value="{bins}"/><float name="bin_width_opl" value="{width!r}"/><float name="start_opl" value="{start!r}"/>
      <rfilter type="box"/></film>
  </sensor>
  <shape type="rectangle" id="wall"><bsdf type="diffuse"><rgb name="reflectance" value="{a[0]!r}, {a[1]!r}, {a[2]!r}"/></bsdf></shape>
  <emitter type="point" id="lamp"><point name="position" x="{l[0]!r}" y="{l[1]!r}" z="{l[2]!r}"/>
    <rgb name="intensity" value="{i[0]!r}, {i[1]!r}, {i[2]!r}"/></emitter>
</scene>
"""


@pytest.mark.parametrize("form", ["origin", "to_world"])
def test_xml_round_trip(host_harness, tmp_path, form):
    """the closed-form scene written as Mitsuba XML renders what its dictionary renders, bit for bit"""
    o, v = RC.O_METER, RC.P_HIT - RC.O_METER
    if form == "origin":
        pose = (f'<point name="origin" x="{float(o[0])!r}" y="{float(o[1])!r}" z="{float(o[2])!r}"/>'
                f'<vector name="direction" x="{float(v[0])!r}" y="{float(v[1])!r}" z="{float(v[2])!r}"/>')
    else:
        pose = (f'<transform name="to_world"><lookat origin="{float(o[0])!r}, {float(o[1])!r}, {float(o[2])!r}" '
                f'target="{float(RC.P_HIT[0])!r}, {float(RC.P_HIT[1])!r}, {float(RC.P_HIT[2])!r}" up="0, 1, 0"/></transform>')
    path = os.path.join(str(tmp_path), "meter.xml")
    with open(path, "w") as fh:
        fh.write(XML.format(pose=pose, bins=RC.CLOSED_BINS, width=RC.BIN_WIDTH, start=RC.closed_form()[2], a=RC.ALBEDO,
                            l=[float(x) for x in RC.L_POINT], i=RC.INTENSITY))
    mi = RC._mi()
    from mitransient_amd.sensors import RadianceMeter
    scene = mi.load_file(path)
    assert isinstance(scene.sensors()[0], RadianceMeter)
    a = RC.host_developed(host_harness, scene, 8, seed=5)
    b = RC.host_developed(host_harness, RC.closed_form_scene(form=form, spp=8), 8, seed=5)
    assert a[1].any() and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]) and a[2] == b[2]


def test_moving_the_meter_through_traverse_moves_the_first_hit_bin(host_harness):
    """params["sensor.to_world"] of a scene is settable as for `perspective`; update() re-flattens the camera alone — the flattened
    geometry is the same object — and the arrival moves by the distance the meter backed off along its ray"""
    from mitransient_amd.transform import ScalarTransform4f as T
    mi = RC._mi()
    scene = RC.closed_form_scene(spp=4)
    sd0 = scene.data()
    tris0 = sd0.tri_verts
    _, t0, _ = RC.host_developed(host_harness, scene, 4)
    assert np.flatnonzero(t0[0, 0].sum(-1)).tolist() == [RC.ARRIVAL_BIN]
    back = 7.0 * RC.BIN_WIDTH                                # mid-bin stays mid-bin, 7 bins later: half a bin of slack for f32
    v = (RC.P_HIT - RC.O_METER) / np.linalg.norm(RC.P_HIT - RC.O_METER)
    moved = RC.O_METER - back * v
    params = mi.traverse(scene)
    assert "sensor.to_world" in params
    params["sensor.to_world"] = T().look_at(origin=list(moved), target=list(RC.P_HIT), up=[0, 1, 0])
    params.update()
    sd1 = scene.data()
    assert sd1 is sd0 and sd1.tri_verts is tris0             # nothing but the camera was flattened again
    assert np.allclose(np.asarray(list(sd1.camera.to_world), np.float64).reshape(4, 4)[:3, 3], moved, atol=1e-6)
    _, t1, _ = RC.host_developed(host_harness, scene, 4)
    opl, value, start = RC.closed_form(origin=moved)
    want_bin = int(np.floor((opl - start) / RC.BIN_WIDTH))
    assert want_bin == RC.ARRIVAL_BIN + 7
    assert np.flatnonzero(t1[0, 0].sum(-1)).tolist() == [want_bin]
    assert np.abs(t1[0, 0, want_bin].astype(np.float64) / value - 1.0).max() <= RC.CLOSED_TOL


def test_samples_mode_is_a_mode_of_the_integrator():
    from mitransient_amd import _cabi
    scene = RC.cornell_meter(amd_mode="samples")
    integ = scene.integrator()
    assert integ.amd_mode == "samples" and int(integ.mode) == _cabi.MTR_MODE_SAMPLES == 3
    integ.amd_mode = "auto"
    assert int(integ.render_params(scene.sensors()[0].film(), 0, 4).mode) == _cabi.MTR_MODE_AUTO
    assert _cabi.MTR_ABI_VERSION == 24


def test_slab_plan():
    """samples_plan (mtr_samples.hip): slabs are whole workgroup passes, ragged at the end, never more than samples, and enough
    (pixel, slab) items to fill the device when the samples allow it"""
    import ctypes as C
    from mitransient_amd import _cabi
    assert os.path.exists(_cabi.LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(_cabi.LIB_PATH)
    lib.mtr_test_samples_plan.argtypes = [C.c_uint32] * 5 + [C.c_int, C.POINTER(C.c_uint32)]

    def plan(bins, scene_b, levels, n_pixels, spp, n_cu=256):
        out = (C.c_uint32 * 5)()
        ok = lib.mtr_test_samples_plan(bins, scene_b, levels, n_pixels, spp, n_cu, out)
        return None if not ok else dict(slab_len=out[0], n_slabs=out[1], grid=out[2], scene_lds=out[3], lds=out[4])

    for bins, n_pixels, spp in [(64, 1, 4096), (64, 1, 1037), (64, 1, 3), (64, 16, 1 << 22), (4096, 1, 1 << 22), (64, 6, 512),
                                (300, 1, 1), (64, 4096, 2), (64, 1, 0xffffffff)]:
        p = plan(bins, 8192, 2, n_pixels, spp)
        assert p is not None
        assert p["slab_len"] % 256 == 0 and 1 <= p["n_slabs"] <= spp
        assert (p["n_slabs"] - 1) * p["slab_len"] < spp <= p["n_slabs"] * p["slab_len"]        # the slabs cover the samples, the last ragged
        assert 1 <= p["grid"] <= n_pixels * p["n_slabs"] and p["lds"] <= 160 * 1024
    assert plan(64, 8192, 2, 1, 4096)["n_slabs"] == 16 and plan(64, 8192, 2, 1, 1037)["n_slabs"] == 5
    assert plan(64, 8192, 2, 1, 3)["n_slabs"] == 1
    p = plan(4096, 8192, 2, 1, 1 << 22, n_cu=256)             # a 48 KiB row: fewer resident workgroups, still hundreds of slabs
    assert p["n_slabs"] == p["grid"] >= 256
    # a long row beside a scene that fits LDS on its own: the scene is walked in HBM instead; a row beyond 160 KiB is refused
    assert plan(64, 60000, 2, 1, 4096)["scene_lds"] == 1
    assert plan(10000, 60000, 2, 1, 4096)["scene_lds"] == 0
    assert plan(14000, 0, 2, 1, 4096) is None
