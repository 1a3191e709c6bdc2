"""MTR_MODE_SAMPLES (a pixel's samples spread over workgroups: k_samples_paths / k_samples_reduce, mtr_samples.hip) and the
`radiancemeter` sensor on the MI355X.  The bound against the CPU references is the one tests/test_gpu_parity.py applies to
non-deterministic f32 rows (relative L2 <= 1e-5, integer counters equal): the GPU adds a pixel's samples in another order.
Films are 1 x 1 (the radiancemeter) or a handful of pixels; the sample counts are the smallest that take each path of the slab
plan: several slabs (4096), a ragged last slab with a partial wave (1037), fewer samples than one slab (3)."""
import ctypes as C

import numpy as np
import pytest

import radiancemeter_cases as RC
import scene_class_cases as cases
from conftest import rel_l2
from test_gpu_parity import TOL
from test_scene_class import EXPECTED

pytestmark = pytest.mark.gpu
GRAD_REL = 1e-5         # tests/test_gpu_grad.py: every gradient element within 1e-5 of its reference
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")


def _render(scene, spp, seed=0, calls=((None, None),), raw=False):
    """the film after one accumulate() per (spp_range, pixel_range) of `calls`: (steady, transient[, raw steady, raw transient],
    counters summed over the calls)"""
    import torch
    integ = scene.integrator()
    integ.collect_stats = True
    sens = scene.sensors()[0]
    passes = integ.prepare(scene, sens, seed, spp, [])
    total = {k: 0 for k in COUNTERS}
    for spp_range, pixel_range in calls:
        integ.accumulate(scene, sens, passes, spp, spp_range=spp_range, pixel_range=pixel_range)
        for k in COUNTERS:
            total[k] += integ.last_counters[k]
    torch.cuda.synchronize()
    s, t = sens.film().develop()
    if raw:
        s_raw, t_raw = sens.film().develop(raw=True)
        return np.array(s), np.array(t), np.array(s_raw), np.array(t_raw), total
    return np.array(s), np.array(t), total


def _plan(scene, spp, spp_range=None, pixel_range=None):
    """(slab_len, n_slabs, kernel name) of mtr_render_samples_plan"""
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    sens = scene.sensors()[0]
    s0, s1 = (0, spp) if spp_range is None else spp_range
    p0, p1 = (0, None) if pixel_range is None else pixel_range
    params = scene.integrator().render_params(sens.film(), 0, spp, s0, s1, p0, p1)
    out = [C.c_uint32(0) for _ in range(4)]
    ctx.check(ctx.lib.mtr_render_samples_plan(scene.gpu_handle(ctx, sens), C.byref(params), *[C.byref(o) for o in out]),
              "mtr_render_samples_plan")
    name = f"k_samples_paths<{'lds' if out[2].value else 'hbm'},{'ext' if out[3].value else 'plain'}>"
    return int(out[0].value), int(out[1].value), name


def _same(got, ref):
    (s, t, c), (rs, rt, rc) = got, ref
    assert np.count_nonzero(rt) > 0
    print("rel-L2 transient", rel_l2(t, rt), "steady", rel_l2(s, rs))
    assert rel_l2(t, rt) <= TOL and rel_l2(s, rs) <= TOL, (rel_l2(t, rt), rel_l2(s, rs))
    for k in COUNTERS:
        assert c[k] == rc[k], (k, c[k], rc[k])


# ---------------------------------------------------------------- radiancemeter, 1 x 1 film, 64 bins
@pytest.mark.parametrize("spp,n_slabs", [(4096, 16), (1037, 5), (3, 1)])
def test_radiancemeter_matches_oracle(oracle, spp, n_slabs):
    scene = RC.cornell_meter(bins=64, spp=spp, amd_mode="samples")
    assert _plan(scene, spp)[1:] == (n_slabs, "k_samples_paths<lds,plain>")
    _same(_render(scene, spp, seed=2), RC.oracle_developed(oracle, scene, spp, seed=2))


def test_radiancemeter_uses_the_samples_mode_by_default():
    """amd_mode unset: a radiancemeter scene renders in the sample-parallel organisation when the plan accepts it — while
    MTR_MODE_AUTO at the C level resolves as for any scene — and falls back to AUTO when it does not (deterministic rows)"""
    from mitransient_amd.integrators import common
    scene = RC.cornell_meter(spp=64)
    integ, sens = scene.integrator(), scene.sensors()[0]
    assert integ.amd_mode == "auto"
    integ.prepare(scene, sens, 0, 64, [])                    # (the film's storage: resolved_mode asks the device it lives on)
    assert cases.planned_mode(scene, 64) in ("fused", "wavefront")
    assert integ.resolved_mode(scene, sens, 64) == ("samples" if common.RADIANCEMETER_DEFAULTS_TO_SAMPLES else cases.planned_mode(scene, 64))
    integ.deterministic = True
    assert integ.resolved_mode(scene, sens, 64) == cases.planned_mode(scene, 64)


@pytest.mark.parametrize("form", ["origin", "to_world"])
def test_closed_form_single_path(host_harness, form):
    scene = RC.closed_form_scene(form=form, spp=1037, amd_mode="samples")
    s, t, c = _render(scene, 1037, seed=5)
    _, value, _ = RC.closed_form()
    print("closed form", value, "gpu", t[0, 0, RC.ARRIVAL_BIN], "steady", s[0, 0])
    assert np.abs(t[0, 0, RC.ARRIVAL_BIN].astype(np.float64) / value - 1.0).max() <= RC.CLOSED_TOL
    assert np.abs(s[0, 0].astype(np.float64) / value - 1.0).max() <= RC.CLOSED_TOL
    assert not np.delete(t[0, 0], RC.ARRIVAL_BIN, axis=0).any()
    _same((s, t, c), RC.host_developed(host_harness, scene, 1037, seed=5))


def test_moving_the_meter_on_the_device(host_harness):
    """a scan: params["sensor.to_world"] in a loop re-flattens the camera alone and hands it to the scene that is on the device"""
    from mitransient_amd.transform import ScalarTransform4f as T
    mi = RC._mi()
    scene = RC.closed_form_scene(spp=64, amd_mode="samples")
    params = mi.traverse(scene)
    handles = None
    for k in (0, 3, 7):
        v = (RC.P_HIT - RC.O_METER) / np.linalg.norm(RC.P_HIT - RC.O_METER)
        moved = RC.O_METER - k * RC.BIN_WIDTH * v
        params["sensor.to_world"] = T().look_at(origin=list(moved), target=list(RC.P_HIT), up=[0, 1, 0])
        params.update()
        s, t, c = _render(scene, 64)
        assert np.flatnonzero(t[0, 0].sum(-1)).tolist() == [RC.ARRIVAL_BIN + k]
        _same((s, t, c), RC.host_developed(host_harness, scene, 64))
        now = {key: h.value for key, h in scene._handles.items()}
        assert handles is None or now == handles             # the device scene was kept: no BVH rebuilt
        handles = now


# ---------------------------------------------------------------- the organisations agree
def _spad_array(mode):
    import mitransient_amd as mitr
    d = mitr.cornell_box()
    d["integrator"]["amd_mode"] = mode
    d["sensor"]["film"].update(width=5, height=4, temporal_bins=64, start_opl=3.0, bin_width_opl=0.125,
                               crop_width=3, crop_height=2, crop_offset_x=1, crop_offset_y=2)
    return RC._mi().load_dict(d)


def test_crop_window_of_a_perspective_film_matches_oracle_and_the_fused_kernel(oracle):
    scene = _spad_array("samples")
    assert _plan(scene, 512)[:2] == (256, 2)                 # 6 pixels x 2 slabs
    got = _render(scene, 512, seed=7)
    _same(got, RC.oracle_developed(oracle, scene, 512, seed=7))
    fused = _render(_spad_array("fused"), 512, seed=7)
    _same(got, fused)
    assert got[1].shape == (4, 5, 64, 3) and not got[1][2:].any() and not got[1][:, 3:].any()      # the crop-size corner alone is written


# ---------------------------------------------------------------- sub-ranges and accumulation
def test_two_sample_ranges_sum_to_the_one_call_film(oracle):
    scene = RC.cornell_meter(bins=64, spp=1037, amd_mode="samples")
    whole = _render(scene, 1037, seed=4)
    parts = _render(scene, 1037, seed=4, calls=(((0, 300), None), ((300, 1037), None)))
    _same(parts, whole)
    _same(parts, RC.oracle_developed(oracle, scene, 1037, seed=4))


def test_pixel_range_leaves_the_other_rows_untouched_and_a_second_call_doubles(oracle):
    scene = _spad_array("samples")
    s, t, s_raw, t_raw, c = _render(scene, 65, seed=1, calls=((None, (2, 5)),), raw=True)
    _same((s, t, c), RC.oracle_developed(oracle, scene, 65, seed=1, pixel_range=(2, 5)))
    flat = t.reshape(20, -1)                                 # crop-window pixels 2, 3, 4 are film pixels (0, 2), (1, 0), (1, 1)
    touched = set(np.flatnonzero(np.abs(flat).sum(-1)).tolist())
    assert touched and touched <= {2, 5, 6}, touched
    assert np.all(t_raw[..., 3] == 0)                        # W stays 0
    s2, t2, s2_raw, t2_raw, c2 = _render(scene, 65, seed=1, calls=((None, (2, 5)), (None, (2, 5))), raw=True)
    assert np.array_equal(t2_raw, 2.0 * t_raw) and np.array_equal(s2_raw, 2.0 * s_raw)           # the contract says ADDS
    assert s2_raw.max() == 130.0 and c2["paths"] == 2 * c["paths"]           # the sample count in .w


# ---------------------------------------------------------------- one scene per instantiation
def _sphere_room(tmp):
    import sphere_cases as SC
    return RC._mi().load_dict(SC.room_dict(res=(4, 3), bins=16, spp=40))


def _hbm_stairs(tmp):
    """852 triangles (tests/test_gpu_parity.py's stand-in for the staircase): over the LDS scene budget; camera_unwarp is on"""
    from mitransient_amd.scenes import staircase_like
    return RC._mi().load_dict(staircase_like(n_steps=12, balusters=2, tiles=6, spp=40, max_depth=12, width=4, height=3, temporal_bins=16))


INSTANCES = {
    "cornell-config1": (cases.CASES["cornell-config1"], "k_samples_paths<lds,plain>"),
    "rough-ggx": (cases.CASES["rough-ggx"], "k_samples_paths<lds,ext>"),                  # a rough lobe
    "textured-diffuse": (cases.CASES["textured-diffuse"], "k_samples_paths<lds,ext>"),    # a bitmap
    "sphere-room": (_sphere_room, "k_samples_paths<lds,plain>"),                           # analytic spheres (the general code walks them)
    "stairs-852": (_hbm_stairs, "k_samples_paths<hbm,plain>"),
    "staircase-rough-normals-textures": (cases.CASES["staircase-rough-normals-textures"], "k_samples_paths<hbm,ext>"),
}


@pytest.mark.parametrize("name", list(INSTANCES))
def test_each_instantiation_matches_the_host_build(host_harness, tmp_path, name):
    """five pixels in the middle of the film, 300 samples each (two slabs, the second ragged); the case names the kernel it ran"""
    build, kernel = INSTANCES[name]
    scene = build(tmp_path)
    scene.integrator().amd_mode = "samples"
    if name in EXPECTED:
        assert ("ext" in kernel) == bool(EXPECTED[name][1])
    cw, ch = scene.sensors()[0].film().crop_size()
    p0 = (cw * ch) // 2
    rng = (p0, p0 + 5)
    slab_len, n_slabs, ran = _plan(scene, 300, pixel_range=rng)
    print(name, "ran", ran, "slabs", n_slabs, "x", slab_len)
    assert ran == kernel and (slab_len, n_slabs) == (256, 2)
    _same(_render(scene, 300, seed=6, calls=((None, rng),)), RC.host_developed(host_harness, scene, 300, seed=6, pixel_range=rng))


@pytest.mark.parametrize("flags", [{"camera_unwarp": True}, {"discard_direct_light": True}, {"camera_unwarp": True, "discard_direct_light": True}])
def test_unwarp_and_discard_direct_light(oracle, flags):
    d = RC.cornell_meter_dict(bins=64, spp=300, amd_mode="samples", **flags)
    d["sensor"]["film"].update(start_opl=0.0, bin_width_opl=0.125)         # (unwarped arrivals start at 0)
    scene = RC._mi().load_dict(d)
    _same(_render(scene, 300, seed=8), RC.oracle_developed(oracle, scene, 300, seed=8))


def test_mono_variant(oracle):
    import mitransient_amd.mi as mi
    try:
        mi.set_variant("llvm_ad_mono")
        scene = mi.load_dict(RC.cornell_meter_dict(bins=64, spp=300, amd_mode="samples"))
        got = _render(scene, 300, seed=9)
        sd = scene.data()
        p = scene.integrator().render_params(scene.sensors()[0].film(), 9, 300)
        t4, s4, cnt = oracle.render(sd, p, use_bvh=True)
        t3, s3 = oracle.develop(sd.film, t4, s4)
        _same((got[0][..., 0], got[1][..., 0], got[2]), (np.array(s3)[..., 0], np.array(t3)[..., 0], cnt))       # the luminance channel
    finally:
        mi.set_variant("llvm_ad_rgb")


# ---------------------------------------------------------------- refusals, plan, AUTO
def _raw_call(scene, flags=0, n_bands=0, film=None, spp=8):
    """mtr_render in mode 3 on tensors filled with 7: (status, message, tensors untouched)"""
    import torch
    from mitransient_amd import _cabi
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    sens = scene.sensors()[0]
    h = scene.gpu_handle(ctx, sens)
    fd = scene.data(sens).film if film is None else film
    if film is not None:
        ctx.check(ctx.lib.mtr_scene_set_film(h, C.byref(fd)), "mtr_scene_set_film")
    params = scene.integrator().render_params(sens.film(), 0, spp)
    params.mode = _cabi.MTR_MODE_SAMPLES
    params.flags |= flags
    words = 2 * fd.n_frequencies + 1 if fd.n_frequencies else max(1, fd.laser_scan_width * fd.laser_scan_height) * fd.temporal_bins * 4
    t4 = torch.full((fd.height, fd.width, words), 7.0, device="cuda")
    s4 = torch.full((fd.height, fd.width, 4), 7.0, device="cuda")
    band = torch.zeros(4, dtype=torch.int32, device="cuda")
    if n_bands:
        params.n_bands, params.band_epoch, params.band_done = n_bands, 1, band.data_ptr()
    mode = C.c_uint32(99)
    plan = ctx.lib.mtr_render_plan(h, C.byref(params), C.byref(mode), None)
    rc = ctx.lib.mtr_render(h, C.byref(params), C.c_void_p(t4.data_ptr()), C.c_void_p(s4.data_ptr()), None, None)
    msg = (ctx.lib.mtr_last_error(ctx.handle) or b"").decode()
    torch.cuda.synchronize()
    return rc, plan, int(mode.value), msg, bool((t4 == 7.0).all() and (s4 == 7.0).all())


def _refused(scene, what, **kw):
    rc, plan, mode, msg, untouched = _raw_call(scene, **kw)
    assert rc == -5 and untouched and what in msg, (rc, msg, untouched)          # MTR_ERR_UNSUPPORTED before any launch
    assert plan == -5 and mode == 99                                             # ... and from the plan


def test_refusals_leave_both_tensors_untouched(tmp_path):
    from conftest import make_nlos
    from mitransient_amd import _cabi
    import mitransient_amd.mi as mi
    meter = RC.cornell_meter()
    _refused(make_nlos(), "the NLOS tier")
    _refused(meter, "MTR_FLAG_POLARIZED", flags=_cabi.MTR_FLAG_POLARIZED)
    _refused(meter, "MTR_FLAG_DETERMINISTIC", flags=_cabi.MTR_FLAG_DETERMINISTIC)
    _refused(meter, "MTR_FLAG_DEVELOPED_ROWS", flags=_cabi.MTR_FLAG_DEVELOPED_ROWS)
    _refused(meter, "band completion words", n_bands=1)
    scan = _cabi.mtr_film_desc.from_buffer_copy(meter.data().film)
    scan.laser_scan_width, scan.laser_scan_height = 2, 2
    _refused(meter, "an exhaustive_scan film", film=scan)
    long_row = _cabi.mtr_film_desc.from_buffer_copy(meter.data().film)
    long_row.temporal_bins = 14000                            # 3 x 14000 x 4 B = 164 KiB of row
    _refused(meter, "exceed the 160 KiB", film=long_row)
    try:
        mi.set_variant("llvm_ad_mono")
        d = RC.cornell_meter_dict()
        d["sensor"]["film"] = {"type": "phasor_hdr_film", "width": 1, "height": 1, "wl_mean": 2.0, "wl_sigma": 1.0, "temporal_bins": 400,
                               "bin_width_opl": 0.05, "start_opl": 3.0, "rfilter": {"type": "box"}}
        _refused(mi.load_dict(d), "a phasor_hdr_film")
    finally:
        mi.set_variant("llvm_ad_rgb")


def test_plan_reports_the_mode_and_auto_is_what_it_was(tmp_path):
    rc, plan, mode, msg, untouched = _raw_call(RC.cornell_meter())
    assert (rc, plan, mode) == (0, 0, 3) and not untouched
    for name in ("cornell-config1", "mirror-box", "cornell-mesh-boxes", "five-cubes", "far-triangle", "rough-ggx", "textured-diffuse"):
        assert cases.planned_mode(cases.CASES[name](tmp_path)) == EXPECTED[name][3], name


# ---------------------------------------------------------------- gradient on a radiancemeter scene
def test_radiance_gradient_is_the_unit_render():
    """render_backward with g = 1 gives, for the emitter's radiance, the film sum of a primal render at the same seed with unit
    radiance: the estimator is linear in it (an identity, not an estimate).  The camera is data to the gradient kernels."""
    import torch
    mi = RC._mi()
    key = "light.emitter.radiance.value"
    scene = RC.cornell_meter(bins=64, spp=300, amd_mode="samples")
    p = mi.traverse(scene)
    saved = list(p[key])
    p[key] = [1.0, 1.0, 1.0]
    p.update()
    u_s, u_t, _ = _render(scene, 300, seed=9)
    p[key] = saved
    p.update()
    assert np.count_nonzero(u_t) > 10
    want = u_s.astype(np.float64).sum((0, 1)) + u_t.astype(np.float64).sum((0, 1, 2))
    g_s = torch.ones((1, 1, 3), device="cuda")
    g_t = torch.ones((1, 1, 64, 3), device="cuda")
    p[key] = torch.tensor(list(p[key]), requires_grad=True)
    got = scene.integrator().render_backward(scene, p, grad_in=(g_s, g_t), seed=9, spp=300)[key].cpu().numpy().astype(np.float64)
    print("gradient", got, "unit render", want)
    assert np.abs(got - want).max() <= GRAD_REL * np.abs(want).max(), (got, want)
