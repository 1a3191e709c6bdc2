"""The `angulararea` emitter on the MI355X: k_fused and the wavefront kernels against the host build of the same arithmetic
(tests/host_harness.cpp over mtr_core.h), same seed; the tutorial notebook's cells as written; the quadrature of
tests/angular_quadrature.py at the notebook's sample count."""
import math
import os

import numpy as np
import pytest

from angular_quadrature import SCENES, agrees, display, load_figure, load_notebook_scene, ncc, quadrature, spot_extent
from conftest import hh_render, rel_l2

pytestmark = pytest.mark.gpu
MODES = ["fused", "wavefront"]
TOL = 1e-5          # the bar of every GPU / CPU parity test here: the GPU adds a pixel's samples in another order
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")


def _notebook(view, res=24, spp=16, mode="fused", **integ):
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    scene = mi.load_file(os.path.join(SCENES, "angular_1light.xml"), res=res, spp=spp)
    if view == 2:                            # the notebook's cell 6
        params = mi.traverse(scene)
        params["sensor.to_world"] = params["sensor.to_world"].look_at(
            mi.ScalarPoint3f(0, 50, 10), mi.ScalarPoint3f(0, 0, 30), mi.ScalarPoint3f(0, 0, 1))
        params.update()
    integrator = scene.integrator()
    integrator.amd_mode = mode
    for k, v in integ.items():
        setattr(integrator, k, v)
    return scene


def _cornell(mode, second_area_light=False):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=24, height=24, temporal_bins=64, bin_width_opl=6.0 / 64)
    d["integrator"]["amd_mode"] = mode
    d["light"]["emitter"] = {"type": "angulararea", "cutoff_angle": 60, "beam_width": 30,
                             "radiance": d["light"]["emitter"].get("radiance", 1.0)}
    if second_area_light:
        d["light2"] = {"type": "rectangle", "to_world": T().translate([-0.98, 0.0, 0.3]).rotate([0, 1, 0], 90).scale(0.15),
                       "bsdf": {"type": "ref", "id": "white"},
                       "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [4.0, 9.0, 2.0]}}}
    return mi.load_dict(d)


def _gpu(scene, spp, seed=0):
    import torch
    integ = scene.integrator()
    integ.collect_stats = True
    s, t = integ.render(scene, seed=seed, spp=spp)
    torch.cuda.synchronize()
    return np.array(s), np.array(t), dict(integ.last_counters)


def _host(host_harness, scene, spp, seed=0):
    from oracle import oracle as _o
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)
    t4, s4, c = hh_render(host_harness, sd, p)
    t3, s3 = _o.develop(sd.film, t4, s4)
    return np.array(s3), np.array(t3), c


def _same(host_harness, scene, spp, seed=0):
    s, t, c = _gpu(scene, spp, seed)
    hs, ht, hc = _host(host_harness, scene, spp, seed)
    assert np.count_nonzero(ht) > 20
    assert rel_l2(t, ht) <= TOL and rel_l2(s, hs) <= TOL, (rel_l2(t, ht), rel_l2(s, hs))
    for k in COUNTERS:
        assert c[k] == hc[k], k
    return s, t


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("view", [1, 2])
def test_notebook_scene_matches_host(host_harness, mode, view):
    scene = _notebook(view, mode=mode)
    assert scene.data().emitters[0].angular == 1
    _same(host_harness, scene, 16, seed=3)


@pytest.mark.parametrize("mode", MODES)
def test_cornell_angular_rectangle_matches_host(host_harness, mode):
    """the Cornell box's luminaire as angulararea (60 / 30 degrees): an analytic rectangle emitter, kept out of the
    kTrOneRectEmitter kernels"""
    from mitransient_amd import _cabi
    scene = _cornell(mode)
    assert scene.data().emitters[0].angular == 1 and scene.data().emitters[0].is_mesh == 0
    assert not (scene.gpu_traits() & _cabi.MTR_TRAIT_ONE_RECT_EMITTER)
    _same(host_harness, scene, 16, seed=1)


@pytest.mark.parametrize("mode", MODES)
def test_area_and_angular_emitters_together(host_harness, mode):
    scene = _cornell(mode, second_area_light=True)
    sd = scene.data()
    assert sd.n_emitters == 2 and sorted(sd.emitters[i].angular for i in range(2)) == [0, 1]
    _same(host_harness, scene, 16, seed=2)


def test_deterministic_renders_are_bit_identical():
    """(the tutorial's meshes carry vertex normals: deterministic rows of such scenes run in the wavefront organisation)"""
    scene = _notebook(1, mode="wavefront", deterministic=True)
    a = _gpu(scene, 16)
    b = _gpu(scene, 16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.count_nonzero(a[1]) > 20


@pytest.mark.parametrize("mode", MODES)
def test_notebook_scene_matches_quadrature(mode):
    """the first view, 48 x 48 pixels, 8 renders of 32 spp (the notebook's 256) against the literal reading's quadrature: the
    bounds of angular_quadrature.agrees (sample variance and the quadrature's own error, nothing fixed)"""
    scene = _notebook(1, res=48, spp=32, mode=mode)
    runs = np.array([_gpu(scene, 32, seed=k)[0] for k in range(8)], np.float64)
    q, _ = quadrature(scene, S=8, transient=False)
    qc, _ = quadrature(scene, S=4, transient=False)
    agrees(runs, q, qc)
    alt, _ = quadrature(scene, S=4, literal=False, transient=False)
    assert rel_l2(runs.mean(0), alt) > 0.9


@pytest.mark.parametrize("kind,view", [("angular", 1), ("angular", 2), ("area", 1), ("area", 2)])
def test_notebook_figures_on_the_gpu(kind, view):
    """the notebook's own renders (tests/golden/angular_figures.npz) against this GPU's render of the same scene at the same
    size and sample count (200 x 200; 256 spp in view 1, 64 in view 2), through the notebook's display (x / max)^(1/4).  Bounds as
    in tests/test_angular_emitter.py::test_quadrature_matches_the_notebook_figures (the host build of the same render, measured:
    angular NCC 0.9991 / 0.9961, mean difference 0.0024 / 0.0033, lit extent 144 x 51 and 67 x 96 against the figures' 144 x 51 and
    68 x 96; area NCC 0.982 / 0.996)."""
    scene = load_notebook_scene(kind, view)
    scene.integrator().amd_mode = "fused"
    s, _, _ = _gpu(scene, 256 if view == 1 else 64)
    img, fig = display(s), load_figure(f"{kind}_view{view}")
    c, d = ncc(img, fig), float(np.abs(img - fig).mean())
    if kind == "area":
        assert c >= 0.975 and d <= 0.01, (c, d)
        return
    assert c >= 0.99 and d <= 0.008, (c, d)
    (gr, gc), (fr, fc) = spot_extent(img), spot_extent(fig)
    assert abs(gr - fr) <= 3 and abs(gc - fc) <= 3, ((gr, gc), (fr, fc))


def test_notebook_cells_run_as_written():
    """cells 3 and 6 of examples/angulararea-emitter/render_angular_1light.ipynb through this package's `mi`"""
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    scene = mi.load_file(os.path.abspath(os.path.join(SCENES, "angular_1light.xml")), res=32)
    data_steady, data_transient = mi.render(scene, spp=16)
    first = np.array(data_steady)
    assert first.shape == (32, 32, 3) and np.array(data_transient).shape == (32, 32, 200, 3) and first.max() > 0

    scene = mi.load_file(os.path.abspath(os.path.join(SCENES, "angular_1light.xml")), res=32)
    params = mi.traverse(scene)
    params['sensor.to_world'] = params['sensor.to_world'].look_at(
        mi.ScalarPoint3f(0, 50, 10),  # origin
        mi.ScalarPoint3f(0, 0, 30),      # target
        mi.ScalarPoint3f(0, 0, 1)    # up
    )
    params.update()
    data_steady, data_transient = mi.render(scene, spp=16)
    second = np.array(data_steady)
    assert second.shape == (32, 32, 3) and second.max() > 0 and not np.allclose(first, second)


# ---------------------------------------------------------------- against the oracle's restatement of angulararea.py (f64 falloff)
import angular_cases as AC          # noqa: E402


def _vs_oracle(scene, spp, seed, what="", **p):
    s, t, c = _gpu(scene, spp, seed)
    return AC.assert_matches_oracle(s, t, c, AC.oracle_render(scene, seed, spp, **p), what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(AC.SCENE_CASES))
def test_gpu_matches_oracle(tmp_path, mode, case):
    """every scene of tests/angular_cases.py in both organisations against the oracle: rel-L2 <= 1e-5 outside the near pixels,
    counters equal up to the near total"""
    build, seed, spp, _ = AC.SCENE_CASES[case]
    scene = build(str(tmp_path))
    scene.integrator().amd_mode = mode
    _vs_oracle(scene, spp, seed, case)


@pytest.mark.parametrize("case", ["notebook_view1", "cornell_60_30", "area_and_angular"])
def test_gpu_deterministic_rows_match_oracle(tmp_path, case):
    """amd_deterministic (64-bit fixed-point rows): two renders bit for bit equal, and the oracle's film within the bar"""
    build, seed, spp, _ = AC.SCENE_CASES[case]
    scene = build(str(tmp_path))
    integ = scene.integrator()
    integ.amd_mode = "auto"
    integ.deterministic = True
    a, b = _gpu(scene, spp, seed), _gpu(scene, spp, seed)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    AC.assert_matches_oracle(*a, AC.oracle_render(scene, seed, spp), case)


@pytest.mark.parametrize("mode", MODES)
def test_gpu_crop_window_one_spp_and_shards(mode):
    """a 13 x 9 film with a 9 x 6 crop window at offset (3, 2), 1 spp; then sample shards of 5 spp that sum to the whole"""
    import torch
    crop = {"width": 13, "height": 9, "crop_width": 9, "crop_height": 6, "crop_offset_x": 3, "crop_offset_y": 2}
    scene = AC.cornell(45, 25, film=crop)
    scene.integrator().amd_mode = mode
    s, t, c = _gpu(scene, 1, 14)
    AC.assert_matches_oracle(s, t, c, AC.oracle_render(scene, 14, 1), "crop 1 spp")
    assert s.shape[:2] == (6, 9) and np.all(t[6:] == 0) and np.all(t[:, 9:] == 0)
    spp = 5
    s_full, t_full, _ = _gpu(scene, spp, 15)
    integ, sens = scene.integrator(), scene.sensors()[0]
    passes = integ.prepare(scene, sens, 15, spp, [])
    for rng in ((0, 2), (2, 5)):
        integ.accumulate(scene, sens, passes, spp, spp_range=rng)
    torch.cuda.synchronize()
    s_a, t_a = (np.array(x) for x in sens.film().develop())
    assert rel_l2(t_a, t_full) <= 1e-6 and rel_l2(s_a, s_full) <= 1e-6
    ref = AC.oracle_render(scene, 15, spp)
    assert rel_l2(t_a, ref[1]) <= TOL and rel_l2(s_a, ref[0]) <= TOL


def test_gpu_staircase_auto_is_wavefront_in_hbm():
    """an angular cube emitter in staircase_like(tiles=6): AUTO resolves to the wavefront organisation (the scene walked in HBM)"""
    scene = AC.staircase()
    integ = scene.integrator()
    integ.amd_mode = "auto"
    _vs_oracle(scene, 8, 16, "staircase")
    assert integ.resolved_mode(scene, scene.sensors()[0], 8) == "wavefront"        # (mtr_render_plan, the film prepared)


def test_gpu_phasor_film_matches_oracle():
    """phasor_hdr_film with an angulararea luminaire against the oracle's phasor render"""
    import torch
    import mitransient_amd.mi as mi
    try:
        scene = AC.phasor(res=12)
        integ = scene.integrator()
        integ.collect_stats = True
        steady, ph = integ.render(scene, seed=17, spp=32)
        torch.cuda.synchronize()
        got = dict(integ.last_counters)
        sd = scene.data()
        assert sd.emitters[0].angular == 1
        from oracle import oracle as _o
        p = integ.render_params(scene.sensors()[0].film(), 17, 32)
        t, s4, cnt, (near, n_near) = _o.render(sd, p, use_bvh=True, near=True)
        ph_ref, s_ref = _o.develop(sd.film, t, s4)
        assert np.abs(np.array(ph_ref)).max() > 0
        assert rel_l2(np.array(ph), ph_ref) <= TOL and rel_l2(np.array(steady)[..., 0], s_ref[..., 0]) <= TOL
        for k in COUNTERS:
            assert abs(got[k] - cnt[k]) <= n_near, k
    finally:
        mi.set_variant("llvm_ad_rgb")
