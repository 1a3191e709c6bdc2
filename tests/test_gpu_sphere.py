"""mitsuba's analytic `sphere` on the MI355X: k_fused and the wavefront kernels against the host build of the same arithmetic
(tests/host_harness.cpp over mtr_core.h) at the same seed — scenes staged in LDS and walked in HBM, trees that are one leaf or
spheres only, the NLOS tier with a hidden ball, the polarized variant, gradients, a phasor film, deterministic rows and the scene
traits.  Films are 8 x 6 with 16 bins and 5 samples a pixel (240 lanes: no multiple of a wave), one case with 1031 samples."""
import numpy as np
import pytest

import delta_cases as DC
import sphere_cases as SC
from conftest import hh_render, make_nlos, rel_l2

pytestmark = pytest.mark.gpu
MODES = ["fused", "wavefront"]
TOL = 1e-5          # the bar of every GPU / CPU parity test here: the GPU adds a pixel's samples in another order
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
FILM = dict(width=8, height=6, temporal_bins=16)


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


def _same(host_harness, scene, spp, seed=0, min_nonzero=20):
    s, t, c = _gpu(scene, spp, seed)
    hs, ht, hc = _host(host_harness, scene, spp, seed)
    assert np.count_nonzero(ht) > min_nonzero
    assert rel_l2(t, ht) <= TOL and rel_l2(s, hs) <= TOL, (rel_l2(t, ht), rel_l2(s, hs))
    for k in COUNTERS:
        assert c[k] == hc[k], k
    return s, t


def _room(mode, **kw):
    d = SC.room_dict(**kw)
    d["integrator"]["amd_mode"] = mode
    return DC._mi().load_dict(d)


def _hbm(mode):
    """852 triangles (tests/test_gpu_parity.py's stand-in for the staircase): over the LDS scene budget, walked in HBM"""
    from mitransient_amd.scenes import staircase_like
    d = staircase_like(n_steps=12, balusters=2, tiles=6, spp=5, max_depth=12, **FILM)
    d["s_ball"] = {"type": "sphere", "center": [0.5, 0.5, -1.0], "radius": 0.4, "bsdf": {"type": "diffuse", "reflectance": DC.rgb(0.3, 0.6, 0.8)}}
    d["s_glass"] = {"type": "sphere", "center": [-0.8, 1.2, -0.5], "radius": 0.35, "bsdf": {"type": "dielectric", "int_ior": 1.5}}
    d["s_bulb"] = {"type": "sphere", "center": [0.3, 3.0, -1.5], "radius": 0.2,
                 "emitter": {"type": "area", "radiance": DC.rgb(90.0, 70.0, 40.0)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}}
    d["integrator"]["amd_mode"] = mode
    return DC._mi().load_dict(d)


# ---------------------------------------------------------------- LDS / HBM
@pytest.mark.parametrize("mode", MODES)
def test_lds_scene_matches_host(host_harness, mode):
    scene = _room(mode)
    sd = scene.data()
    assert sd.n_emitters == 2 and [sd.emitters[i].kind for i in range(2)] == [0, 3]
    _same(host_harness, scene, 5, seed=1)


@pytest.mark.parametrize("mode", MODES)
def test_hbm_scene_matches_host(host_harness, mode):
    scene = _hbm(mode)
    assert scene.data().tri_verts.shape[0] >= 850
    _same(host_harness, scene, 5, seed=2)
    integ = scene.integrator()
    integ.amd_mode = "auto"
    assert integ.resolved_mode(scene, scene.sensors()[0], 5) == "wavefront"              # the scene does not fit LDS


@pytest.mark.parametrize("mode", MODES)
def test_many_samples_take_several_trips(host_harness, mode):
    _same(host_harness, _room(mode, max_depth=3), 1031, seed=3)


# ---------------------------------------------------------------- tree edges
def _lone(mode):
    """the only shape is one emitting sphere: the root of every tree is a leaf"""
    d = {"type": "scene", "integrator": dict(SC.integ(2), amd_mode=mode),
         "sensor": DC._sensor(dict(FILM, start_opl=2.0, bin_width_opl=0.125), 5, origin=(0.0, -4.0, 0.0)),
         "ball": {"type": "sphere", "emitter": {"type": "area", "radiance": DC.rgb(*SC.L_BALL)}}}
    return DC._mi().load_dict(d)


def _nine(mode):
    """nine spheres and no triangle but their carriers"""
    d = {"type": "scene", "integrator": dict(SC.integ(4), amd_mode=mode),
         "sensor": DC._sensor(dict(FILM, start_opl=2.0, bin_width_opl=0.5), 5, origin=(0.0, -5.0, 0.5))}
    for k in range(9):
        i, j = k % 3 - 1, k // 3 - 1
        ball = {"type": "sphere", "center": [1.1 * i, 0.3 * (i + j), 1.1 * j], "radius": 0.3 + 0.05 * k}
        if k == 4:
            ball["emitter"] = {"type": "area", "radiance": DC.rgb(5.0, 6.0, 7.0)}
        elif k % 3 == 0:
            ball["bsdf"] = {"type": "dielectric", "int_ior": 1.5}
        elif k % 3 == 1:
            ball["bsdf"] = {"type": "conductor", "eta": 0.47, "k": 2.4}
        else:
            ball["bsdf"] = {"type": "diffuse", "reflectance": DC.rgb(0.2 + 0.08 * k, 0.5, 0.9 - 0.08 * k)}
        d[f"ball{k}"] = ball
    return DC._mi().load_dict(d)


@pytest.mark.parametrize("mode", MODES)
def test_root_is_a_sphere_leaf(host_harness, mode):
    _same(host_harness, _lone(mode), 5, seed=4)


@pytest.mark.parametrize("mode", MODES)
def test_nine_spheres_and_nothing_else(host_harness, mode):
    _same(host_harness, _nine(mode), 5, seed=5)


# ---------------------------------------------------------------- NLOS
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("capture", ["single", "confocal"])
def test_hidden_ball_matches_host(host_harness, capture, mode):
    scene = make_nlos(sx=6, sy=5, capture=capture, hidden=dict(SC.HIDDEN), spp=5, bins=16, bin_width=0.25, start=1.0, amd_mode=mode)
    _same(host_harness, scene, 5, seed=6, min_nonzero=8)


def test_hidden_ball_exhaustive_matches_host(host_harness):
    scene = make_nlos(sx=3, sy=2, capture="exhaustive", hidden=dict(SC.HIDDEN), spp=5, bins=16, bin_width=0.25, start=1.0,
                      film={"exhaustive_scan": True, "laser_scan_width": 3, "laser_scan_height": 2}, force_equal_illumination_scanning=True)
    s, t, c = _gpu(scene, 5, 7)
    _, ht, hc = _host(host_harness, scene, 5, 7)
    assert t.shape == (2, 3, 2, 3, 16, 3) and np.count_nonzero(ht) > 8
    assert rel_l2(t, ht) <= TOL, rel_l2(t, ht)
    # transient_hdr_film.py:213-214: the "steady" image of an exhaustive film is mean(transient, axis=-1)
    assert s.shape == t.shape[:-1] and np.allclose(s, t.mean(axis=-1), rtol=1e-6, atol=1e-12)
    for k in COUNTERS:
        assert c[k] == hc[k], k


# ---------------------------------------------------------------- polarized
def test_polarized_metal_ball_matches_host_build():
    import ctypes as C
    import mitransient_amd.mi as mi
    from test_polarized import build_host_polarized, hp_render
    try:
        mi.set_variant("llvm_ad_mono_polarized")
        d = SC.room_dict(balls=("metal",))
        d["integrator"]["amd_mode"] = "wavefront"
        scene = mi.load_dict(d)
        s, t, c = _gpu(scene, 5, 8)
        t4, s4, hc = hp_render(C.CDLL(build_host_polarized()), scene, seed=8, spp=5)
        with np.errstate(invalid="ignore", divide="ignore"):
            hs = np.where(s4[..., 3:] > 0, s4[..., :1] / s4[..., 3:], 0.0).astype(np.float32)
        assert rel_l2(t, t4) <= TOL and rel_l2(s, hs) <= TOL
        for k in range(4):                          # tests/test_gpu_polarized.py's bar per Stokes channel
            assert rel_l2(t[..., k], t4[..., k]) <= 1e-4, k
        assert np.abs(t[..., 1:]).max() > 0
        for k in COUNTERS:
            assert c[k] == hc[k], k
    finally:
        mi.set_variant("llvm_ad_rgb")


# ---------------------------------------------------------------- gradients
KEYS = ("ball.bsdf.reflectance.value", "bulb.emitter.radiance.value")


def _grad_scene():
    scene = _room("auto")
    f = scene.data().film
    rng = np.random.default_rng(5)
    import torch
    g_s = torch.from_numpy(rng.standard_normal((f.height, f.width, 3)).astype(np.float32)).cuda()
    g_t = torch.from_numpy(rng.standard_normal((f.height, f.width, f.temporal_bins, 3)).astype(np.float32)).cuda()
    return scene, g_s, g_t


def test_radiance_gradient_of_a_sphere_light_is_the_unit_render():
    """render_backward of <id>.emitter.radiance.value = sum g . render(unit radiance, the other light dark) at the same seed: the
    estimator is linear in the radiance; render_forward is its transpose"""
    import torch
    import mitransient_amd.mi as mi
    scene, g_s, g_t = _grad_scene()
    integ = scene.integrator()
    key, other = KEYS[1], "light.emitter.radiance.value"
    p = mi.traverse(scene)
    saved = {k: list(p[k]) for k in (key, other)}
    p[key], p[other] = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]
    p.update()
    u_s, u_t, _ = _gpu(scene, 5, 9)
    p[key], p[other] = saved[key], saved[other]
    p.update()
    u_s, u_t = u_s.astype(np.float64), u_t.astype(np.float64)
    assert np.count_nonzero(u_t) > 20
    want = (g_s.cpu().numpy().astype(np.float64) * u_s).sum((0, 1)) + (g_t.cpu().numpy().astype(np.float64) * u_t).sum((0, 1, 2))
    p = mi.traverse(scene)
    p[key] = torch.tensor(list(p[key]), requires_grad=True)
    got = integ.render_backward(scene, p, grad_in=(g_s, g_t), seed=9, spp=5)[key].cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (got, want)
    tan = torch.tensor([0.5, -2.0, 3.0])
    d_s, d_t = integ.render_forward(scene, p, seed=9, spp=5, tangents={key: tan})
    assert rel_l2(np.array(d_t), u_t * tan.numpy()) <= 1e-5 and rel_l2(np.array(d_s), u_s * tan.numpy()) <= 1e-5


def test_albedo_gradient_of_a_ball_and_its_transpose():
    """the albedo of the diffuse ball: <g, J v> of render_forward equals <J^T g, v> of render_backward on a random g and v"""
    import torch
    import mitransient_amd.mi as mi
    scene, g_s, g_t = _grad_scene()
    integ = scene.integrator()
    key = KEYS[0]
    p = mi.traverse(scene)
    assert key in p and KEYS[1] in p
    p[key] = torch.tensor(list(p[key]), requires_grad=True)
    grad = integ.render_backward(scene, p, grad_in=(g_s, g_t), seed=9, spp=5)[key].cpu().numpy().astype(np.float64)
    assert np.abs(grad).min() > 0
    tan = torch.tensor([0.5, -2.0, 3.0])
    d_s, d_t = integ.render_forward(scene, p, seed=9, spp=5, tangents={key: tan})
    lhs = (g_s.cpu().numpy().astype(np.float64) * np.array(d_s)).sum() + (g_t.cpu().numpy().astype(np.float64) * np.array(d_t)).sum()
    rhs = float((grad * tan.numpy()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_albedo_gradient_of_a_ball_is_the_difference_of_two_renders():
    """a diffuse ball under a sphere light and nothing else, max_depth 2: every path has one BSDF vertex, so the render is affine in the
    ball's albedo, R(a) = R(0) + a U with U = R(1) - R(0) at the same seed (R(0): the directly seen light alone), and render_backward
    of <id>.bsdf.reflectance.value = sum g . U — the value itself, not only its adjointness"""
    import torch
    import mitransient_amd.mi as mi
    d = {"type": "scene", "integrator": dict(SC.integ(2), amd_mode="auto"),
         "sensor": DC._sensor(dict(FILM, start_opl=3.0, bin_width_opl=0.5), 5, origin=(0.0, -4.0, 1.0), target=(0.0, 0.0, 0.3)),
         "ball": {"type": "sphere", "center": [0.0, 0.0, 0.0], "radius": 0.8, "bsdf": {"type": "diffuse", "reflectance": DC.rgb(0.3, 0.6, 0.8)}},
         "bulb": {"type": "sphere", "center": [0.9, -0.8, 1.3], "radius": 0.25,
                  "emitter": {"type": "area", "radiance": DC.rgb(9.0, 7.0, 4.0)}, "bsdf": {"type": "diffuse", "reflectance": 0.0}}}
    scene = DC._mi().load_dict(d)
    f = scene.data().film
    rng = np.random.default_rng(11)
    g_s = torch.from_numpy(rng.standard_normal((f.height, f.width, 3)).astype(np.float32)).cuda()
    g_t = torch.from_numpy(rng.standard_normal((f.height, f.width, f.temporal_bins, 3)).astype(np.float32)).cuda()
    key = KEYS[0]
    p = mi.traverse(scene)
    saved = list(p[key])
    renders = []
    for a in (1.0, 0.0):
        p[key] = [a, a, a]
        p.update()
        s, t, _ = _gpu(scene, 5, 9)
        renders.append((s.astype(np.float64), t.astype(np.float64)))
    p[key] = saved
    p.update()
    u_s, u_t = renders[0][0] - renders[1][0], renders[0][1] - renders[1][1]
    assert np.count_nonzero(u_t) > 20 and np.count_nonzero(renders[1][1]) > 0
    want = (g_s.cpu().numpy().astype(np.float64) * u_s).sum((0, 1)) + (g_t.cpu().numpy().astype(np.float64) * u_t).sum((0, 1, 2))
    p = mi.traverse(scene)
    p[key] = torch.tensor(list(p[key]), requires_grad=True)
    got = scene.integrator().render_backward(scene, p, grad_in=(g_s, g_t), seed=9, spp=5)[key].cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (got, want)


# ---------------------------------------------------------------- phasor film, deterministic rows, traits
def test_phasor_film_under_a_sphere_light_matches_host(host_harness):
    import torch
    import mitransient_amd.mi as mi
    from oracle import oracle as _o
    try:
        mi.set_variant("llvm_ad_mono")
        d = SC.room_dict(rect_light=False)
        d["sensor"]["film"] = {"type": "phasor_hdr_film", "width": 8, "height": 6, "wl_mean": 2.0, "wl_sigma": 1.0, "temporal_bins": 400,
                               "bin_width_opl": 0.05, "start_opl": 3.0, "rfilter": {"type": "box"}}
        scene = mi.load_dict(d)
        integ = scene.integrator()
        integ.collect_stats = True
        steady, ph = integ.render(scene, seed=6, spp=5)
        torch.cuda.synchronize()
        got = dict(integ.last_counters)
        sd = scene.data()
        p = integ.render_params(scene.sensors()[0].film(), 6, 5)
        t4, s4, cnt = hh_render(host_harness, sd, p)
        ph_ref, s_ref = _o.develop(sd.film, t4, s4)
        assert np.abs(np.array(ph_ref)).max() > 0
        assert rel_l2(np.array(ph), ph_ref) <= TOL and rel_l2(np.array(steady)[..., 0], s_ref[..., 0]) <= TOL
        for k in COUNTERS:
            assert got[k] == cnt[k], k
    finally:
        mi.set_variant("llvm_ad_rgb")


def test_deterministic_renders_are_bit_identical():
    scene = _room("auto")
    scene.integrator().deterministic = True                      # amd_deterministic: 64-bit fixed-point rows
    a = _gpu(scene, 5)
    b = _gpu(scene, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.count_nonzero(a[1]) > 20


def test_a_ball_takes_the_box_out_of_the_specialised_kernels():
    from mitransient_amd import _cabi
    special = (_cabi.MTR_TRAIT_ONE_RECT_EMITTER | _cabi.MTR_TRAIT_LEAF_PAIR | _cabi.MTR_TRAIT_FLAT_TOP | _cabi.MTR_TRAIT_FLAT_LEAVES |
               _cabi.MTR_TRAIT_GREY)
    plain = DC.cornell_scene(point=False, spot=False, boxes=True).gpu_traits()
    want = _cabi.MTR_TRAIT_DIFFUSE | _cabi.MTR_TRAIT_ONE_RECT_EMITTER | _cabi.MTR_TRAIT_LEAF_PAIR | _cabi.MTR_TRAIT_FLAT_TOP
    assert plain & want == want
    assert SC.room_scene(balls=("diffuse",), boxes=True).gpu_traits() & special == 0
    grey = make_nlos(sx=4, sy=4, capture="single")
    assert grey.gpu_traits() & _cabi.MTR_TRAIT_GREY
    assert make_nlos(sx=4, sy=4, capture="single", hidden=dict(SC.HIDDEN)).gpu_traits() & special == 0
