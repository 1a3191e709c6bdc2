"""mitsuba's `point` and `spot` emitters on the MI355X: k_fused and the wavefront kernels against the host build of the same
arithmetic (tests/host_harness.cpp over mtr_core.h) at the same seed, scenes staged in LDS and walked in HBM, the extended shading
code, the scene traits, gradients of the intensity, a phasor film and deterministic rows.  Films are 8 x 6 with 16 bins and 5
samples a pixel (240 lanes: no multiple of a wave), one case with 1031 samples for the grid-stride loops."""
import numpy as np
import pytest

import delta_cases as DC
from conftest import hh_render, rel_l2

pytestmark = pytest.mark.gpu
MODES = ["fused", "wavefront"]
TOL = 1e-5          # the bar of every GPU / CPU parity test here: the GPU adds a pixel's samples in another order
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
LIGHTS = {"point": dict(area=False, spot=False), "spot": dict(area=False, point=False), "three": dict()}
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


def _same(host_harness, scene, spp, seed=0):
    s, t, c = _gpu(scene, spp, seed)
    hs, ht, hc = _host(host_harness, scene, spp, seed)
    assert np.count_nonzero(ht) > 20
    assert rel_l2(t, ht) <= TOL and rel_l2(s, hs) <= TOL, (rel_l2(t, ht), rel_l2(s, hs))
    for k in COUNTERS:
        assert c[k] == hc[k], k
    return s, t


def _cornell(which, mode, max_depth=4, **kw):
    """the Cornell box with its two boxes (staged in LDS; the flat walk under the general shading code)"""
    d = DC.cornell_dict(boxes=True, res=(8, 6), spp=5, max_depth=max_depth, **LIGHTS[which], **kw)
    d["integrator"]["amd_mode"] = mode
    return DC._mi().load_dict(d)


def _lights(d, which):
    from mitransient_amd.transform import ScalarTransform4f as T
    if which in ("point", "three"):
        d["lamp"] = {"type": "point", "position": [-1.2, 2.6, 2.0], "intensity": DC.rgb(30.0, 20.0, 10.0)}
    if which in ("spot", "three"):
        d["beam"] = {"type": "spot", "to_world": T().look_at(origin=[2.0, 3.2, 3.0], target=[0.4, 1.0, 0.5], up=[0, 1, 0]),
                     "cutoff_angle": 35.0, "beam_width": 15.0, "intensity": DC.rgb(40.0, 60.0, 80.0)}
    if which != "three":
        del d["light"]
    return d


def _hbm(which, mode):
    """852 triangles (tests/test_gpu_parity.py's stand-in for the staircase): over the LDS scene budget, walked in HBM; conductors and
    glass beside the diffuse surfaces, Russian roulette from depth 5"""
    from mitransient_amd.scenes import staircase_like
    d = _lights(staircase_like(n_steps=12, balusters=2, tiles=6, spp=5, max_depth=12, **FILM), which)
    d["integrator"]["amd_mode"] = mode
    return DC._mi().load_dict(d)


# ---------------------------------------------------------------- G1
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(LIGHTS))
def test_lds_scene_matches_host(host_harness, mode, which):
    scene = _cornell(which, mode)
    assert scene.data().n_emitters == (3 if which == "three" else 1)
    _same(host_harness, scene, 5, seed=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(LIGHTS))
def test_hbm_scene_matches_host(host_harness, mode, which):
    scene = _hbm(which, mode)
    assert scene.data().tri_verts.shape[0] >= 850
    _same(host_harness, scene, 5, seed=2)
    integ = scene.integrator()
    integ.amd_mode = "auto"
    assert integ.resolved_mode(scene, scene.sensors()[0], 5) == "wavefront"              # the scene does not fit LDS


@pytest.mark.parametrize("mode", MODES)
def test_many_samples_take_several_trips(host_harness, mode):
    _same(host_harness, _cornell("three", mode, max_depth=3), 1031, seed=3)


# ---------------------------------------------------------------- G2
def _ext(tmp_path, which, mode):
    """a roughplastic floor and an obj with vertex normals: the <EXT> shading kernels, rough_eval_pdf under mis_em = 1"""
    d = DC.cornell_dict(boxes=False, res=(8, 6), spp=5, max_depth=4, **LIGHTS[which])
    d["integrator"]["amd_mode"] = mode
    d["floor"] = dict(d["floor"], bsdf={"type": "roughplastic", "alpha": 0.15, "diffuse_reflectance": DC.rgb(0.5, 0.3, 0.2)})
    d["bump"] = {"type": "obj", "filename": DC.obj_file(tmp_path),
                 "to_world": DC._T()().translate([0.1, -0.6, 0.1]).rotate([1, 0, 0], -70).scale(0.45), "bsdf": {"type": "ref", "id": "white"}}
    return DC._mi().load_dict(d)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(LIGHTS))
def test_extended_shading_matches_host(host_harness, tmp_path, mode, which):
    scene = _ext(tmp_path, which, mode)
    assert scene.data().tri_normals is not None
    _same(host_harness, scene, 5, seed=4)


# ---------------------------------------------------------------- G3
def test_one_rectangle_trait_never_with_a_delta_emitter():
    from mitransient_amd import _cabi
    plain = DC.cornell_scene(point=False, spot=False, boxes=True)
    assert plain.gpu_traits() & _cabi.MTR_TRAIT_ONE_RECT_EMITTER
    assert not (DC.cornell_scene(spot=False, boxes=True).gpu_traits() & _cabi.MTR_TRAIT_ONE_RECT_EMITTER)
    assert not (DC.cornell_scene(area=False, spot=False, boxes=True).gpu_traits() & _cabi.MTR_TRAIT_ONE_RECT_EMITTER)


# ---------------------------------------------------------------- G4
def _grad_scene():
    scene = _cornell("three", "auto", max_depth=4)
    f = scene.data().film
    rng = np.random.default_rng(5)
    import torch
    g_s = torch.from_numpy(rng.standard_normal((f.height, f.width, 3)).astype(np.float32)).cuda()
    g_t = torch.from_numpy(rng.standard_normal((f.height, f.width, f.temporal_bins, 3)).astype(np.float32)).cuda()
    return scene, g_s, g_t


KEYS = ("lamp.intensity.value", "beam.intensity.value", "light.emitter.radiance.value")


def _unit_render(scene, key, seed, spp):
    """the GPU's own primal with `key` at unit value and the other emitters dark: the render is linear in each of them"""
    import mitransient_amd.mi as mi
    p = mi.traverse(scene)
    saved = {k: list(p[k]) for k in KEYS}
    for k in KEYS:
        p[k] = [1.0, 1.0, 1.0] if k == key else [0.0, 0.0, 0.0]
    p.update()
    s, t, _ = _gpu(scene, spp, seed)
    for k in KEYS:
        p[k] = saved[k]
    p.update()
    return s.astype(np.float64), t.astype(np.float64)


@pytest.mark.parametrize("key", KEYS[:2])
def test_intensity_gradient_is_the_unit_render(key):
    """render_backward of <id>.intensity.value = sum g . render(unit intensity) at the same seed (the estimator is linear in the
    intensity: an identity, not an estimate), and render_forward is its transpose"""
    import torch
    import mitransient_amd.mi as mi
    scene, g_s, g_t = _grad_scene()
    integ = scene.integrator()
    u_s, u_t = _unit_render(scene, key, 9, 5)
    assert np.count_nonzero(u_t) > 20
    want = (g_s.cpu().numpy().astype(np.float64) * u_s).sum((0, 1)) + (g_t.cpu().numpy().astype(np.float64) * u_t).sum((0, 1, 2))
    p = mi.traverse(scene)
    p[key] = torch.tensor(list(p[key]), requires_grad=True)
    got = integ.render_backward(scene, p, grad_in=(g_s, g_t), seed=9, spp=5)[key].cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (got, want)
    tan = torch.tensor([0.5, -2.0, 3.0])
    d_s, d_t = integ.render_forward(scene, p, seed=9, spp=5, tangents={key: tan})
    assert rel_l2(np.array(d_t), u_t * tan.numpy()) <= 1e-5 and rel_l2(np.array(d_s), u_s * tan.numpy()) <= 1e-5


def test_autograd_through_mi_render_is_render_backward():
    import torch
    import mitransient_amd.mi as mi
    scene, g_s, g_t = _grad_scene()
    key = KEYS[0]
    p = mi.traverse(scene)
    x = torch.tensor([1.5, 1.0, 0.5], requires_grad=True)
    p[key] = x
    p.update()
    steady, transient = mi.render(scene, p, spp=5, seed=11, seed_grad=77, spp_grad=5)
    ((steady.torch() * g_s).sum() + (transient.torch() * g_t).sum()).backward()
    ref = scene.integrator().render_backward(scene, p, grad_in=(g_s, g_t), seed=77, spp=5)[key]
    assert x.grad.abs().min() > 0 and torch.equal(x.grad, ref.cpu())


# ---------------------------------------------------------------- G5
def test_phasor_film_of_a_point_lit_scene_matches_host(host_harness):
    import torch
    import mitransient_amd.mi as mi
    from oracle import oracle as _o
    try:
        mi.set_variant("llvm_ad_mono")
        d = DC.cornell_dict(area=False, spot=False, boxes=True, res=(8, 6), spp=5, max_depth=4)
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
    scene = _cornell("point", "auto")
    scene.integrator().deterministic = True                      # amd_deterministic: 64-bit fixed-point rows
    a = _gpu(scene, 5)
    b = _gpu(scene, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.count_nonzero(a[1]) > 20
