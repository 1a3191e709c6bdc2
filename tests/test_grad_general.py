"""mtr_render_grad beyond the diffuse, roulette-free Cornell box: the host build of mtr_grad.h against the unchanged CPU oracle
through three identities that hold exactly.

(FD)        With rr_depth > max_depth the seeded loss is a polynomial of degree < max_depth in every `diffuse` albedo channel
            whatever other materials the scene has (lobe sampling, Fresnel choices, MIS weights and emitter sampling do not read a
            diffuse reflectance): test_grad.py's five-point stencil stays exact on scenes with microfacet lobes, glass, smooth
            normals and bitmaps — the scenes that take grad_lane<true>.
(RR-const)  In a diffuse-only scene whose every albedo has blue = 1.0, max(beta) >= 1 on every path, so rr_prob == 0.95 for every
            value of the red and green channels: with roulette ACTIVE the loss is still a polynomial in those two channels.
(RR-degree) With sampling detached every term c is multilinear in the albedos at the vertices whose BSDF factor it carries, so per
            channel  sum_m a_m d loss / d a_m = sum_c w_c c N(c),  N(c) the number of such vertices: in a diffuse-only scene
            N = depth for an emission and depth + 1 for an emitter-sampling term, both in the oracle's splat log.  This is the
            detached semantics with rr_prob varying from vertex to vertex, computed without mtr_grad.h.
No GPU needed; tests/grad_gpu_cases.py holds the kernel to the same references."""
import time

import numpy as np
import pytest

import test_grad as T
from test_grad import hg  # noqa: F401  (the module's fixture: the host build of mtr_grad.h)
from scene_class_cases import host_class

SMALL = dict(width=16, height=16, temporal_bins=32, start_opl=3.5, bin_width_opl=0.1)
# Finite differences here are fd_material(wide=True).  With the a / 4 step of test_grad.py the red wall's 0.043 channel is
# differenced over 2^-7, and the f32 sums of the oracle's film then leave up to 1.04e-4 of the material's largest gradient in the
# finite difference itself (measured on the smooth-normals scene: 1.08168 over 2^-7, 1.08154 over 2^-4, 2^-3 and 2^-5, the host
# build 1.08154) — the size of the tolerance.  The wide fit is as exact for the polynomial and keeps that noise below 1e-5.
ROUGH = ["ggx", None, "aniso", "glass", "plastic"]
ROUGH_IDS = ["ggx", "beckmann-by-default", "anisotropic", "roughdielectric", "plastic-thindielectric"]


def rough_scene(distribution, max_depth=4, rr_depth=5, angular=False):
    from test_rough_bsdf import _rough_cornell
    d = _rough_cornell(distribution, **SMALL)
    d["integrator"].update(max_depth=max_depth, rr_depth=rr_depth)
    if angular:
        d["spot"] = T.angular_spot()
    return T._mi().load_dict(d)


def textured(tmp_path):
    """a bitmap-textured diffuse panel and crate in the Cornell box: the extended shading code, and two materials that get no gradient"""
    from test_textures import textured_scene
    scene = textured_scene(tmp_path, "diffuse", **SMALL)
    scene.integrator().max_depth, scene.integrator().rr_depth = 4, 5
    return scene


def smooth(tmp_path):
    """a diffuse `obj` ball with vertex normals in the Cornell box: smooth-shaded triangles"""
    from test_smooth_normals import sphere_scene
    scene = sphere_scene(tmp_path, **SMALL)
    scene.integrator().max_depth, scene.integrator().rr_depth = 4, 5
    return scene


def small_staircase(tiles=2, **integ):
    """the staircase stand-in: smooth conductors and a glass pane between diffuse walls, camera_unwarp, eta-scaled path lengths"""
    from mitransient_amd.scenes import staircase_like
    d = staircase_like(n_steps=4, balusters=1, tiles=tiles, width=16, height=16, temporal_bins=32)
    d["integrator"].update(max_depth=4, rr_depth=5)
    d["integrator"].update(integ)
    return T._mi().load_dict(d)


def material_keys(scene):
    return {k: i for k, (kind, i) in scene.grad_keys().items() if kind == "material"}


def check_all_materials(hg, scene, chans=(0, 1, 2), kind="random"):
    """check_materials on every differentiable material; every gradient non-zero; and the control: the same comparison rejects
    the same gradients scaled by 1 + 2e-4.  Returns the worst error relative to a material's largest finite difference."""
    g_s, g_t = T.upstream(scene, kind)
    mats = sorted(set(material_keys(scene).values()))
    assert mats
    report = {}
    gm = T.check_materials(hg, scene, g_s, g_t, mats=mats, chans=chans, report=report, wide=True)
    assert np.all(np.isfinite(gm))
    for m, (g, fd, err) in report.items():
        assert np.abs(g).max() > 0 and np.abs(fd).max() > 0, (m, g, fd)
        assert not T.within(g * (1 + 2e-4), fd, 1e-4), (m, g, fd)
    return max(err for _, _, err in report.values())


def _report(label, worst, t0):
    print(f"\n[grad] {label}: worst relative error {worst:.2e} ({time.time() - t0:.1f} s)")


# -- (FD) on mixed-material scenes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distribution", ROUGH, ids=ROUGH_IDS)
def test_albedo_gradients_in_a_scene_with_microfacet_lobes(hg, host_harness, distribution):
    t0 = time.time()
    scene = rough_scene(distribution)
    assert host_class(host_harness, scene)[1] == 1                      # grad_lane<true>
    assert len(material_keys(scene)) >= 3                               # white, red, green
    _report(f"FD rough-{distribution}", check_all_materials(hg, scene), t0)


def test_albedo_gradients_beside_a_bitmap_and_none_for_it(hg, host_harness, tmp_path):
    t0 = time.time()
    scene = textured(tmp_path)
    sd = scene.data()
    assert host_class(host_harness, scene)[1] == 1
    tex = [m for m in range(sd.n_materials) if sd.materials[m].albedo_texture != 0]
    assert tex
    keyed = set(i for _, i in scene.grad_keys().values())
    assert not keyed & set(tex)                                         # a textured reflectance is no differentiable parameter
    worst = check_all_materials(hg, scene)
    g_s, g_t = T.upstream(scene, "random")
    gm, _ = T.host_grad(hg, scene, T.render_params(scene), g_s, g_t)
    for m in tex:
        assert np.all(gm[m] == 0.0), (m, gm[m])                         # ... and receives no gradient
    _report("FD textured", worst, t0)


def test_albedo_gradients_with_smooth_shaded_triangles(hg, host_harness, tmp_path):
    t0 = time.time()
    scene = smooth(tmp_path)
    sd = scene.data()
    assert host_class(host_harness, scene)[1] == 1 and sd.tri_normals is not None
    ball = material_keys(scene)["ball.bsdf.reflectance.value"]
    worst = check_all_materials(hg, scene)
    g_s, g_t = T.upstream(scene, "random")
    gm, _ = T.host_grad(hg, scene, T.render_params(scene), g_s, g_t)
    assert np.all(gm[ball] != 0.0)                                      # the smooth-shaded material itself is differentiated
    _report("FD smooth normals", worst, t0)


def test_albedo_gradients_beside_smooth_conductors_and_glass(hg, host_harness):
    """staircase_like: specular chains between diffuse vertices, a dielectric pane (path lengths scaled by eta), camera_unwarp —
    through the plain shading code (no microfacet lobe, no vertex normal, no bitmap)"""
    from mitransient_amd import _cabi
    t0 = time.time()
    scene = small_staircase()
    sd = scene.data()
    assert host_class(host_harness, scene)[1] == 0
    types = {sd.materials[m].type for m in range(sd.n_materials)}
    assert {_cabi.MTR_BSDF_CONDUCTOR, _cabi.MTR_BSDF_DIELECTRIC} <= types
    _report("FD staircase_like", check_all_materials(hg, scene), t0)


# -- (RR-const) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr_depth", [1, 3])
def test_albedo_gradients_with_roulette_at_a_constant_probability(hg, oracle, rr_depth):
    t0 = time.time()
    scene = T.cornell(max_depth=5, rr_depth=rr_depth, blue=1.0)
    sd = scene.data()
    assert all(sd.materials[m].a[2] == 1.0 for m in set(material_keys(scene).values()))
    # roulette did end paths: fewer bounces than the same render without it
    params = T.render_params(scene)
    assert params.rr_depth == rr_depth and params.max_depth == 5
    with_rr = oracle.render(sd, params, use_bvh=True)[2]
    params.rr_depth = 6
    without = oracle.render(sd, params, use_bvh=True)[2]
    assert with_rr["paths"] == without["paths"] and with_rr["bounces"] < without["bounces"], (with_rr, without)
    _report(f"RR-const rr_depth {rr_depth}", check_all_materials(hg, scene, chans=(0, 1)), t0)


# -- (RR-degree) -------------------------------------------------------------------------------------------------------------
def degree_scene(max_depth, bins):
    """diffuse-only Cornell box, roulette from the second bounce, a film window [0, bins) that holds every term"""
    return T.cornell(bins=bins, start_opl=0.0, bin_width=1.0, max_depth=max_depth, rr_depth=2)


def degree_upstream(scene, kind):
    """test_grad.upstream's three shapes; one_bin: bin 6 alone (the bin a third of the way into this window is empty)"""
    g_s, g_t = T.upstream(scene, "random" if kind == "one_bin" else kind)
    if kind == "one_bin":
        g_s[:] = 0
        g_t[:, :, :6] = 0
        g_t[:, :, 7:] = 0
    return g_s, g_t


def degree_sides(scene, params, g_s, g_t, grad_materials, offset=0, log_capacity=1 << 20):
    """(sum_m a_m grad_m, sum_c w_c c N(c), the largest |a_m grad_m| summand) per channel, N from the oracle's splat log (+ offset
    for the control).  Every term must lie inside the film's window — the log holds the splats of the window only, the steady
    image every term — which is checked against a render of the same lanes over a window 1000 times as long."""
    from oracle import oracle
    sd = scene.data()
    f = sd.film
    _, _, cnt, log = oracle.render(sd, params, use_bvh=True, log_capacity=log_capacity)
    assert len(log) == cnt["splats_issued"] < log_capacity
    saved = f.bin_width_opl
    f.bin_width_opl = saved * 1000.0
    try:
        cnt_wide = oracle.render(sd, params, use_bvh=True)[2]
    finally:
        f.bin_width_opl = saved
    assert cnt_wide["splats_issued"] == cnt["splats_issued"] and cnt_wide["bounces"] == cnt["bounces"]
    assert np.all(log["opl"] >= f.start_opl) and np.all(log["opl"] < f.start_opl + f.temporal_bins * f.bin_width_opl)
    depth = (log["depth_kind"] & 0xffff).astype(np.int64)
    kind = log["depth_kind"] >> 16
    assert set(np.unique(kind)) <= {0, 1}
    n = np.where(kind == 0, depth, depth + 1) + offset
    val = np.stack([log["r"], log["g"], log["b"]], 1).astype(np.float64)        # the term times sample_scale (f32, as splatted)
    gs_full = np.zeros((f.height, f.width, 3), np.float32)
    gs_full[:g_s.shape[0], :g_s.shape[1]] = g_s
    w = gs_full.reshape(-1, 3)[log["pixel"]].astype(np.float64) \
        + g_t.reshape(f.height * f.width, f.temporal_bins, 3)[log["pixel"], log["bin"]].astype(np.float64)
    rhs = (w * val * n[:, None]).sum(0)
    parts = np.array([[sd.materials[m].a[k] for k in range(3)] * np.asarray(grad_materials[m], np.float64)
                      for m in range(sd.n_materials)])
    return parts.sum(0), rhs, np.abs(parts).max(0), (int(depth.min()), int(depth.max()), len(log))


@pytest.mark.parametrize("kind", ["random", "one_bin", "steady"])
@pytest.mark.parametrize("max_depth,bins", [(12, 64), (-1, 256)])
def test_albedo_gradients_have_the_degree_of_the_detached_estimator(hg, max_depth, bins, kind):
    t0 = time.time()
    scene = degree_scene(max_depth, bins)
    sd = scene.data()
    assert all(sd.materials[m].type == 0 and sd.materials[m].albedo_texture == 0 for m in range(sd.n_materials))
    params = T.render_params(scene)
    assert params.rr_depth == 2 and params.max_depth == max_depth
    g_s, g_t = degree_upstream(scene, kind)
    gm, _ = T.host_grad(hg, scene, params, g_s, g_t)
    lhs, rhs, _, (d0, d1, n_terms) = degree_sides(scene, params, g_s, g_t, gm)
    assert n_terms > 1000 and d0 == 0 and d1 >= 8                       # roulette active over many bounces
    assert np.all(np.abs(rhs) > 0)
    assert np.all(np.abs(lhs - rhs) <= 1e-5 * np.abs(rhs)), (lhs, rhs)
    # the control: a count of vertices off by one is seen
    _, rhs1, _, _ = degree_sides(scene, params, g_s, g_t, gm, offset=1)
    assert np.all(np.abs(lhs - rhs1) > 0.1 * np.abs(rhs1)), (lhs, rhs1)
    _report(f"RR-degree max_depth {max_depth} {kind} ({n_terms} terms, depths {d0}-{d1})", float(np.max(np.abs(lhs - rhs) / np.abs(rhs))), t0)


# -- emitter gradients, roulette active, microfacet lobes -----------------------------------------------------------------------
def test_emitter_gradients_are_the_linear_coefficients_with_lobes_and_roulette(hg, host_harness):
    t0 = time.time()
    scene = rough_scene("ggx", max_depth=6, rr_depth=2, angular=True)
    sd = scene.data()
    assert host_class(host_harness, scene)[1] == 1
    assert sd.n_emitters == 2 and sd.emitters[1].angular == 1
    g_s, g_t = T.upstream(scene, "random")
    params = T.render_params(scene)
    assert params.rr_depth == 2
    _, ge = T.host_grad(hg, scene, params, g_s, g_t)
    ref = T.emitter_coefficients(scene, params, g_s, g_t)
    assert np.all(ref != 0.0)
    assert np.all(np.abs(ge - ref) <= 1e-5 * np.abs(ref) + 1e-9), (ge, ref)
    _report("emitter coefficients rough-ggx", float(np.max(np.abs(ge - ref) / np.abs(ref))), t0)
