"""Reverse-mode gradients of transient_nlos_path (mtr_render_grad on a NLOS scene; mtr_grad.h: grad_nlos_lane): the host build of
the replay walk (tests/host_grad_nlos.cpp) against the unchanged CPU oracle at the same seed, and the Python surface.  No GPU needed;
tests/grad_nlos_gpu_cases.py holds the kernel to the same references.

(FD)        With rr_depth > max_depth and max_depth 4 the seeded loss is a polynomial of degree <= 4 in every albedo channel (a term
            of loop depth k <= 2 carries k + 1 vertices, and one more — the laser spot — under laser sampling): the slope at `a` of
            the quartic fitted to the oracle's loss is exact.  Two fits on different abscissae measure what the oracle's f32 sums
            leave in such a slope (test_the_oracles_own_fits_agree); the fit's residual shows that no term crossed a dr.epsilon
            cut-off between abscissae.
(Laser)     The estimator is linear in each irradiance channel: its gradient is the oracle's loss with that channel alone at 1.
(RR-degree) sum_m a_m d loss / d a_m = sum_c w_c c N(c) with roulette active, N(c) from the oracle's splat log alone:
            nlos_bounce (mtr_nlos.h) emits the term of loop depth k — the depth the log records — at vertex k of the path, after k
            sampling weights (vertices 0 .. k - 1 in beta) and the BSDF value of vertex k: k + 1 albedo factors; under
            nlos_laser_sampling the term is connected through the laser spot c2, whose BSDF value is one more: N = depth + 1
            (+ 1 with laser sampling) in an all-diffuse scene.
Every comparison also rejects the gradient scaled by 1 + 2e-4."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import test_grad as T
from conftest import make_nlos, make_nlos_camera, make_nlos_z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIDDEN = [0.7, 0.5, 0.6]           # albedos well away from 0 (the dr.epsilon cut-offs) and from each other
RELAY = [0.8, 0.6, 0.7]


def build_host_grad_nlos():
    """tests/host_grad_nlos.cpp with the flags of test_grad.build_host_grad()"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_grad_nlos.so")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "host_grad_nlos.cpp"), os.path.join(csrc, "mtr_scene_host.cpp"), os.path.join(csrc, "mtr_bvh.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mtr_core.h", "mtr_nlos.h", "mtr_grad.h", "mtr_scene_host.h", "mtr_bvh.h", "mtr_knobs.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-DMTR_EXPERIMENTS", "-o", tmp] + srcs, check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hgn():
    return C.CDLL(build_host_grad_nlos())


def diffuse(rgb):
    return {"type": "diffuse", "reflectance": {"type": "rgb", "value": list(rgb)}}


def side_mirror():
    """a rough conductor beside the hidden quad: a microfacet lobe elsewhere on the paths (the extended shading code)"""
    from mitransient_amd.transform import ScalarTransform4f as X
    return {"side": {"type": "rectangle", "to_world": X().translate([0.7, 0.0, 0.5]).rotate([0, 1, 0], -90).scale(0.5),
                     "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": 0.3}}}


# case: make_nlos arguments (max_depth 4, rr_depth 5 unless the case says otherwise); "camera": make_nlos_camera
LS, HG = "nlos_laser_sampling", "nlos_hidden_geometry_sampling"
FD_CASES = {
    "confocal_ls_hg": dict(capture="confocal", **{LS: True, HG: True}),
    "single_ls_hg": dict(capture="single", **{LS: True, HG: True}),
    # (without laser sampling a vertex is lit only inside the projector's cone: a wide one)
    "confocal_plain": dict(capture="confocal", laser_fov=90.0, **{LS: False, HG: False}),
    "single_ls": dict(capture="single", **{LS: True, HG: False}),
    "confocal_hg_coin": dict(capture="confocal", laser_fov=90.0, **{LS: False, HG: True}, nlos_hidden_geometry_sampling_do_rroulette=True),
    "single_hg_wall": dict(capture="single", **{LS: True, HG: True}, nlos_hidden_geometry_sampling_includes_relay_wall=True),
    "confocal_wall_coin": dict(capture="confocal", laser_fov=90.0, **{LS: False, HG: True}, nlos_hidden_geometry_sampling_do_rroulette=True,
                               nlos_hidden_geometry_sampling_includes_relay_wall=True),
    "first_last": dict(capture="confocal", **{LS: True, HG: True}, account_first_and_last_bounces=True, start=2.4),
    "filter_depth": dict(capture="confocal", **{LS: True, HG: True}, filter_depth=3),
    # (transient_nlos_path reads `discard_direct_paths`, transientnlospath.py:217, :491; `discard_direct_light` is the base class's)
    "discard_direct": dict(capture="single", **{LS: True, HG: True}, discard_direct_paths=True, discard_direct_light=True),
    "twosided": dict(capture="confocal", **{LS: True, HG: True}, hidden_bsdf={"type": "twosided", "bsdf": diffuse(HIDDEN)}),
    "is_confocal_meter": dict(capture="single", **{LS: True, HG: True}, sensor_extra={"is_confocal": True}),
    "rough_side": dict(capture="confocal", **{LS: True, HG: True}, scene_extra="side_mirror"),
    "z_bars": dict(capture="confocal", hidden="z", **{LS: True, HG: True}),
    "camera": "camera",
}


def nlos_scene(case, max_depth=4, rr_depth=5, **over):
    """the scene of a case: 8 x 8 pixels (Confocal, Single), 4 x 4 with the camera sensor; the hidden object HIDDEN, the wall RELAY"""
    kw = FD_CASES[case] if isinstance(case, str) else dict(case)
    T._mi()                                                     # (make_nlos_camera leaves the variant to its caller)
    if kw == "camera":
        scene = make_nlos_camera(res=4, bins=64, max_depth=max_depth, rr_depth=rr_depth, **over)
        set_albedo(scene, 0, [0.9, 0.7, 0.8])
        return scene
    kw = dict(kw)
    kw.setdefault("hidden_bsdf", diffuse(HIDDEN))
    if kw.get("scene_extra") == "side_mirror":
        kw["scene_extra"] = side_mirror()
    kw.update(over)
    kw = {**dict(sx=8, sy=8, bins=64, spp=4, max_depth=max_depth, rr_depth=rr_depth), **kw}
    scene = make_nlos(**kw)
    set_albedo(scene, relay_material(scene), RELAY)
    return scene


def relay_material(scene):
    sd = scene.data()
    return int(sd.tri_material[sd.shape_ranges[sd.relay_shape][0]])


def set_albedo(scene, m, rgb):
    sd = scene.data()
    for k in range(3):
        sd.materials[m].a[k] = np.float32(rgb[k])


def diffuse_materials(scene):
    sd = scene.data()
    return [m for m in range(sd.n_materials) if sd.materials[m].type == 0 and sd.materials[m].albedo_texture == 0]


def host_grad_nlos(hgn, scene, params, g_s, g_t):
    """the host build's (grad_materials (n, 3), grad_laser (3,)), f64"""
    sd = scene.data()
    f = sd.film
    gs_full = np.zeros((f.height, f.width, 3), np.float32)
    gs_full[:g_s.shape[0], :g_s.shape[1]] = g_s
    gt = np.ascontiguousarray(g_t, dtype=np.float32)
    gm = np.zeros((max(1, sd.n_materials), 3))
    gl = np.zeros(3)
    d = sd.desc()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    rc = hgn.hgn_render_grad(C.byref(d), C.byref(params), gs_full.ctypes.data_as(fp), gt.ctypes.data_as(fp),
                             gm.ctypes.data_as(dp), gl.ctypes.data_as(dp))
    assert rc == 0, rc
    return gm[:sd.n_materials], gl


def abscissae(a, which=0):
    """16 abscissae from a / 8 to a + 1 / 4 (test_grad.fd_material's wide fit), or — the second fit of the self-check — 12
    from a / 4 to a + 1 / 2; all positive, all exact in f32"""
    xs = np.linspace(a / 8, a + 0.25, 16) if which == 0 else np.linspace(a / 4, a + 0.5, 12)
    return xs.astype(np.float32).astype(np.float64)


def fit_slope(scene, params, g_s, g_t, m, k, which=0):
    """(slope at a, residual of the fit relative to the largest loss) of the quartic fitted to the oracle's loss over channel k of
    material m"""
    sd = scene.data()
    a = float(sd.materials[m].a[k])
    xs = abscissae(a, which)
    vals = []
    for x in xs:
        sd.materials[m].a[k] = x
        vals.append(T.oracle_loss(scene, params, g_s, g_t)[0])
    sd.materials[m].a[k] = a
    span = xs[-1] - xs[0]
    t = (xs - a) / span
    poly = np.poly1d(np.polyfit(t, vals, 4))
    resid = float(np.abs(poly(t) - vals).max() / max(np.abs(vals).max(), 1e-300))
    return float(np.polyder(poly)(0.0) / span), resid


def fd_gradients(scene, params, g_s, g_t, mats, which=0):
    out, worst = {}, 0.0
    for m in mats:
        row = []
        for k in range(3):
            s, r = fit_slope(scene, params, g_s, g_t, m, k, which)
            row.append(s)
            worst = max(worst, r)
        out[m] = np.array(row)
    return out, worst


# the residual of an exact quartic through f32 sums: the oracle's film and loss carry about 2^-24 per added term; a term that
# crossed a cut-off between abscissae would leave a step of the size of a term (1e-3 of the loss and more on these scenes)
RESIDUAL = 2e-6


def check_fd(hgn, case, gm=None):
    scene = nlos_scene(case)
    g_s, g_t = T.upstream(scene, "random")
    params = T.render_params(scene)
    if gm is None:
        gm, _ = host_grad_nlos(hgn, scene, params, g_s, g_t)
    mats = diffuse_materials(scene)
    assert mats
    fd, resid = fd_gradients(scene, params, g_s, g_t, mats)
    assert resid <= RESIDUAL, resid
    scale = max(np.abs(v).max() for v in fd.values())
    assert scale > 0 and np.all(np.isfinite(gm))
    worst = 0.0
    for m in mats:
        err = float(np.abs(gm[m] - fd[m]).max() / scale)
        worst = max(worst, err)
        print(f"[grad-nlos] {case} material {m}: host {gm[m]}, fit {fd[m]}, error {err:.2e} of the largest, residual {resid:.1e}")
        assert np.abs(fd[m]).max() > 0
        assert err <= 1e-4, (case, m, gm[m], fd[m])
    # the control: the same comparison sees a gradient scaled by 1 + 2e-4 (on the material that carries the largest element)
    big = max(mats, key=lambda m: np.abs(fd[m]).max())
    assert np.abs(gm[big] * (1 + 2e-4) - fd[big]).max() / scale > 1e-4, (gm[big], fd[big])
    return worst, scene


@pytest.mark.parametrize("case", ["confocal_ls_hg", "single_ls_hg", "camera"])
def test_the_oracles_own_fits_agree(case):
    """two fits of the oracle's loss on different abscissae: their slopes differ by less than 1e-5 of the largest gradient
    element — a tenth of (FD)'s bound, so that f32 rounding in the oracle cannot decide (FD)"""
    scene = nlos_scene(case)
    g_s, g_t = T.upstream(scene, "random")
    params = T.render_params(scene)
    mats = diffuse_materials(scene)
    a, ra = fd_gradients(scene, params, g_s, g_t, mats, 0)
    b, rb = fd_gradients(scene, params, g_s, g_t, mats, 1)
    scale = max(np.abs(v).max() for v in a.values())
    worst = max(float(np.abs(a[m] - b[m]).max()) for m in mats) / scale
    print(f"[grad-nlos] {case}: the oracle's two fits disagree by {worst:.2e} of the largest gradient; residuals {ra:.1e}, {rb:.1e}")
    assert worst <= 1e-5, worst
    assert max(ra, rb) <= RESIDUAL


@pytest.mark.parametrize("case", list(FD_CASES))
def test_albedo_gradients_match_the_oracles_polynomial(hgn, case):
    t0 = time.time()
    worst, scene = check_fd(hgn, case)
    sd = scene.data()
    if case != "camera":
        gm, _ = host_grad_nlos(hgn, scene, T.render_params(scene), *T.upstream(scene, "random"))
        relay = relay_material(scene)
        assert np.all(gm[relay] != 0.0) and any(np.all(gm[m] != 0.0) for m in diffuse_materials(scene) if m != relay)
    if case == "rough_side":
        from scene_class_cases import host_class
        import __graft_entry__ as g
        assert host_class(C.CDLL(g.build_host_harness()), scene)[1] == 1               # the extended shading code
        assert any(sd.materials[m].type != 0 for m in range(sd.n_materials))
    print(f"[grad-nlos] FD {case}: worst {worst:.2e} ({time.time() - t0:.1f} s)")


def laser_coefficients(scene, params, g_s, g_t):
    """(3,): the oracle's loss with channel k of the laser's irradiance at 1 and the others at 0"""
    laser = scene.emitters()[0]
    saved = list(laser.irradiance)
    ref = np.zeros(3)
    try:
        for k in range(3):
            laser.irradiance = [1.0 if j == k else 0.0 for j in range(3)]
            ref[k] = T.oracle_loss(scene, params, g_s, g_t)[0]
    finally:
        laser.irradiance = saved
    return ref


LASER_CASES = ["confocal_ls_hg", "single_hg_wall", "single_ls", "confocal_plain", "confocal_hg_coin", "first_last", "rough_side", "camera"]


@pytest.mark.parametrize("rr", [False, True], ids=["no_roulette", "roulette"])
@pytest.mark.parametrize("case", LASER_CASES)
def test_laser_gradient_is_the_oracles_linear_coefficient(hgn, case, rr):
    scene = nlos_scene(case, max_depth=8, rr_depth=2) if rr else nlos_scene(case)
    scene.emitters()[0].irradiance = [3.0, 0.0, 1.5]          # a zero channel still has its gradient
    g_s, g_t = T.upstream(scene, "random")
    params = T.render_params(scene)
    _, gl = host_grad_nlos(hgn, scene, params, g_s, g_t)
    ref = laser_coefficients(scene, params, g_s, g_t)
    assert np.all(ref != 0.0)
    err = np.abs(gl - ref) / np.abs(ref)
    print(f"[grad-nlos] laser {case} rr={rr}: host {gl}, oracle {ref}, error {err.max():.2e}")
    assert np.all(err <= 1e-5), (gl, ref)
    assert not np.all(np.abs(gl * (1 + 2e-4) - ref) <= 1e-5 * np.abs(ref))


def degree_sides(scene, params, g_t, grad_materials, laser_sampling, offset=0, log_capacity=1 << 22):
    """(sum_m a_m grad_m, sum_c w_c c N(c), terms) per channel for g_s = 0: the log holds every term the loss weighs"""
    from oracle import oracle
    sd = scene.data()
    f = sd.film
    _, _, cnt, log = oracle.render(sd, params, use_bvh=True, log_capacity=log_capacity)
    assert len(log) == cnt["splats_issued"] < log_capacity
    depth = (log["depth_kind"] & 0xffff).astype(np.int64)
    n = depth + 1 + (1 if laser_sampling else 0) + offset
    val = np.stack([log["r"], log["g"], log["b"]], 1).astype(np.float64)
    w = g_t.reshape(f.height * f.width, f.temporal_bins, 3)[log["pixel"], log["bin"]].astype(np.float64)
    rhs = (w * val * n[:, None]).sum(0)
    parts = np.array([[sd.materials[m].a[k] for k in range(3)] * np.asarray(grad_materials[m], np.float64)
                      for m in range(sd.n_materials)])
    return parts.sum(0), rhs, np.abs(parts).max(0), (int(depth.min()), int(depth.max()), len(log))


# case: laser sampling.  (Hidden-geometry sampling without the relay wall among its shapes ends a path at the hidden object: the
# cases here reach deep vertices through BSDF sampling, the coin, or the wall among the sampled shapes)
DEGREE_CASES = {"single_hg_wall": True, "single_ls": True, "confocal_plain": False, "confocal_wall_coin": False}


def degree_scene(case, max_depth):
    """roulette from the second bounce; a long film window (256 bins of 0.25) so that the deep terms are weighed too"""
    return nlos_scene(case, max_depth=max_depth, rr_depth=2, bins=256, bin_width=0.25, start=0.0, spp=64)


@pytest.mark.parametrize("max_depth", [12, -1])
@pytest.mark.parametrize("case", list(DEGREE_CASES))
def test_albedo_gradients_have_the_degree_of_the_detached_estimator(hgn, case, max_depth):
    scene = degree_scene(case, max_depth)
    sd = scene.data()
    assert all(sd.materials[m].type == 0 for m in range(sd.n_materials))
    g_s, g_t = T.upstream(scene, "random")
    g_s[:] = 0
    params = T.render_params(scene, spp=64)
    assert params.rr_depth == 2 and params.max_depth == max_depth
    gm, _ = host_grad_nlos(hgn, scene, params, g_s, g_t)
    ls = DEGREE_CASES[case]
    lhs, rhs, _, (d0, d1, n_terms) = degree_sides(scene, params, g_t, gm, ls)
    print(f"[grad-nlos] degree {case} max_depth {max_depth}: {n_terms} terms, depths {d0}-{d1}, lhs {lhs}, rhs {rhs}")
    assert n_terms > 300 and d1 >= 3                                  # terms beyond the first roulette (rr_depth 2)
    assert np.all(np.abs(rhs) > 0)
    assert np.all(np.abs(lhs - rhs) <= 1e-5 * np.abs(rhs)), (lhs, rhs)
    assert not np.all(np.abs(lhs * (1 + 2e-4) - rhs) <= 1e-5 * np.abs(rhs))
    _, rhs1, _, _ = degree_sides(scene, params, g_t, gm, ls, offset=1)            # N + 1 is rejected
    assert np.all(np.abs(lhs - rhs1) > 0.1 * np.abs(rhs1)), (lhs, rhs1)


def test_zero_albedo_channel_is_finite(hgn):
    scene = nlos_scene("confocal_ls_hg")
    relay = relay_material(scene)
    set_albedo(scene, relay, [0.8, 0.0, 0.7])
    g_s, g_t = T.upstream(scene, "random")
    gm, gl = host_grad_nlos(hgn, scene, T.render_params(scene), g_s, g_t)
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gl))
    assert gm[relay, 1] == 0.0 and gm[relay, 0] != 0.0


# -- the Python surface --------------------------------------------------------------------------------------------------------
def test_keys_of_nlos_z_and_of_an_assembled_scene(tmp_path):
    import mitransient_amd as mitr
    mi = T._mi()
    from mitransient_amd.scenes import nlos_z
    p = mi.traverse(nlos_z(width=4, height=4, temporal_bins=64, bin_width_opl=0.03, spp=2))
    for k in ("relay_wall.bsdf.reflectance.value", "Z.bsdf.reflectance.value", "laser.irradiance.value"):
        assert k in p and len(p[k]) == 3, (k, sorted(p))
    scene = make_nlos_z(tmp_path, sx=4, sy=4, bins=64, bin_width=0.03, spp=2)      # shapes and the laser loaded on their own
    p = mi.traverse(scene)
    for k in ("relay_wall.bsdf.reflectance.value", "Z.bsdf.reflectance.value", "laser.irradiance.value"):
        assert k in p and len(p[k]) == 3, (k, sorted(p))
    assert p["laser.irradiance.value"] == [1.0, 1.0, 1.0]
    keys = scene.grad_keys()
    assert keys["laser.irradiance.value"] == ("emitter", 0)
    assert keys["relay_wall.bsdf.reflectance.value"][0] == keys["Z.bsdf.reflectance.value"][0] == "material"
    two = make_nlos(sx=4, sy=4, hidden_bsdf={"type": "twosided", "bsdf": diffuse(HIDDEN)})
    assert "hidden.bsdf.brdf_0.reflectance.value" in mi.traverse(two)
    cam = make_nlos_camera(res=4)
    assert {"wall.bsdf.brdf_0.reflectance.value", "hidden.bsdf.brdf_0.reflectance.value", "laser.irradiance.value"} <= set(mi.traverse(cam))


def test_update_changes_the_primal(hgn, oracle):
    mi = T._mi()
    scene = make_nlos(sx=4, sy=4, spp=2)
    params = T.render_params(scene, spp=2)
    before = oracle.render(scene.data(), params, use_bvh=True)[0].copy()
    p = mi.traverse(scene)
    p["hidden.bsdf.reflectance.value"] = [0.5, 0.25, 1.0]
    p["laser.irradiance.value"] = [2.0, 1.0, 1.0]
    p.update()
    sd = scene.data()
    hidden = scene.grad_keys()["hidden.bsdf.reflectance.value"][1]
    assert list(sd.materials[hidden].a) == [0.5, 0.25, 1.0]
    assert list(sd.nlos.laser_irradiance) == [2.0, 1.0, 1.0]
    assert mi.traverse(scene)["laser.irradiance.value"] == [2.0, 1.0, 1.0]
    after = oracle.render(sd, params, use_bvh=True)[0]
    assert before[..., :3].sum() > 0
    # third-bounce light (wall, hidden, wall) is linear in the hidden albedo and the irradiance: exactly 1.0, 0.25, 1.0
    sel = before[..., 0] > 0
    ratio = after[sel][:, :3] / before[sel][:, :3]
    assert np.allclose(np.median(ratio, axis=0), [1.0, 0.25, 1.0], rtol=1e-5)


def _grad(key="hidden.bsdf.reflectance.value"):
    import torch
    return {key: torch.tensor([0.5, 0.4, 0.3], requires_grad=True)}


def _refused(scene, params, match):
    with pytest.raises(ValueError, match=match):
        scene.integrator().check_grad_(scene, 0, params)
    assert not scene._handles                                   # before any GPU work


def test_refusals():
    import torch
    mi = T._mi()
    scene = make_nlos(sx=4, sy=4)
    assert set(scene.integrator().check_grad_(scene, 0, _grad())) >= {"hidden.bsdf.reflectance.value", "laser.irradiance.value"}
    _refused(scene, {"sensor.film.start_opl": torch.tensor(3.0, requires_grad=True)}, "not a differentiable parameter")
    _refused(scene, {"laser.scale": torch.tensor(3.0, requires_grad=True)}, "not a differentiable parameter")
    _refused(scene, {"hidden.bsdf.reflectance.data": torch.zeros((2, 2, 3), requires_grad=True)}, "transient_path only")
    ex = make_nlos(sx=4, sy=4, capture="exhaustive", film={"exhaustive_scan": True, "laser_scan_width": 4, "laser_scan_height": 4})
    _refused(ex, _grad(), "[Ee]xhaustive")
    ex2 = make_nlos(sx=4, sy=4, film={"exhaustive_scan": True, "laser_scan_width": 4, "laser_scan_height": 4})
    _refused(ex2, _grad(), "exhaustive_scan")
    for v in ("llvm_ad_mono",):
        mi.set_variant(v)
        try:
            _refused(scene, _grad(), "_ad_rgb")
        finally:
            mi.set_variant("llvm_ad_rgb")
    mi.set_variant("llvm_ad_mono_polarized")
    try:
        with pytest.raises(ValueError, match="_ad_rgb|polarized"):
            scene.integrator().check_grad_(scene, 0, _grad())
    finally:
        mi.set_variant("llvm_ad_rgb")
    with pytest.raises(NotImplementedError):
        scene.integrator().render_forward(scene, _grad())
    # a transient_nlos_path integrator on a scene without a projector
    from mitransient_amd.integrators.transientnlospath import TransientNLOSPath
    with pytest.raises(ValueError, match="transient_nlos_path"):
        TransientNLOSPath.check_grad_(object.__new__(TransientNLOSPath), T.cornell(), 0, {})


# -- the Adam fit of tests/grad_nlos_gpu_cases.py, rehearsed on the CPU -------------------------------------------------------------
ADAM_BAND = 0.02     # |final - true| per channel; set from the rehearsal below (oracle primal + host-build gradients), not from a GPU run


def adam_rehearsal(hgn, tmp_path):
    """grad_nlos_gpu_cases.adam() with the oracle as the primal and the host build as render_backward, at mi.render's seeds"""
    import torch
    from oracle import oracle
    import grad_nlos_gpu_cases as G
    from mitransient_amd.mi import _tea32
    scene = make_nlos_z(tmp_path, **G.ADAM)
    key = "Z.bsdf.reflectance.value"
    m = scene.grad_keys()[key][1]
    sd = scene.data()
    f = sd.film

    def primal(seed, spp):
        t4, s4, _ = oracle.render(sd, T.render_params(scene, seed=seed, spp=spp), use_bvh=True)
        return oracle.develop(f, t4, s4)[0]

    set_albedo(scene, m, G.ADAM_TRUE)
    target = primal(100, 256)
    x = torch.tensor(G.ADAM_START, requires_grad=True)
    opt = torch.optim.Adam([x], lr=G.ADAM_LR)
    hist, losses = [], []
    for it in range(G.ADAM_STEPS):
        opt.zero_grad()
        set_albedo(scene, m, x.detach().numpy())
        t = primal(it + 1, G.ADAM_SPP)
        losses.append(float(np.sum((t.astype(np.float64) - target) ** 2)))
        g_t = (2.0 * (t - target)).astype(np.float32)
        g_s = np.zeros((f.height, f.width, 3), np.float32)
        gm, _ = host_grad_nlos(hgn, scene, T.render_params(scene, seed=_tea32(it + 1, 1), spp=G.ADAM_SPP), g_s, g_t)
        x.grad = torch.from_numpy(gm[m].astype(np.float32))
        opt.step()
        with torch.no_grad():
            x.clamp_(0.01, 1.0)
        hist.append([float(v) for v in x.detach()])
    return hist, losses


def test_adam_rehearsal_on_the_cpu(hgn, tmp_path):
    import grad_nlos_gpu_cases as G
    hist, losses = adam_rehearsal(hgn, tmp_path)
    thirds = [float(np.mean(losses[i:i + 20])) for i in (0, 20, 40)]
    err = np.abs(np.array(hist[-1]) - G.ADAM_TRUE)
    print(f"[grad-nlos] adam rehearsal: final {hist[-1]}, error {err}, mean loss per 20 steps {thirds}")
    assert thirds[0] > thirds[1] > thirds[2]                # the loss decreases
    assert np.all(err <= ADAM_BAND / 2), (hist[-1], err)    # the band leaves the CPU run a factor of two
