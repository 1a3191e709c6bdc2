"""Forward-mode derivatives of transient_path (mtr_render_fwd, mtr_fwd.h): the host build tests/host_fwd.cpp against the unchanged
CPU oracle at the same seed and against the host builds of the reverse mode (tests/host_grad.cpp, tests/host_grad_tex.cpp), and the
Python surface (render_forward's refusals).  All tolerances are the project's own (tests/test_grad*.py).

(FD)        With rr_depth > max_depth every cell of the oracle's film along  a + s v  — all parameters moved at once — is a
            polynomial in s of degree <= max_depth (at most max_depth - 1 albedo factors and one radiance): the slope at 0 of its
            least-squares fit is exact.  Tangent film within rel-L2 1e-4 of the slope; two fits on different abscissae agree
            within 1e-5.  Every abscissa keeps the albedos in (0, 1].
            (What stays positive are the ALBEDOS, not s: s runs over both signs on purpose — a departure from a fit on
            positive steps alone, because nodes on both sides of 0 condition the slope at 0 far better than an extrapolation
            from one side — and slope_film asserts that every albedo and texel it hands the oracle lies in (0, 1].)
(Linear)    dL_e = L_e, da = 0: the tangent film IS the primal film (1e-5), no fit.
(Degree)    da_m = a_m, dt = t, dL = 0: the tangent film is  sum_c N(c) c  from the oracle's splat log (1e-5), roulette active,
            max_depth 12; N + 1 is rejected.
(Duality)   sum g . (J v) = sum (J^T g) . v  with J^T g from the reverse mode's host builds, within 1e-5 of sum |g . J v|.
No GPU needed; tests/fwd_gpu_cases.py holds the kernel to the host build."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import test_grad as T
import test_grad_general as G
import test_grad_texture as X
from test_grad import hg  # noqa: F401  (host build of mtr_grad.h)
from test_grad_texture import hgt  # noqa: F401  (... with the texel hook)

ROOT = T.ROOT


def build_host_fwd():
    """tests/host_fwd.cpp with the flags of test_grad.build_host_grad()"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_fwd.so")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "host_fwd.cpp"), os.path.join(csrc, "mtr_scene_host.cpp"), os.path.join(csrc, "mtr_bvh.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mtr_core.h", "mtr_grad.h", "mtr_fwd.h", "mtr_scene_host.h", "mtr_bvh.h", "mtr_knobs.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-DMTR_EXPERIMENTS", "-o", tmp] + srcs, check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hf():
    return C.CDLL(build_host_fwd())


class Tangents:
    """tangents of a flattened scene: mats (n_materials, 3), ems (n_emitters, 3), texels [one (H, W, 3) per texture] or None"""

    def __init__(self, scene, mats=None, ems=None, texels=None):
        sd = scene.data()
        self.mats = np.zeros((sd.n_materials, 3), np.float32) if mats is None else np.asarray(mats, np.float32)
        self.ems = np.zeros((sd.n_emitters, 3), np.float32) if ems is None else np.asarray(ems, np.float32)
        self.texels = None if texels is None else [np.asarray(t, np.float32) for t in texels]

    def flat_texels(self):
        return None if self.texels is None else np.ascontiguousarray(np.concatenate([t.reshape(-1, 3) for t in self.texels]))


def albedos(scene):
    sd = scene.data()
    return np.array([[sd.materials[m].a[k] for k in range(3)] for m in range(sd.n_materials)], np.float32)


def radiances(scene):
    sd = scene.data()
    return np.array([[sd.emitters[e].radiance[k] for k in range(3)] for e in range(sd.n_emitters)], np.float32).reshape(-1, 3)


def host_fwd(hf, scene, params, tan):
    """the host build's developed tangent (steady (crop_h, crop_w, 3), transient (H, W, T, 3)), f64"""
    sd = scene.data()
    f = sd.film
    tm = np.zeros((max(1, sd.n_materials), 3), np.float32)
    tm[:sd.n_materials] = tan.mats
    te = np.zeros((max(1, sd.n_emitters), 3), np.float32)
    te[:sd.n_emitters] = tan.ems
    tx = tan.flat_texels()
    steady = np.full((f.height, f.width, 3), np.nan)
    transient = np.full((f.height, f.width, f.temporal_bins, 3), np.nan)
    n_out = C.c_uint64(0)
    d = sd.desc()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    rc = hf.hf_render_fwd(C.byref(d), C.byref(params), tm.ctypes.data_as(fp), te.ctypes.data_as(fp),
                          tx.ctypes.data_as(fp) if tx is not None else None,
                          steady.ctypes.data_as(dp), transient.ctypes.data_as(dp), C.byref(n_out))
    assert rc == 0
    if tx is not None:
        assert int(n_out.value) == len(tx)
    return steady[:f.crop_height, :f.crop_width].copy(), transient


def oracle_film(scene, params):
    """the oracle's developed (steady, transient), f64"""
    _, s3, t3 = T.oracle_loss(scene, params, np.zeros(1, np.float32), np.zeros(1, np.float32))
    return np.asarray(s3, np.float64), np.asarray(t3, np.float64)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def diffuse_constant(scene):
    sd = scene.data()
    return [m for m in range(sd.n_materials) if sd.materials[m].type == 0 and sd.materials[m].albedo_texture == 0]


def random_tangents(scene, seed=7, texels=False, lo=-1.0):
    """da = a u, dL = L u, dt = t u with u ~ U(lo, 1) per channel; materials other than plain `diffuse` get none"""
    rng = np.random.default_rng(seed)
    sd = scene.data()
    a = albedos(scene)
    tm = np.zeros_like(a)
    for m in diffuse_constant(scene):
        tm[m] = a[m] * rng.uniform(lo, 1.0, 3)
    te = radiances(scene) * rng.uniform(lo, 1.0, (sd.n_emitters, 3))
    tx = [t * rng.uniform(lo, 1.0, t.shape) for t in sd.textures] if texels else None
    return Tangents(scene, tm, te, tx)


# -- (FD) --------------------------------------------------------------------------------------------------------------------
# two sets of abscissae, |s| <= 0.4: a + s v stays in (0, 1] with fd_tangents' |v| <= min(a, 2.4 (1 - a)); slope_film asserts it
ABSCISSAE = (np.linspace(-0.4, 0.4, 12), np.linspace(-0.35, 0.3, 11))


def fd_tangents(scene, texels, seed=7):
    """random_tangents clipped so that every abscissa keeps the albedos in (0, 1]: |da| <= min(a, 2.4 (1 - a))"""
    tan = random_tangents(scene, seed, texels)
    a = albedos(scene)
    tan.mats = (np.sign(tan.mats) * np.minimum(np.abs(tan.mats), 2.4 * (1.0 - np.minimum(a, 1.0)))).astype(np.float32)
    if tan.texels is not None:
        sd = scene.data()
        tan.texels = [(np.sign(d) * np.minimum(np.abs(d), 2.4 * (1.0 - t))).astype(np.float32) for d, t in zip(tan.texels, sd.textures)]
    return tan


def slope_film(scene, params, tan, xs, degree):
    """the slope at s = 0 of the degree-`degree` least-squares fit of every cell of the oracle's film along  p + s tan"""
    sd = scene.data()
    a0, l0 = albedos(scene), radiances(scene)
    t0 = [t.copy() for t in sd.textures]
    mats = diffuse_constant(scene)
    films = []
    try:
        for s in xs:
            for m in mats:
                for k in range(3):
                    sd.materials[m].a[k] = float(np.float32(a0[m, k] + np.float32(s) * tan.mats[m, k]))
                    assert 0.0 < sd.materials[m].a[k] <= 1.0 or tan.mats[m, k] == 0.0
            for e in range(sd.n_emitters):
                for k in range(3):
                    sd.emitters[e].radiance[k] = float(np.float32(l0[e, k] + np.float32(s) * tan.ems[e, k]))
            if tan.texels is not None:
                for t, base, d in zip(sd.textures, t0, tan.texels):
                    t[...] = base + np.float32(s) * d
                    assert t.min() > 0.0 and t.max() <= 1.0
            st, tr = oracle_film(scene, params)
            films.append(np.concatenate([st.ravel(), tr.ravel()]))
    finally:
        for m in mats:
            for k in range(3):
                sd.materials[m].a[k] = float(a0[m, k])
        for e in range(sd.n_emitters):
            for k in range(3):
                sd.emitters[e].radiance[k] = float(l0[e, k])
        for t, base in zip(sd.textures, t0):
            t[...] = base
    # the abscissae as the oracle saw them (f32 steps)
    xs32 = np.asarray(xs, np.float32).astype(np.float64)
    coef = np.polyfit(xs32, np.stack(films), degree)
    n_s = scene.data().film.crop_height * scene.data().film.crop_width * 3
    return coef[-2][:n_s], coef[-2][n_s:]


def fd_scene(name, tmp_path):
    if name == "cornell":
        return T.cornell(), False
    if name == "ggx":
        return G.rough_scene("ggx"), False
    if name == "angulararea":
        return T.cornell(angular=True), False
    scene = G.textured(tmp_path)
    X.set_texels(scene, 0)
    return scene, True


@pytest.mark.parametrize("name", ["cornell", "ggx", "bitmap", "angulararea"])
def test_tangent_film_matches_the_oracles_polynomial(hf, tmp_path, name):
    t0 = time.time()
    scene, texels = fd_scene(name, tmp_path)
    integ = scene.integrator()
    assert integ.rr_depth > integ.max_depth == 4
    params = T.render_params(scene)
    tan = fd_tangents(scene, texels)
    assert np.abs(tan.mats).max() > 0 and np.abs(tan.ems).max() > 0 and (not texels or np.abs(tan.texels[0]).max() > 0)
    d_s, d_t = host_fwd(hf, scene, params, tan)
    fits = [slope_film(scene, params, tan, xs, integ.max_depth) for xs in ABSCISSAE]
    own = max(rel_l2(fits[0][0], fits[1][0]), rel_l2(fits[0][1], fits[1][1]))
    err = max(rel_l2(d_s, fits[0][0].reshape(d_s.shape)), rel_l2(d_t, fits[0][1].reshape(d_t.shape)))
    print(f"\n[fwd] FD {name}: tangent film within {err:.2e} of the fitted slope, the oracle's two fits within {own:.2e} "
          f"({time.time() - t0:.1f} s)")
    assert np.all(np.isfinite(d_s)) and np.all(np.isfinite(d_t)) and np.abs(fits[0][1]).max() > 0
    assert own <= 1e-5, own
    assert err <= 1e-4, err
    assert rel_l2(d_t * (1 + 2e-4), fits[0][1].reshape(d_t.shape)) > 1e-4


# -- (Linear) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "ggx-angulararea-roulette"])
def test_radiance_tangent_equal_to_the_radiance_gives_the_primal_film(hf, name):
    scene = T.cornell(angular=True) if name == "cornell" else G.rough_scene("ggx", max_depth=6, rr_depth=2, angular=True)
    params = T.render_params(scene)
    d_s, d_t = host_fwd(hf, scene, params, Tangents(scene, ems=radiances(scene)))
    s3, t3 = oracle_film(scene, params)
    err = max(rel_l2(d_s, s3), rel_l2(d_t, t3))
    print(f"\n[fwd] linearity {name}: {err:.2e}")
    assert np.abs(t3).max() > 0 and err <= 1e-5, err
    assert rel_l2(d_t * (1 + 2e-4), t3) > 1e-5


# -- (Degree) ----------------------------------------------------------------------------------------------------------------
def degree_film(scene, params, offset=0, log_capacity=1 << 20):
    """(steady, transient) =  sum_c N(c) c  per film cell from the oracle's splat log: N = depth for an emission, depth + 1 for an
    emitter-sampling term (diffuse-only scene; + offset for the control).  Every term lies inside the window (checked as
    test_grad_general.degree_sides does)."""
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
    depth = (log["depth_kind"] & 0xffff).astype(np.int64)
    kind = log["depth_kind"] >> 16
    assert set(np.unique(kind)) <= {0, 1}
    n = np.where(kind == 0, depth, depth + 1) + offset
    val = np.stack([log["r"], log["g"], log["b"]], 1).astype(np.float64) * n[:, None]
    transient = np.zeros((f.height * f.width, f.temporal_bins, 3))
    np.add.at(transient, (log["pixel"], log["bin"]), val)
    steady = transient.sum(1).reshape(f.height, f.width, 3)[:f.crop_height, :f.crop_width]
    return steady, transient.reshape(f.height, f.width, f.temporal_bins, 3), (int(depth.min()), int(depth.max()), len(log))


@pytest.mark.parametrize("textured", [False, True], ids=["constants", "texels"])
def test_tangent_equal_to_the_parameters_counts_the_vertices(hf, tmp_path, textured):
    if textured:
        scene = X.wall_scene(tmp_path, 5, 3, walls=("back", "floor", "red-wall"), max_depth=12, rr_depth=2,
                             film=dict(bins=64, start_opl=0.0, bin_width=1.0))
        X.set_texels(scene, 0)
    else:
        scene = G.degree_scene(12, 64)
    sd = scene.data()
    assert all(sd.materials[m].type == 0 for m in range(sd.n_materials))
    params = T.render_params(scene)
    assert params.rr_depth == 2 and params.max_depth == 12
    a = albedos(scene)
    for m in range(sd.n_materials):
        if sd.materials[m].albedo_texture:
            a[m] = 0                                                    # (not read: the texels are the parameter)
    tan = Tangents(scene, mats=a, texels=[t.copy() for t in sd.textures] if textured else None)
    d_s, d_t = host_fwd(hf, scene, params, tan)
    r_s, r_t, (d0, d1, n_terms) = degree_film(scene, params)
    assert n_terms > 1000 and d0 == 0 and d1 >= 8
    err = max(rel_l2(d_s, r_s), rel_l2(d_t, r_t))
    print(f"\n[fwd] degree {'texels' if textured else 'constants'}: {err:.2e} ({n_terms} terms, depths {d0}-{d1})")
    assert err <= 1e-5, err
    w_s, w_t, _ = degree_film(scene, params, offset=1)
    assert rel_l2(d_t, w_t) > 0.1 and rel_l2(d_s, w_s) > 0.1


# -- (Duality) ---------------------------------------------------------------------------------------------------------------
def duality_scene(case, tmp_path):
    kw = {}
    if case in ("camera_unwarp", "discard_direct_light"):
        kw[case] = True
    if case == "camera_unwarp":
        kw["start_opl"] = 0.0
    if case == "crop":
        kw.update(crop=(10, 7, 3, 5))
    if case == "texels":
        scene = X.wall_scene(tmp_path, 4, 3, walls=("back", "floor"))
        X.set_texels(scene, 0)
        return scene
    scene = T.cornell(angular=case in ("constants-and-emitters", "zero-albedo-channel"), **kw)
    if case == "zero-albedo-channel":
        p = T._mi().traverse(scene)
        p["red.reflectance.value"] = [0.57, 0.0, 0.04]
        p.update()
    return scene


def duality_sides(hf, hg, hgt, scene, tan, g_s, g_t):
    """(sum g . (J v), sum |g . (J v)|, sum (J^T g) . v) in f64"""
    params = T.render_params(scene)
    d_s, d_t = host_fwd(hf, scene, params, tan)
    prod = np.concatenate([(g_s.astype(np.float64) * d_s).ravel(), (g_t.astype(np.float64) * d_t).ravel()])
    if tan.texels is not None:
        gm, ge, gx = X.host_grad_tex(hgt, scene, params, g_s, g_t)
        rhs = sum(float(np.sum(g * t.astype(np.float64))) for g, t in zip(gx, tan.texels))
    else:
        gm, ge = T.host_grad(hg, scene, params, g_s, g_t)
        rhs = 0.0
    rhs += float(np.sum(gm * tan.mats.astype(np.float64)) + np.sum(ge * tan.ems.astype(np.float64)))
    return float(prod.sum()), float(np.abs(prod).sum()), rhs, (d_s, d_t)


@pytest.mark.parametrize("case", ["constants-and-emitters", "texels", "zero-albedo-channel", "crop", "camera_unwarp",
                                  "discard_direct_light"])
def test_forward_and_reverse_mode_are_transposes(hf, hg, hgt, tmp_path, case):
    scene = duality_scene(case, tmp_path)
    # g ~ N(1, 1) and v ~ p U(-0.2, 1): both signs occur, and sum g . J v keeps a share of sum |g . J v| that the scaled control
    # can be told from (asserted below)
    g_s, g_t = T.upstream(scene, "random")
    g_s, g_t = g_s + 1.0, g_t + 1.0
    tan = random_tangents(scene, texels=case == "texels", lo=-0.2)
    lhs, mag, rhs, (d_s, d_t) = duality_sides(hf, hg, hgt, scene, tan, g_s, g_t)
    print(f"\n[fwd] duality {case}: |<g, J v> - <J^T g, v>| = {abs(lhs - rhs) / mag:.2e} of sum |g . J v| (<g, J v> is {abs(lhs) / mag:.2f} of it)")
    assert np.all(np.isfinite(d_s)) and np.all(np.isfinite(d_t)) and mag > 0
    assert np.abs(d_t).max() > 0 and np.abs(d_s).max() > 0
    assert abs(lhs - rhs) <= 1e-5 * mag, (lhs, rhs, mag)
    assert abs(lhs) > 0.1 * mag
    assert abs(lhs * (1 + 2e-4) - rhs) > 1e-5 * mag
    if case == "zero-albedo-channel":
        # a tangent on the zero channel alone moves nothing (the zero rule), and nothing is NaN
        red = scene.grad_keys()["red.reflectance.value"][1]
        only = Tangents(scene)
        only.mats[red, 1] = 1.0
        z_s, z_t = host_fwd(hf, scene, T.render_params(scene), only)
        assert np.all(z_s == 0.0) and np.all(z_t == 0.0)


# -- film and output ---------------------------------------------------------------------------------------------------------
def test_steady_is_the_sum_over_time_only_when_the_window_holds_every_term(hf):
    whole = T.cornell(bins=64, start_opl=0.0, bin_width=0.5)            # the window [0, 32) holds every term of max_depth 4
    tan = random_tangents(whole)
    d_s, d_t = host_fwd(hf, whole, T.render_params(whole), tan)
    assert np.abs(d_s).max() > 0 and rel_l2(d_t.sum(2), d_s) <= 1e-5
    cut = T.cornell(bins=8)
    c_s, c_t = host_fwd(hf, cut, T.render_params(cut), random_tangents(cut))
    assert rel_l2(c_t.sum(2), c_s) > 1e-2
    assert rel_l2(c_s, d_s) <= 1e-12                                    # ... and the steady tangent does not depend on the window


def test_max_depth_one_has_no_albedo_tangent(hf):
    scene = T.cornell(max_depth=1)
    a = albedos(scene)
    d_s, d_t = host_fwd(hf, scene, T.render_params(scene), Tangents(scene, mats=a))
    assert np.all(d_s == 0.0) and np.all(d_t == 0.0)
    e_s, e_t = host_fwd(hf, scene, T.render_params(scene), Tangents(scene, ems=radiances(scene)))
    assert np.abs(e_s).max() > 0 and np.all(np.isfinite(e_t))


def test_pixel_ranges_compose_and_leave_the_rest_alone(hf):
    scene = T.cornell()
    tan = random_tangents(scene)
    params = T.render_params(scene)
    full_s, full_t = host_fwd(hf, scene, params, tan)
    params.pixel_begin, params.pixel_end = 0, 100
    a_s, a_t = host_fwd(hf, scene, params, tan)
    params.pixel_begin, params.pixel_end = 100, 256
    b_s, b_t = host_fwd(hf, scene, params, tan)
    assert np.array_equal(a_s + b_s, full_s) and np.array_equal(a_t + b_t, full_t)
    assert np.all(a_t.reshape(256, -1)[100:] == 0) and np.all(b_t.reshape(256, -1)[:100] == 0)


# -- refusals ----------------------------------------------------------------------------------------------------------------
def _refused(scene, params, match, **kw):
    with pytest.raises(NotImplementedError, match=match):
        scene.integrator().render_forward(scene, params, **kw)
    assert not scene._handles                                           # before any GPU work


def test_render_forward_refusals():
    import torch
    import mitransient_amd as mitr
    from conftest import make_nlos
    mi = T._mi()
    tan = {"red.reflectance.value": torch.tensor([0.5, 0.1, 0.1])}
    for v in ("llvm_ad_mono", "llvm_ad_mono_polarized"):
        mi.set_variant(v)
        try:
            scene = mi.load_dict(mitr.cornell_box())
            _refused(scene, {}, "_ad_rgb", tangents=tan)
        finally:
            mi.set_variant("llvm_ad_rgb")
    for film_kw, match in (({"type": "phasor_hdr_film"}, "phasor"), ({"exhaustive_scan": True, "laser_scan_width": 2,
                                                                     "laser_scan_height": 2}, "exhaustive_scan")):
        d = mitr.cornell_box()
        d["sensor"]["film"].update(width=8, height=8, temporal_bins=8, **film_kw)
        if film_kw.get("type") == "phasor_hdr_film":
            d["sensor"]["film"].update(wl_mean=0.5, wl_sigma=0.2)
        _refused(mi.load_dict(d), {}, match, tangents=tan)
    _refused(make_nlos(sx=4, sy=4), {}, "transient_nlos_path", tangents={"hidden.bsdf.reflectance.value": torch.ones(3)})
    scene = T.cornell()
    _refused(scene, {}, "not a differentiable parameter", tangents={"sensor.film.start_opl": torch.tensor(1.0)})
    _refused(scene, {}, "not a differentiable parameter", tangents={"no.such.key": torch.ones(3)})
    _refused(scene, {"sensor.film.start_opl": torch.tensor(3.0, requires_grad=True)}, "not a differentiable parameter")
    _refused(scene, {}, "1 or 3 elements", tangents={"red.reflectance.value": torch.ones(2)})
    # a dual tensor on a key that is no parameter; one on a parameter passes the checks (and then needs a GPU)
    import torch.autograd.forward_ad as fwAD
    with fwAD.dual_level():
        _refused(scene, {"sensor.film.start_opl": fwAD.make_dual(torch.tensor(3.0), torch.tensor(1.0))}, "not a differentiable parameter")
        keys = scene.integrator().check_grad_(scene, 0, {"red.reflectance.value": fwAD.make_dual(torch.ones(3), torch.ones(3))})
        assert keys["red.reflectance.value"][0] == "material"
    # more than 2^32 lanes: the reference refuses multi-pass forward renders too (common.py:237-240)
    _refused(scene, {}, "several passes", tangents=tan, spp=2 ** 32 // 256 + 1)
    from mitransient_amd.distributed import DistributedRenderer
    with pytest.raises(NotImplementedError):
        object.__new__(DistributedRenderer).render_forward(scene, {}, tangents=tan)
