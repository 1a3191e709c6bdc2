"""Derivatives of transient_path with respect to the constant specular tints of conductors and dielectrics (mtr_render_grad_tint,
mtr_render_fwd_tint; the tint hooks of mtr_grad.h / mtr_fwd.h): the host build tests/host_tint.cpp against the unchanged CPU oracle
rendered at the same seed with the tint changed in the scene tables.

(FD)        With rr_depth > max_depth the seeded loss is a polynomial of degree <= max_depth in every tint channel (no sampling
            decision reads a tint): the slope of test_grad.py's least-squares quartic over 16 positive abscissae, within 1e-4 of the
            material's largest finite difference.
(Split)     Vertices on a roughdielectric whose emitter-sampling term carries another tint than the continued path occur.
(Linear)    With every tint of one material scaled together and the material met at most once per path, the loss is linear.
(Duality)   sum g . (J v) = sum (J^T g) . v between the forward and the reverse host build, roulette active.
(Unchanged) Without a tint pointer the new entry gives host_grad's albedo and emitter gradients bit for bit.
No GPU needed; tests/tint_gpu_cases.py holds the kernels of mtr_tint.hip to the same host build."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import test_grad as T
from test_grad import hg  # noqa: F401  (the module's fixture: the host build of mtr_grad.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(width=16, height=16, temporal_bins=32, start_opl=3.5, bin_width_opl=0.1)


def build_host_tint():
    """tests/host_tint.cpp with the flags of build_host_harness() (__graft_entry__.py)"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_tint.so")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "host_tint.cpp"), os.path.join(csrc, "mtr_scene_host.cpp"), os.path.join(csrc, "mtr_bvh.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mtr_core.h", "mtr_grad.h", "mtr_fwd.h", "mtr_scene_host.h", "mtr_bvh.h", "mtr_knobs.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-DMTR_EXPERIMENTS", "-o", tmp] + srcs, check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(build_host_tint())


COPPER = dict(eta=dict(type="rgb", value=[0.2, 0.92, 1.1]), k=dict(type="rgb", value=[3.9, 2.45, 2.14]))


# -- scenes ------------------------------------------------------------------------------------------------------------------
def rgb(*v):
    return dict(type="rgb", value=list(v))


def tint_scene(kind, max_depth=4, rr_depth=None, **film):
    """the Cornell box with its two boxes (and a pane) made of tinted conductors and dielectrics:
    smooth     a `conductor` small box, a `dielectric` large box — the plain shading code
    ggx        a `roughconductor` (ggx, anisotropic) small box, a `roughdielectric` (ggx) large box
    beckmann   a `roughconductor` (beckmann) small box, a `roughdielectric` (beckmann, anisotropic) large box
    pane       a `thindielectric` pane in front of the boxes, the large box a conductor inside `twosided`"""
    import mitransient_amd as mitr
    from mitransient_amd.transform import ScalarTransform4f as Tr
    mi = T._mi()
    d = mitr.cornell_box()
    d["integrator"].update(max_depth=max_depth, rr_depth=max(max_depth, 1) + 1 if rr_depth is None else rr_depth)
    d["sensor"]["film"].update(**{**SMALL, **film})
    refl, trans = rgb(0.9, 0.7, 0.5), rgb(0.6, 0.8, 0.95)
    if kind == "smooth":
        d["small-box"]["bsdf"] = dict(type="conductor", **COPPER, specular_reflectance=rgb(0.8, 0.9, 0.6))
        d["large-box"]["bsdf"] = dict(type="dielectric", int_ior=1.5, specular_reflectance=refl, specular_transmittance=trans)
    elif kind == "ggx":
        d["small-box"]["bsdf"] = dict(type="roughconductor", **COPPER, distribution="ggx", alpha_u=0.15, alpha_v=0.4,
                                      specular_reflectance=rgb(0.8, 0.9, 0.6))
        d["large-box"]["bsdf"] = dict(type="roughdielectric", distribution="ggx", alpha=0.3, int_ior=1.5,
                                      specular_reflectance=refl, specular_transmittance=trans)
    elif kind == "beckmann":
        d["small-box"]["bsdf"] = dict(type="roughconductor", **COPPER, distribution="beckmann", alpha=0.25,
                                      specular_reflectance=rgb(0.8, 0.9, 0.6))
        d["large-box"]["bsdf"] = dict(type="roughdielectric", distribution="beckmann", alpha_u=0.2, alpha_v=0.45, int_ior=1.5,
                                      specular_reflectance=refl, specular_transmittance=trans)
    elif kind == "pane":
        d["pane"] = dict(type="rectangle", to_world=Tr().translate([0.0, 0.0, 0.6]).scale([0.7, 0.7, 1.0]),
                         bsdf=dict(type="thindielectric", int_ior=1.5, specular_reflectance=refl, specular_transmittance=trans))
        d["large-box"]["bsdf"] = dict(type="twosided", bsdf=dict(type="conductor", **COPPER, specular_reflectance=rgb(0.8, 0.9, 0.6)))
    else:
        raise ValueError(kind)
    return mi.load_dict(d)


# -- the host build ----------------------------------------------------------------------------------------------------------
def _ptrs(scene, g_s, g_t):
    f = scene.data().film
    gs_full = np.zeros((f.height, f.width, 3), np.float32)
    gs_full[:g_s.shape[0], :g_s.shape[1]] = g_s
    return gs_full, np.ascontiguousarray(g_t, dtype=np.float32)


def host_tint_layout(ht, scene):
    """[(material, which)] of every slot (mtr_scene_tint_layout on the host)"""
    sd = scene.data()
    d = sd.desc()
    n = C.c_uint32(0)
    assert ht.ht_tint_layout(C.byref(d), C.byref(n), None, None) == 0
    m = np.zeros(max(1, n.value), np.uint32)
    w = np.zeros(max(1, n.value), np.uint32)
    assert ht.ht_tint_layout(C.byref(d), C.byref(n), m.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)) == 0
    return [(int(m[i]), int(w[i])) for i in range(n.value)]


def host_grad_tint(ht, scene, params, g_s, g_t, tints=True):
    """the host build's (grad_materials, grad_emitters, grad_tints (n_slots, 3), (tinted vertices, split vertices)), f64; tints
    False: a null tint pointer"""
    sd = scene.data()
    gs_full, gt = _ptrs(scene, g_s, g_t)
    n = len(host_tint_layout(ht, scene))
    gm = np.zeros((max(1, sd.n_materials), 3))
    ge = np.zeros((max(1, sd.n_emitters), 3))
    gx = np.zeros((max(1, n), 3))
    cnt = np.zeros(2, np.uint64)
    d = sd.desc()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    rc = ht.ht_render_grad_tint(C.byref(d), C.byref(params), gs_full.ctypes.data_as(fp), gt.ctypes.data_as(fp),
                                gm.ctypes.data_as(dp), ge.ctypes.data_as(dp), gx.ctypes.data_as(dp) if tints else None,
                                cnt.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return gm[:sd.n_materials], ge[:sd.n_emitters], gx[:n], (int(cnt[0]), int(cnt[1]))


def host_fwd_tint(ht, scene, params, tm, te, tt):
    """the host build's tangent film (steady (H, W, 3), transient (H, W, T, 3)), f64"""
    sd = scene.data()
    f = sd.film
    steady = np.zeros((f.height, f.width, 3))
    transient = np.zeros((f.height, f.width, f.temporal_bins, 3))
    d = sd.desc()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    arr = [np.ascontiguousarray(x, dtype=np.float32) for x in (tm, te, tt)]
    rc = ht.ht_render_fwd_tint(C.byref(d), C.byref(params), arr[0].ctypes.data_as(fp), arr[1].ctypes.data_as(fp), None,
                               arr[2].ctypes.data_as(fp) if tt is not None and len(tt) else None,
                               steady.ctypes.data_as(dp), transient.ctypes.data_as(dp))
    assert rc == 0
    return steady, transient


def tint_array(sd, m, which):
    return sd.materials[m].c2 if which else sd.materials[m].c


def fd_tint(scene, params, g_s, g_t, m, which, k):
    """test_grad.fd_material(wide=True) on channel k of a tint: the derivative at s of the quartic fitted by least squares to the
    oracle's loss at 16 positive abscissae from s / 8 to s + 1 / 4"""
    sd = scene.data()
    arr = tint_array(sd, m, which)
    s = float(arr[k])
    xs = np.linspace(s / 8, s + 0.25, 16).astype(np.float32).astype(np.float64)
    vals = []
    for x in xs:
        arr[k] = x
        vals.append(T.oracle_loss(scene, params, g_s, g_t)[0])
    arr[k] = s
    span = xs[-1] - xs[0]
    return float(np.polyder(np.poly1d(np.polyfit((xs - s) / span, vals, 4)))(0.0) / span)


# -- (FD) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "ggx", "beckmann", "pane"])
def test_tint_gradients_are_the_slopes_of_the_oracles_polynomial(ht, oracle, kind):
    """worst errors relative to a material's largest finite difference, measured: smooth 4.9e-7, ggx 1.9e-5, beckmann 8.5e-6,
    pane 2.8e-7 (bound 1e-4)"""
    t0 = time.time()
    scene = tint_scene(kind)
    params = T.render_params(scene)
    g_s, g_t = T.upstream(scene, "random")
    slots = host_tint_layout(ht, scene)
    keyed = set(scene.data().tint_params.values())
    assert keyed and keyed <= set(slots)
    _, _, gx, _ = host_grad_tint(ht, scene, params, g_s, g_t)
    assert np.all(np.isfinite(gx))
    worst = 0.0
    for m in sorted({m for m, _ in keyed}):
        mine = [(i, w) for i, (mm, w) in enumerate(slots) if mm == m and (mm, w) in keyed]
        g = np.concatenate([gx[i] for i, _ in mine])
        fd = np.array([fd_tint(scene, params, g_s, g_t, m, w, k) for _, w in mine for k in range(3)])
        err = float(np.abs(g - fd).max() / max(np.abs(fd).max(), 1e-12))
        print(f"\n[tint] FD {kind} material {m}: gradient {g}, fit {fd}, error {err:.2e}")
        # every tint of the material moves the loss (both lobes of a dielectric are met), in the fit and in the gradient
        assert np.all(np.abs(fd.reshape(-1, 3)).max(1) > 0) and np.all(np.abs(g.reshape(-1, 3)).max(1) > 0), (m, g, fd)
        assert T.within(g, fd, 1e-4), (m, g, fd)
        assert not T.within(g * (1 + 2e-4), fd, 1e-4), (m, g, fd)        # the control: the comparison sees a 2e-4 scaling
        worst = max(worst, err)
    print(f"[tint] FD {kind}: worst relative error {worst:.2e} ({time.time() - t0:.1f} s)")


# -- (Split) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ggx", "beckmann"])
def test_a_rough_dielectric_vertex_can_carry_two_tints(ht, kind):
    scene = tint_scene(kind)
    g_s, g_t = T.upstream(scene, "random")
    _, _, _, (n_vertices, n_split) = host_grad_tint(ht, scene, T.render_params(scene), g_s, g_t)
    print(f"\n[tint] split {kind}: {n_split} of {n_vertices} tinted vertices")
    assert n_vertices > 0 and n_split > 0


# -- (Linear) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,max_depth,boxes", [("smooth", 3, ("small-box",)), ("ggx", 2, ("small-box", "large-box"))])
def test_scaling_every_tint_of_a_material_met_once_is_linear(ht, oracle, kind, max_depth, boxes):
    """A path has at most one vertex on the material whose BSDF factor enters a term — max_depth 2: one such vertex per path, with
    its emitter-sampling term (rough lobes); max_depth 3 on the convex conductor box: a mirror lights nothing by emitter sampling and
    cannot see itself — so the loss is linear in the common scale t of the material's tints and  d loss / d t = sum s . grad_s  is
    the oracle's difference quotient between t = 1 and t = 1 / 2"""
    scene = tint_scene(kind, max_depth=max_depth)
    sd = scene.data()
    params = T.render_params(scene)
    # positive upstream gradients: every term adds to the loss with one sign, so a slope is no difference of large summands and
    # the oracle's f32 film sums leave their rounding at the scale of the slope itself
    g_s, g_t = (np.abs(g) for g in T.upstream(scene, "random"))
    slots = host_tint_layout(ht, scene)
    _, _, gx, _ = host_grad_tint(ht, scene, params, g_s, g_t)
    base = T.oracle_loss(scene, params, g_s, g_t)[0]
    for m in sorted({m for k, (m, _) in sd.tint_params.items() if k.split(".")[0] in boxes}):
        mine = [(i, w) for i, (mm, w) in enumerate(slots) if mm == m]
        saved = {w: [float(tint_array(sd, m, w)[k]) for k in range(3)] for _, w in mine}
        parts = np.concatenate([np.asarray(saved[w]) * gx[i] for i, w in mine])
        lhs = float(parts.sum())
        for _, w in mine:
            for k in range(3):
                tint_array(sd, m, w)[k] = saved[w][k] * 0.5
        half = T.oracle_loss(scene, params, g_s, g_t)[0]
        for _, w in mine:
            for k in range(3):
                tint_array(sd, m, w)[k] = saved[w][k]
        rhs = (base - half) / 0.5
        print(f"\n[tint] linear {kind} material {m}: {lhs} against {rhs}, relative {abs(lhs - rhs) / abs(rhs):.2e}, summands {parts}")
        assert rhs != 0.0 and abs(lhs - rhs) <= 1e-5 * abs(rhs), (m, lhs, rhs)
        assert abs(lhs * (1 + 1e-4) - rhs) > 1e-5 * abs(rhs), (m, lhs, rhs)        # the control: a slope off by 1e-4 is seen


# -- (Duality) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "beckmann", "pane"])
def test_forward_and_reverse_mode_are_transposes_with_roulette(ht, kind):
    scene = tint_scene(kind, max_depth=8, rr_depth=2)
    sd = scene.data()
    params = T.render_params(scene)
    assert params.rr_depth == 2 and params.max_depth == 8
    g_s, g_t = T.upstream(scene, "random")
    rng = np.random.default_rng(5)
    n = len(host_tint_layout(ht, scene))
    tm = rng.standard_normal((max(1, sd.n_materials), 3)).astype(np.float32)
    te = rng.standard_normal((max(1, sd.n_emitters), 3)).astype(np.float32)
    tt = rng.standard_normal((n, 3)).astype(np.float32)
    gm, ge, gx, _ = host_grad_tint(ht, scene, params, g_s, g_t)
    d_s, d_t = host_fwd_tint(ht, scene, params, tm, te, tt)
    gs_full, gt = _ptrs(scene, g_s, g_t)
    parts = np.concatenate([(gs_full.astype(np.float64) * d_s).reshape(-1), (gt.astype(np.float64) * d_t).reshape(-1)])
    lhs = parts.sum()
    rhs = float((gm * tm[:sd.n_materials]).sum() + (ge * te[:sd.n_emitters]).sum() + (gx * tt).sum())
    tints_part = float((gx * tt).sum())
    print(f"\n[tint] duality {kind}: {lhs} against {rhs} (tints {tints_part}), relative to sum |g . J v| {abs(lhs - rhs) / np.abs(parts).sum():.2e}")
    assert tints_part != 0.0
    assert abs(lhs - rhs) <= 1e-5 * np.abs(parts).sum()
    # the control: without the tint tangents the forward side misses the tints' part
    d_s0, d_t0 = host_fwd_tint(ht, scene, params, tm, te, None)
    lhs0 = float((gs_full.astype(np.float64) * d_s0).sum() + (gt.astype(np.float64) * d_t0).sum())
    assert abs(lhs0 - rhs) > 1e-5 * np.abs(parts).sum()


# -- (Unchanged) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "ggx"])
def test_albedo_and_emitter_gradients_without_a_tint_pointer_are_host_grads(ht, hg, kind):
    scene = tint_scene(kind)
    assert scene.tint_keys()
    params = T.render_params(scene)
    g_s, g_t = T.upstream(scene, "random")
    gm0, ge0 = T.host_grad(hg, scene, params, g_s, g_t)
    gm, ge, _, _ = host_grad_tint(ht, scene, params, g_s, g_t, tints=False)
    assert np.array_equal(gm, gm0) and np.array_equal(ge, ge0) and np.abs(gm0).max() > 0
    # ... and with it as well: the tint hook adds to its own words only
    gm1, ge1, _, _ = host_grad_tint(ht, scene, params, g_s, g_t)
    assert np.array_equal(gm1, gm0) and np.array_equal(ge1, ge0)


# -- the zero rule -----------------------------------------------------------------------------------------------------------
def test_a_zero_tint_channel_receives_and_adds_nothing(ht):
    scene = tint_scene("ggx")
    sd = scene.data()
    slots = host_tint_layout(ht, scene)
    params = T.render_params(scene)
    g_s, g_t = T.upstream(scene, "random")
    m = sd.tint_params["large-box.bsdf.specular_transmittance.value"][0]
    i_r, i_t = slots.index((m, 0)), slots.index((m, 1))
    sd.materials[m].c2[1] = 0.0
    sd.materials[m].c[2] = 0.0
    _, _, gx, _ = host_grad_tint(ht, scene, params, g_s, g_t)
    assert np.all(np.isfinite(gx)) and gx[i_t][1] == 0.0 and gx[i_r][2] == 0.0
    assert gx[i_t][0] != 0.0 and gx[i_r][0] != 0.0
    tt = np.zeros((len(slots), 3), np.float32)
    tt[i_t, 1] = 1.0
    tt[i_r, 2] = 1.0
    zm, ze = np.zeros((sd.n_materials, 3), np.float32), np.zeros((max(1, sd.n_emitters), 3), np.float32)
    d_s, d_t = host_fwd_tint(ht, scene, params, zm, ze, tt)
    assert np.all(d_s == 0.0) and np.all(d_t == 0.0)
    tt[i_t, 0] = 1.0
    d_s, d_t = host_fwd_tint(ht, scene, params, zm, ze, tt)
    assert np.all(np.isfinite(d_t)) and np.abs(d_t).max() > 0


# -- keys --------------------------------------------------------------------------------------------------------------------
def test_tint_keys_exist_exactly_where_the_dictionary_sets_the_property(ht):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    scene = tint_scene("pane")
    keys = scene.tint_keys()
    assert set(keys) == {"pane.bsdf.specular_reflectance.value", "pane.bsdf.specular_transmittance.value",
                         "large-box.bsdf.brdf_0.specular_reflectance.value"}
    params = mi.traverse(scene)
    assert set(keys) <= set(params) and list(params["pane.bsdf.specular_transmittance.value"]) == [np.float32(x) for x in (0.6, 0.8, 0.95)]
    # slots are mtr_scene_tint_layout's
    slots = host_tint_layout(ht, scene)
    sd = scene.data()
    assert {k: slots.index(sd.tint_params[k]) for k in keys} == keys
    # grad_keys() is what it is without tints: materials and emitters only
    assert {kind for kind, _ in scene.grad_keys().values()} == {"material", "emitter"}
    assert not set(keys) & set(scene.grad_keys())
    # an unset tint is no parameter; a top-level BSDF referenced by id has <id>.* keys; plastic tints have none
    d = mitr.cornell_box()
    d["sensor"]["film"].update(**SMALL)
    d["glass"] = dict(type="dielectric", int_ior=1.5, specular_transmittance=0.9)
    d["small-box"]["bsdf"] = dict(type="ref", id="glass")
    d["large-box"]["bsdf"] = dict(type="plastic", specular_reflectance=rgb(0.9, 0.8, 0.7), diffuse_reflectance=rgb(0.2, 0.3, 0.4))
    d["back"]["bsdf"] = dict(type="conductor", **COPPER)
    scene = T._mi().load_dict(d)
    assert set(scene.tint_keys()) == {"glass.specular_transmittance.value"}
    assert list(mi.traverse(scene)["glass.specular_transmittance.value"]) == [np.float32(0.9)] * 3


def test_shared_dictionaries_alias_until_a_tint_key_is_set():
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    d = mitr.cornell_box()
    d["sensor"]["film"].update(**SMALL)
    shared = dict(type="conductor", **COPPER, specular_reflectance=rgb(0.8, 0.9, 0.6))
    d["small-box"]["bsdf"] = shared
    d["large-box"]["bsdf"] = shared
    scene = T._mi().load_dict(d)
    sd = scene.data()
    a, b = "small-box.bsdf.specular_reflectance.value", "large-box.bsdf.specular_reflectance.value"
    assert sd.tint_params[a] == sd.tint_params[b]
    params = mi.traverse(scene)
    params[a] = [0.5, 0.4, 0.3]
    params.update()
    sd = scene.data()
    ma, mb = sd.tint_params[a][0], sd.tint_params[b][0]
    assert ma != mb
    assert [sd.materials[ma].c[k] for k in range(3)] == [np.float32(x) for x in (0.5, 0.4, 0.3)]
    assert [sd.materials[mb].c[k] for k in range(3)] == [np.float32(x) for x in (0.8, 0.9, 0.6)]


def test_updating_a_tint_gives_the_scene_a_fresh_load_gives(host_harness):
    import mitransient_amd.mi as mi
    from conftest import hh_render
    scene = tint_scene("ggx")
    params = mi.traverse(scene)
    params["large-box.bsdf.specular_transmittance.value"] = [0.3, 0.5, 0.7]
    params["small-box.bsdf.specular_reflectance.value"] = 0.4
    params.update()
    fresh = tint_scene("ggx")
    fsd = fresh.data()
    m = fsd.tint_params["large-box.bsdf.specular_transmittance.value"][0]
    for k, x in enumerate((0.3, 0.5, 0.7)):
        fsd.materials[m].c2[k] = x
    m = fsd.tint_params["small-box.bsdf.specular_reflectance.value"][0]
    for k in range(3):
        fsd.materials[m].c[k] = 0.4
    rp = T.render_params(scene)
    t_a, s_a, _ = hh_render(host_harness, scene.data(), rp)
    t_b, s_b, _ = hh_render(host_harness, fsd, rp)
    untouched = hh_render(host_harness, tint_scene("ggx").data(), rp)[0]
    assert np.array_equal(t_a, t_b) and np.array_equal(s_a, s_b) and not np.array_equal(t_a, untouched)


# -- refusals: all before any GPU work ---------------------------------------------------------------------------------------
def test_refusals():
    import torch
    import mitransient_amd as mitr
    from conftest import make_nlos
    scene = tint_scene("smooth")
    integ = scene.integrator()
    key = "small-box.bsdf.specular_reflectance.value"
    assert integ.check_grad_(scene, 0, {key: torch.ones(3, requires_grad=True)})[key][0] == "tint"
    assert integ.check_grad_(scene, 0, {key: torch.ones(1, requires_grad=True)})[key][0] == "tint"
    with pytest.raises(ValueError, match="1 or 3 elements"):
        integ.check_grad_(scene, 0, {key: torch.ones(2, requires_grad=True)})
    with pytest.raises(NotImplementedError, match="1 or 3 elements"):
        integ.render_forward(scene, {}, tangents={key: torch.ones(2)})
    # plastic / roughplastic: the tint enters lobe sampling
    d = mitr.cornell_box()
    d["sensor"]["film"].update(**SMALL)
    d["small-box"]["bsdf"] = dict(type="plastic", specular_reflectance=rgb(0.9, 0.8, 0.7))
    d["large-box"]["bsdf"] = dict(type="roughplastic", alpha=0.2, specular_reflectance=rgb(0.9, 0.8, 0.7))
    plastic = T._mi().load_dict(d)
    for k in ("small-box.bsdf.specular_reflectance.value", "large-box.bsdf.specular_reflectance.value"):
        with pytest.raises(ValueError, match="not a differentiable parameter"):
            plastic.integrator().check_grad_(plastic, 0, {k: torch.ones(3, requires_grad=True)})
        with pytest.raises(NotImplementedError, match="not a differentiable parameter"):
            plastic.integrator().render_forward(plastic, {}, tangents={k: torch.ones(3)})
    # a tint key on a NLOS scene
    nlos = make_nlos(hidden_bsdf=dict(type="conductor", **COPPER, specular_reflectance=rgb(0.8, 0.9, 0.6)))
    assert nlos.tint_keys() == {}
    with pytest.raises(ValueError, match="not a differentiable parameter"):
        nlos.integrator().check_grad_(nlos, 0, {"hidden.bsdf.specular_reflectance.value": torch.ones(3, requires_grad=True)})


# -- the Adam fit of tests/tint_gpu_cases.py, rehearsed on the CPU ------------------------------------------------------------
ADAM_BAND = 0.015    # |final - true| per channel; set from the rehearsal below (oracle primal + host-build gradients: worst 0.0073), not from a GPU run


def adam_rehearsal(ht):
    """tint_gpu_cases.adam() with the oracle as the primal and the host build as render_backward, at the same seeds (primal 100, gradient it + 1)"""
    import torch
    from oracle import oracle
    import tint_gpu_cases as G
    scene = G.adam_scene()
    sd = scene.data()
    f = sd.film
    m, which = sd.tint_params[G.ADAM_KEY]
    slot = host_tint_layout(ht, scene).index((m, which))

    def set_tint(v):
        for k in range(3):
            sd.materials[m].c[k] = float(v[k])

    def primal(seed, spp):
        t4, s4, _ = oracle.render(sd, T.render_params(scene, seed=seed, spp=spp), use_bvh=True)
        return oracle.develop(f, t4, s4)[0]

    set_tint(G.ADAM_TRUE)
    target = primal(100, G.ADAM_SPP)
    x = torch.tensor(G.ADAM_START, requires_grad=True)
    opt = torch.optim.Adam([x], lr=G.ADAM_LR)
    hist, losses = [], []
    for it in range(G.ADAM_STEPS):
        opt.zero_grad()
        set_tint(x.detach().numpy())
        t = primal(100, G.ADAM_SPP)
        losses.append(float(np.sum((t.astype(np.float64) - target) ** 2)))
        g_t = (2.0 * (t - target)).astype(np.float32)
        g_s = np.zeros((f.height, f.width, 3), np.float32)
        gx = host_grad_tint(ht, scene, T.render_params(scene, seed=it + 1, spp=G.ADAM_SPP), g_s, g_t)[2]
        x.grad = torch.from_numpy(gx[slot].astype(np.float32))
        opt.step()
        with torch.no_grad():
            x.clamp_(0.01, 1.0)
        hist.append([float(v) for v in x.detach()])
    return hist, losses


def test_adam_rehearsal_on_the_cpu(ht, oracle):
    import tint_gpu_cases as G
    hist, losses = adam_rehearsal(ht)
    thirds = [float(np.mean(losses[i:i + 20])) for i in (0, 20, 40)]
    err = np.abs(np.array(hist[-1]) - G.ADAM_TRUE)
    print(f"\n[tint] adam rehearsal: final {hist[-1]}, error {err}, mean loss per 20 steps {thirds}")
    assert thirds[0] > thirds[1] > thirds[2]                # the loss decreases
    assert np.all(err <= ADAM_BAND / 2), (hist[-1], err)    # the band leaves the CPU run a factor of two
