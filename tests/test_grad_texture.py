"""Gradients of bitmap texels (mtr_render_grad_tex, the texel hook of mtr_grad.h): the host build tests/host_grad_tex.cpp against
the unchanged CPU oracle at the same seed, and the Python surface (``.reflectance.data`` keys, params.update(), refusals).

(FD)        With rr_depth > max_depth the seeded loss is a polynomial of degree < max_depth in every texel channel (the
            interpolated albedo is linear in its four taps): test_grad.fd_material(wide=True)'s quartic fit, applied to texels,
            is exact.  Bound: the project's 1e-4 of the texture's largest finite difference (test_grad.within).
(RR-const)  blue = 1 in every albedo AND every texel keeps rr_prob at 0.95 (test_grad_general.py).
(RR-degree) sum_texels t dloss/dt + sum_m a_m dloss/da_m = sum_c w_c c N(c): a(v) = sum_taps w_t t, so t dloss/dt summed over the
            taps of a vertex is a(v) dloss/da(v) — the textured vertices count like the constant ones.
Measured on the CPU (printed by the tests): worst FD error 1.9e-6 .. 4.2e-6 of the largest finite difference (the
oracle's own two-fit disagreement on the 8 x 4 case is 2.3e-6), the degree identity within 1.3e-6, a constant texture within 1.7e-8.
No GPU needed; tests/grad_tex_gpu_cases.py holds the kernel to the host build."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import test_grad as T
import test_grad_general as G
from test_grad import hg  # noqa: F401  (the host build of mtr_grad.h without the texel hook)
from conftest import hh_render

ROOT = T.ROOT


def build_host_grad_tex():
    """tests/host_grad_tex.cpp with the flags of test_grad.build_host_grad()"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_grad_tex.so")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "host_grad_tex.cpp"), os.path.join(csrc, "mtr_scene_host.cpp"), os.path.join(csrc, "mtr_bvh.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mtr_core.h", "mtr_grad.h", "mtr_scene_host.h", "mtr_bvh.h", "mtr_knobs.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-DMTR_EXPERIMENTS", "-o", tmp] + srcs, check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hgt():
    return C.CDLL(build_host_grad_tex())


def host_grad_tex(hgt, scene, params, g_s, g_t):
    """the host build's (grad_materials, grad_emitters, [one (H, W, 3) array per texture]), f64"""
    sd = scene.data()
    f = sd.film
    gs_full = np.zeros((f.height, f.width, 3), np.float32)
    gs_full[:g_s.shape[0], :g_s.shape[1]] = g_s
    gt = np.ascontiguousarray(g_t, dtype=np.float32)
    gm = np.zeros((max(1, sd.n_materials), 3))
    ge = np.zeros((max(1, sd.n_emitters), 3))
    n = sum(int(t.shape[0] * t.shape[1]) for t in sd.textures)
    gx = np.zeros((max(1, n), 3))
    n_out = C.c_uint64(0)
    d = sd.desc()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    rc = hgt.hg_render_grad_tex(C.byref(d), C.byref(params), gs_full.ctypes.data_as(fp), gt.ctypes.data_as(fp),
                                gm.ctypes.data_as(dp), ge.ctypes.data_as(dp), gx.ctypes.data_as(dp), C.byref(n_out))
    assert rc == 0 and int(n_out.value) == n
    per, at = [], 0
    for t in sd.textures:
        k = int(t.shape[0] * t.shape[1])
        per.append(gx[at:at + k].reshape(t.shape).copy())
        at += k
    return gm[:sd.n_materials], ge[:sd.n_emitters], per


def write_png(path, w, h, seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(40, 250, (h, w, 3), dtype=np.uint8)).save(path)


def bitmap(path):
    return {"type": "bitmap", "filename": str(path)}


def box_scene(tmp_path, edit, max_depth=4, rr_depth=5, blue=None, film=None):
    """test_grad.cornell()'s small Cornell box with its dictionary edited by ``edit(d)`` before it is loaded"""
    scene = T.cornell(max_depth=max_depth, rr_depth=rr_depth, blue=blue, **(film or {}))
    d = scene.dict_
    edit(d)
    return T._mi().load_dict(d)


def set_texels(scene, tex, values=None, seed=11, blue=None):
    """overwrite texture ``tex`` of the flattened scene in place: U(0.2, 0.9) — strictly positive — unless ``values`` are given"""
    t = scene.data().textures[tex]
    t[...] = np.random.default_rng(seed).uniform(0.2, 0.9, t.shape).astype(np.float32) if values is None else values
    if blue is not None:
        t[..., 2] = blue
    return t


def fd_texel(scene, params, g_s, g_t, tex, idx):
    """test_grad.fd_material(wide=True)'s scheme on one texel channel: the derivative at t of the quartic fitted by least squares
    to the oracle's loss at 16 abscissae from t / 8 to t + 1 / 4"""
    t = scene.data().textures[tex]
    a = float(t[idx])
    xs = np.linspace(a / 8, a + 0.25, 16).astype(np.float32).astype(np.float64)
    vals = []
    for x in xs:
        t[idx] = x
        vals.append(T.oracle_loss(scene, params, g_s, g_t)[0])
    t[idx] = a
    span = xs[-1] - xs[0]
    return float(np.polyder(np.poly1d(np.polyfit((xs - a) / span, vals, 4)))(0.0) / span)


def check_texels(hgt, scene, tex=0, chans=(0, 1, 2), kind="random", label=""):
    """every texel channel of texture ``tex`` within 1e-4 of the texture's largest finite difference, every gradient non-zero,
    and the control: the same gradients scaled by 1 + 2e-4 are rejected.  Returns the worst error."""
    t0 = time.time()
    g_s, g_t = T.upstream(scene, kind)
    params = T.render_params(scene)
    _, _, gx = host_grad_tex(hgt, scene, params, g_s, g_t)
    g = gx[tex][..., list(chans)]
    H, W = g.shape[:2]
    fd = np.array([[[fd_texel(scene, params, g_s, g_t, tex, (y, x, k)) for k in chans] for x in range(W)] for y in range(H)])
    worst = float(np.abs(g - fd).max() / np.abs(fd).max())
    print(f"\n[grad-tex] {label}: {g.size} texel channels, worst error {worst:.2e} of the largest finite difference "
          f"({time.time() - t0:.1f} s)")
    assert np.all(np.isfinite(g)) and np.all(g != 0.0) and np.all(fd != 0.0)
    assert T.within(g, fd, 1e-4), (g, fd)
    assert not T.within(g * (1 + 2e-4), fd, 1e-4)
    return worst


# -- (FD) --------------------------------------------------------------------------------------------------------------------
def test_texel_gradients_match_finite_differences(hgt, tmp_path):
    """test_grad_general.textured: one 8 x 4 bitmap on a two-sided panel (an `obj` with vt coordinates) and on a cube"""
    scene = G.textured(tmp_path)
    assert scene.integrator().rr_depth > scene.integrator().max_depth
    set_texels(scene, 0)
    assert scene.data().textures[0].shape == (4, 8, 3)
    check_texels(hgt, scene, label="textured (panel + crate)")


def panel_scene(tmp_path, vt, w=4, h=3):
    """a two-sided textured diffuse panel alone (an `obj` mesh, with or without vt coordinates) in the Cornell box"""
    mi = T._mi()
    write_png(tmp_path / "p.png", w, h)
    with open(tmp_path / "quad.obj", "w") as fh:
        fh.write("v -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\n")
        if vt:
            fh.write("vt 0.1 0.05\nvt 1.3 0\nvt 1.2 0.9\nvt 0 1\nf 1/1 2/2 3/3\nf 1/1 3/3 4/4\n")     # (beyond 1: the repeat wrap)
        else:
            fh.write("f 1 2 3\nf 1 3 4\n")

    def edit(d):
        del d["small-box"], d["large-box"]
        d["panel"] = {"type": "obj", "filename": str(tmp_path / "quad.obj"), "face_normals": True,
                      "to_world": mi.ScalarTransform4f().translate([0.0, -0.1, -0.5]).rotate([0, 1, 0], 20).scale([0.7, 0.6, 1.0]),
                      "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": bitmap(tmp_path / "p.png")}}}
    return box_scene(tmp_path, edit)


@pytest.mark.parametrize("vt", [True, False], ids=["twosided-mesh-with-vt", "mesh-without-texture-coordinates"])
def test_texel_gradients_on_meshes(hgt, tmp_path, vt):
    scene = panel_scene(tmp_path, vt)
    sd = scene.data()
    assert (sd.tri_uv is not None and np.abs(sd.tri_uv).max() > 0) == vt
    assert "panel.bsdf.brdf_0.reflectance.data" in scene.texture_keys()
    set_texels(scene, 0)
    check_texels(hgt, scene, label=f"panel vt={vt}")


def wall_scene(tmp_path, w, h, walls=("back",), **kw):
    """the Cornell box with a top-level textured `diffuse` BSDF ``pattern`` on ``walls`` (rectangles: uv = (prim_uv + 1) / 2)"""
    write_png(tmp_path / "wall.png", w, h)

    def edit(d):
        d["pattern"] = {"type": "diffuse", "reflectance": bitmap(tmp_path / "wall.png")}
        for name in walls:
            d[name]["bsdf"] = {"type": "ref", "id": "pattern"}
    return box_scene(tmp_path, edit, **kw)


@pytest.mark.parametrize("rr_depth", [1, 3])
def test_texel_gradients_with_roulette_at_a_constant_probability(hgt, oracle, tmp_path, rr_depth):
    scene = wall_scene(tmp_path, 3, 2, max_depth=5, rr_depth=rr_depth, blue=1.0)
    set_texels(scene, 0, blue=1.0)
    sd = scene.data()
    params = T.render_params(scene)
    assert params.rr_depth == rr_depth
    with_rr = oracle.render(sd, params, use_bvh=True)[2]
    params.rr_depth = 6
    without = oracle.render(sd, params, use_bvh=True)[2]
    assert with_rr["bounces"] < without["bounces"]                      # roulette did end paths
    check_texels(hgt, scene, chans=(0, 1), label=f"RR-const rr_depth {rr_depth}")


# -- (RR-degree) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "one_bin", "steady"])
def test_texel_gradients_have_the_degree_of_the_detached_estimator(hgt, tmp_path, kind):
    scene = wall_scene(tmp_path, 5, 3, walls=("back", "floor", "red-wall"), max_depth=12, rr_depth=2,
                       film=dict(bins=64, start_opl=0.0, bin_width=1.0))
    set_texels(scene, 0)
    sd = scene.data()
    assert all(sd.materials[m].type == 0 for m in range(sd.n_materials))
    assert any(sd.materials[m].albedo_texture for m in range(sd.n_materials)) and \
        not all(sd.materials[m].albedo_texture for m in range(sd.n_materials))
    params = T.render_params(scene)
    g_s, g_t = G.degree_upstream(scene, kind)
    gm, _, gx = host_grad_tex(hgt, scene, params, g_s, g_t)
    for m in range(sd.n_materials):
        if sd.materials[m].albedo_texture:
            assert np.all(gm[m] == 0.0)                                 # the textured material's own entry stays 0
    tex_part = (sd.textures[0].astype(np.float64) * gx[0]).sum(axis=(0, 1))
    mat_part, rhs, _, (d0, d1, n_terms) = G.degree_sides(scene, params, g_s, g_t, gm)
    lhs = tex_part + mat_part
    assert n_terms > 1000 and d0 == 0 and d1 >= 8
    assert np.all(np.abs(tex_part) > 0.05 * np.abs(rhs))                # the texels carry a real share of the identity
    print(f"\n[grad-tex] RR-degree {kind}: {float(np.max(np.abs(lhs - rhs) / np.abs(rhs))):.2e}")
    assert np.all(np.abs(lhs - rhs) <= 1e-5 * np.abs(rhs)), (lhs, rhs)
    _, rhs1, _, _ = G.degree_sides(scene, params, g_s, g_t, gm, offset=1)
    assert np.all(np.abs(lhs - rhs1) > 0.1 * np.abs(rhs1)), (lhs, rhs1)


# -- constant texture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(8, 4), (1, 1), (1, 5), (6, 1)])
def test_constant_texture_sums_to_the_constant_albedo_gradient(hg, hgt, tmp_path, w, h):
    c = np.array([0.625, 0.375, 0.25], np.float32)
    scene = wall_scene(tmp_path, w, h, walls=("back", "floor"))
    set_texels(scene, 0, values=c)
    g_s, g_t = T.upstream(scene, "random")
    _, _, gx = host_grad_tex(hgt, scene, T.render_params(scene), g_s, g_t)

    def edit(d):
        d["pattern"] = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [float(x) for x in c]}}
        for name in ("back", "floor"):
            d[name]["bsdf"] = {"type": "ref", "id": "pattern"}
    const = box_scene(tmp_path, edit)
    gm, _ = T.host_grad(hg, const, T.render_params(const), g_s, g_t)
    ref = gm[const.grad_keys()["pattern.reflectance.value"][1]]
    got = gx[0].sum(axis=(0, 1))
    print(f"\n[grad-tex] constant {w}x{h}: {float(np.max(np.abs(got - ref) / np.abs(ref))):.2e}")
    assert np.all(ref != 0) and np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref)), (got, ref)


# -- shared and excluded textures ---------------------------------------------------------------------------------------------
def test_two_materials_on_one_bitmap_sum_into_it(hgt, tmp_path):
    import shutil
    write_png(tmp_path / "a.png", 4, 3)
    shutil.copy(tmp_path / "a.png", tmp_path / "b.png")

    def two(file_b):
        def edit(d):
            d["back"]["bsdf"] = {"type": "diffuse", "reflectance": bitmap(tmp_path / "a.png")}
            d["floor"]["bsdf"] = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": bitmap(tmp_path / file_b)}}
        return box_scene(tmp_path, edit)
    shared, apart = two("a.png"), two("b.png")
    assert len(shared.data().textures) == 1 and len(apart.data().textures) == 2
    keys = shared.texture_keys()
    assert keys == {"back.bsdf.reflectance.data": 0, "floor.bsdf.brdf_0.reflectance.data": 0}
    assert sorted(apart.texture_keys().values()) == [0, 1]
    vals = np.random.default_rng(3).uniform(0.2, 0.9, (3, 4, 3)).astype(np.float32)
    set_texels(shared, 0, values=vals)
    set_texels(apart, 0, values=vals)
    set_texels(apart, 1, values=vals)
    g_s, g_t = T.upstream(shared, "random")
    _, _, one = host_grad_tex(hgt, shared, T.render_params(shared), g_s, g_t)
    _, _, two_ = host_grad_tex(hgt, apart, T.render_params(apart), g_s, g_t)
    assert np.abs(two_[0]).max() > 0 and np.abs(two_[1]).max() > 0
    assert np.abs(one[0] - (two_[0] + two_[1])).max() <= 1e-12 * np.abs(one[0]).max()
    # one tensor for two keys: differentiating both at once is refused
    import torch
    p = T._mi().traverse(shared)
    for k in keys:
        p[k] = torch.tensor(p[k], requires_grad=True)
    with pytest.raises(ValueError, match="one bitmap"):
        shared.integrator().check_grad_(shared, 0, p)


def test_a_bitmap_that_a_roughplastic_uses_is_no_parameter(tmp_path):
    import torch
    write_png(tmp_path / "a.png", 4, 3)

    def edit(d):
        d["back"]["bsdf"] = {"type": "diffuse", "reflectance": bitmap(tmp_path / "a.png")}
        d["small-box"]["bsdf"] = {"type": "roughplastic", "distribution": "ggx", "alpha": 0.2,
                                  "diffuse_reflectance": bitmap(tmp_path / "a.png")}
    scene = box_scene(tmp_path, edit)
    p = T._mi().traverse(scene)
    assert not [k for k in p if k.endswith(".data")] and scene.texture_keys() == {}
    assert len(scene.data().textures) == 1
    with pytest.raises(ValueError, match="not a differentiable parameter"):
        scene.integrator().check_grad_(scene, 0, {"back.bsdf.reflectance.data": torch.zeros((3, 4, 3), requires_grad=True)})
    # ... and a roughplastic alone (test_textures.textured_scene) has none either
    from test_textures import textured_scene
    assert textured_scene(tmp_path, "roughplastic").texture_keys() == {}


# -- keys and updates ---------------------------------------------------------------------------------------------------------
def test_data_keys_round_trip_and_update_is_a_fresh_load(host_harness, tmp_path):
    import torch
    from mitransient_amd.scene import decode_texture_u8
    from PIL import Image
    mi = T._mi()
    (tmp_path / "one").mkdir()
    (tmp_path / "two").mkdir()
    scene = G.textured(tmp_path / "one")
    before = dict(scene.grad_keys())
    p = mi.traverse(scene)
    panel, crate = "panel.bsdf.brdf_0.reflectance.data", "crate.bsdf.reflectance.data"
    assert panel in p and crate in p and scene.texture_keys() == {panel: 0, crate: 0}
    u8 = np.asarray(Image.open(tmp_path / "one" / "tex.png"))
    assert p[panel].shape == (4, 8, 3) and p[panel].dtype == np.float32
    assert np.array_equal(p[panel], decode_texture_u8(u8, False))            # linear RGB, after sRGB decoding
    assert scene.grad_keys() == before and all(kind in ("material", "emitter") for kind, _ in before.values())
    assert not [k for k in before if k.endswith(".data")]
    # a freshly loaded scene with another bitmap of the same size
    new_u8 = np.random.default_rng(5).integers(0, 256, (4, 8, 3), dtype=np.uint8)
    fresh = G.textured(tmp_path / "two")
    Image.fromarray(new_u8).save(tmp_path / "two" / "tex.png")
    fresh = mi.load_dict(fresh.dict_)
    new = decode_texture_u8(new_u8, False)
    assert np.array_equal(mi.traverse(fresh)[panel], new)
    for value in (new, torch.from_numpy(new.copy())):
        scene.data()                                                         # flattened before the update, as after a render
        p[panel] = value
        p.update()
        assert np.array_equal(mi.traverse(scene)[panel], new) and np.array_equal(mi.traverse(scene)[crate], new)
        sd, fd = scene.data(), fresh.data()
        assert np.array_equal(sd.textures[0], fd.textures[0])
        for m in range(sd.n_materials):
            assert list(sd.materials[m].a) == list(fd.materials[m].a)        # the mean-colour stand-in follows
        fresh.integrator().max_depth, fresh.integrator().rr_depth = 4, 5
        a = hh_render(host_harness, sd, T.render_params(scene))
        b = hh_render(host_harness, fd, T.render_params(fresh))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].max() > 0
        p[panel] = decode_texture_u8(u8, False)
        p.update()
        assert not np.array_equal(scene.data().textures[0], fd.textures[0])
    for bad in (np.zeros((8, 4, 3), np.float32), np.zeros((4, 8), np.float32), np.zeros(3, np.float32)):
        p[panel] = bad
        with pytest.raises(ValueError, match="shape"):
            p.update()
        p._dirty.clear()
    with pytest.raises(ValueError, match="shape"):
        scene.integrator().check_grad_(scene, 0, {panel: torch.zeros((8, 4, 3), requires_grad=True)})
    keys = scene.integrator().check_grad_(scene, 0, {panel: torch.zeros((4, 8, 3), requires_grad=True)})
    assert keys[panel] == ("texture", 0)
    assert scene.grad_keys() == before
