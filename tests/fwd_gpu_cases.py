"""One GPU step of tests/test_gpu_fwd.py, run in a child process of its own (the test gives each step a time limit):
``python tests/fwd_gpu_cases.py <case>`` prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import test_grad as T  # noqa: E402
import test_fwd as F  # noqa: E402
import grad_gpu_cases as GC  # noqa: E402

MTR_ERR_UNSUPPORTED = -5


def refilm(scene, width=12, height=10, bins=32, **film):
    """the scene loaded again with a film of `width` x `height` pixels and `bins` time bins"""
    import mitransient_amd.mi as mi
    d = scene.dict_
    d["sensor"]["film"].update(width=width, height=height, temporal_bins=bins, **film)
    return mi.load_dict(d)


def gpu_fwd(scene, tan, seed=3, spp=8, p0=0, p1=None, s0=0, s1=None, prefill=0.0, check=True):
    """mtr_render_fwd itself: (status, steady (H, W, 3), transient (H, W, T, 3)) as f32 arrays, the outputs pre-filled"""
    import torch
    from mitransient_amd.runtime import get_context
    sd = scene.data()
    f = sd.film
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    tm = torch.zeros((max(1, sd.n_materials), 3), device="cuda")
    tm[:sd.n_materials] = torch.from_numpy(tan.mats).cuda()
    te = torch.zeros((max(1, sd.n_emitters), 3), device="cuda")
    te[:sd.n_emitters] = torch.from_numpy(tan.ems).cuda()
    tx = tan.flat_texels()
    d_tx = torch.from_numpy(tx).cuda() if tx is not None else None
    steady = torch.full((f.height, f.width, 3), prefill, device="cuda")
    transient = torch.full((f.height, f.width, f.temporal_bins, 3), prefill, device="cuda")
    prm = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp, s0, s1, p0, p1)
    rc = ctx.lib.mtr_render_fwd(h, C.byref(prm), C.c_void_p(tm.data_ptr()), C.c_void_p(te.data_ptr()),
                                C.c_void_p(d_tx.data_ptr()) if d_tx is not None else None,
                                C.c_void_p(steady.data_ptr()), C.c_void_p(transient.data_ptr()))
    torch.cuda.synchronize()
    if check:
        ctx.check(rc, "mtr_render_fwd")
    return rc, steady.cpu().numpy(), transient.cpu().numpy()


def tier(scene, spp=8):
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    prm = scene.integrator().render_params(scene.sensors()[0].film(), 3, spp)
    t = C.c_uint32(0)
    ctx.check(ctx.lib.mtr_render_fwd_tier(h, C.byref(prm), C.byref(t)), "mtr_render_fwd_tier")
    return {1: "rows", 2: "global"}[int(t.value)]


def host(scene, tan, seed=3, spp=8, p0=0, p1=None, threads=1):
    """the host build over the same lanes: (steady (H, W, 3) with the crop window at the top-left corner, transient), f64"""
    from concurrent.futures import ThreadPoolExecutor
    hf = C.CDLL(F.build_host_fwd())
    f = scene.data().film
    integ, film = scene.integrator(), scene.sensors()[0].film()
    p1 = f.crop_width * f.crop_height if p1 is None else p1
    edges = np.linspace(p0, p1, threads + 1).astype(int)

    def part(i):
        s, t = F.host_fwd(hf, scene, integ.render_params(film, seed, spp, 0, None, int(edges[i]), int(edges[i + 1])), tan)
        full = np.zeros((f.height, f.width, 3))
        full[:s.shape[0], :s.shape[1]] = s
        return np.concatenate([full.ravel(), t.ravel()])

    if threads == 1:
        flat = part(0)
    else:
        with ThreadPoolExecutor(threads) as pool:
            flat = sum(pool.map(part, range(threads)))
    n_s = f.height * f.width * 3
    return flat[:n_s].reshape(f.height, f.width, 3), flat[n_s:].reshape(f.height, f.width, f.temporal_bins, 3)


def against_host(scene, tan, spp=8, threads=1, **kw):
    _, s, t = gpu_fwd(scene, tan, spp=spp, **kw)
    hs, ht = host(scene, tan, spp=spp, threads=threads, **{k: v for k, v in kw.items() if k in ("p0", "p1", "seed")})
    return {"rel_s": F.rel_l2(s, hs), "rel_t": F.rel_l2(t, ht), "scale": float(np.abs(ht).max()),
            "finite": bool(np.all(np.isfinite(s)) and np.all(np.isfinite(t))),
            "instantiation": GC.instantiation(scene), "tier": tier(scene, spp)}


def textured():
    import test_grad_general as G
    import test_grad_texture as X
    scene = refilm(G.textured(GC._tmp()))
    scene.integrator().max_depth, scene.integrator().rr_depth = 4, 5
    X.set_texels(scene, 0)
    return scene


# the four <SCENE_LDS, EXT> forms: (scene, texel tangents?)
FORMS = {
    "lds,plain": (lambda: refilm(T.cornell(angular=True)), False), "lds,ext": (textured, True),
    "hbm,plain": (lambda: refilm(GC.staircase()), False), "hbm,ext": (lambda: refilm(GC.rough_staircase()), False),
}


def form(name):
    make, tex = FORMS[name]
    scene = make()
    out = against_host(scene, F.random_tangents(scene, texels=tex), threads=4)
    out["expected"] = name
    return out


def rows(spp):
    """the row scheme at spp 16 (16 pixels per run; 120 pixels are no multiple of it), 24 (10 pixels per run: 256 is no multiple of
    24) and 300 (one pixel per run, two trips)"""
    scene = refilm(T.cornell())
    return against_host(scene, F.random_tangents(scene), spp=spp, threads=8)


def many_runs():
    """more runs than the grid has workgroups: 64 x 40 pixels at 256 spp are 2560 one-pixel runs, the grid at most
    kFwdPerCu = 3 workgroups per compute unit"""
    import torch
    scene = refilm(T.cornell(max_depth=3), 64, 40, 32)
    out = against_host(scene, F.random_tangents(scene), spp=256, threads=16)
    out.update(n_runs=64 * 40, grid_cap=3 * torch.cuda.get_device_properties(0).multi_processor_count)
    return out


def ranges():
    """two pixel ranges whose boundary (pixel 37) splits a 16-pixel run compose to the full render bit for bit — at 16 spp a
    pixel's lanes are a quarter of ONE wave whichever slot the pixel takes, so its LDS adds keep their order — and leave the
    pixels outside them at the sentinel"""
    scene = refilm(T.cornell())
    tan = F.random_tangents(scene)
    _, fs, ft = gpu_fwd(scene, tan, spp=16)
    sentinel = -7.0
    _, as_, at = gpu_fwd(scene, tan, spp=16, p0=0, p1=37, prefill=sentinel)
    _, bs, bt = gpu_fwd(scene, tan, spp=16, p0=37, p1=120, prefill=sentinel)
    a_in = np.zeros(120, bool)
    a_in[:37] = True
    flat = lambda x: x.reshape(120, -1)      # noqa: E731
    return {"composed_equal": bool(np.array_equal(flat(as_)[a_in], flat(fs)[a_in]) and np.array_equal(flat(at)[a_in], flat(ft)[a_in]) and
                                   np.array_equal(flat(bs)[~a_in], flat(fs)[~a_in]) and np.array_equal(flat(bt)[~a_in], flat(ft)[~a_in])),
            "untouched": bool(np.all(flat(as_)[~a_in] == sentinel) and np.all(flat(at)[~a_in] == sentinel) and
                              np.all(flat(bs)[a_in] == sentinel) and np.all(flat(bt)[a_in] == sentinel)),
            "nonzero": bool(np.abs(ft).max() > 0), "no_sentinel_in_full": bool(not np.any(ft == sentinel))}


def global_tier():
    """a 4 x 4 film with 16384 bins: the 192 KB row cannot fit LDS"""
    scene = refilm(T.cornell(), 4, 4, 16384, start_opl=3.0, bin_width_opl=0.0005)
    out = against_host(scene, F.random_tangents(scene), spp=64, threads=4, prefill=5.0)
    out["small_film_tier"] = tier(refilm(T.cornell()))
    return out


def duality():
    """mtr_render_fwd against mtr_render_grad_tex on the device: sum g . (J v) = sum (J^T g) . v"""
    import torch
    scene = textured()
    # the texels go through the parameter store, so that render_backward's params.update() uploads the texels both passes see
    p = GC.all_params(scene)
    key = sorted(scene.texture_keys())[0]
    p[key] = torch.tensor(scene.data().textures[0].copy(), dtype=torch.float32, requires_grad=True)
    p.update()
    sd = scene.data()
    f = sd.film
    tan = F.random_tangents(scene, texels=True, lo=-0.2)
    g_s, g_t = T.upstream(scene, "random")
    g_s, g_t = g_s + 1.0, g_t + 1.0
    _, s, t = gpu_fwd(scene, tan)
    prod = np.concatenate([(g_s.astype(np.float64) * s[:f.crop_height, :f.crop_width]).ravel(), (g_t.astype(np.float64) * t).ravel()])
    g = scene.integrator().render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=3, spp=8)
    keys = scene.grad_keys()
    rhs = float(np.sum(g[key].double().cpu().numpy() * tan.texels[0]))
    for k, (kind, i) in keys.items():
        rhs += float(np.sum(g[k].double().cpu().numpy() * (tan.mats if kind == "material" else tan.ems)[i]))
    lhs, mag = float(prod.sum()), float(np.abs(prod).sum())
    return {"err": abs(lhs - rhs) / mag, "share": abs(lhs) / mag, "control": abs(lhs * (1 + 2e-4) - rhs) / mag,
            "instantiation": GC.instantiation(scene)}


def oracle_linear():
    """dL = L: the kernel's tangent film is the oracle's primal film (no mtr_fwd.h on the checking side)"""
    import test_grad_general as G
    scene = refilm(G.rough_scene("ggx", max_depth=6, rr_depth=2, angular=True))
    _, s, t = gpu_fwd(scene, F.Tangents(scene, ems=F.radiances(scene)))
    s3, t3 = F.oracle_film(scene, T.render_params(scene))
    return {"rel_s": F.rel_l2(s, s3), "rel_t": F.rel_l2(t, t3), "scale": float(np.abs(t3).max()), "instantiation": GC.instantiation(scene)}


def oracle_degree():
    """da = a: the kernel's tangent film is sum_c N(c) c of the oracle's splat log, roulette active"""
    import test_grad_general as G
    scene = refilm(G.degree_scene(12, 64), 12, 10, 64)
    _, s, t = gpu_fwd(scene, F.Tangents(scene, mats=F.albedos(scene)))
    params = T.render_params(scene)
    r_s, r_t, (d0, d1, n) = F.degree_film(scene, params)
    w_s, w_t, _ = F.degree_film(scene, params, offset=1)
    return {"rel_s": F.rel_l2(s, r_s), "rel_t": F.rel_l2(t, r_t), "control": F.rel_l2(t, w_t), "depths": [d0, d1], "n_terms": n,
            "instantiation": GC.instantiation(scene)}


def forward_ad():
    """mi.render inside forward_ad.dual_level(): the outputs' tangents are render_forward at seed_grad / spp_grad; a 1-element
    reflectance stands for three equal channels"""
    import torch
    import torch.autograd.forward_ad as fwAD
    import mitransient_amd.mi as mi
    scene = refilm(T.cornell())
    red, light = "red.reflectance.value", "light.emitter.radiance.value"
    x, dx = torch.tensor([0.5, 0.2, 0.1]), torch.tensor([0.3, -0.1, 0.05])
    y, dy = torch.tensor([10.0, 8.0, 6.0]), torch.tensor([1.0, 0.0, -2.0])
    p = mi.traverse(scene)
    with fwAD.dual_level():
        p[red], p[light] = fwAD.make_dual(x, dx), fwAD.make_dual(y, dy)
        p.update()
        steady, transient = mi.render(scene, p, spp=8, seed=11, seed_grad=77, spp_grad=16)
        ts, tt = fwAD.unpack_dual(steady.torch()).tangent, fwAD.unpack_dual(transient.torch()).tangent
        has = ts is not None and tt is not None
        ts, tt = ts.double().cpu().numpy(), tt.double().cpu().numpy()
        auto_s, auto_t = scene.integrator().render_forward(scene, p, seed=77, spp=16)        # tangents=None: the dual values
        auto = max(F.rel_l2(np.array(auto_s), ts), F.rel_l2(np.array(auto_t), tt))
    integ = scene.integrator()
    rs, rt = integ.render_forward(scene, p, seed=77, spp=16, tangents={red: dx, light: dy})
    other = integ.render_forward(scene, p, seed=78, spp=16, tangents={red: dx, light: dy})[1]
    out = {"has_tangents": bool(has), "rel_s": F.rel_l2(ts, np.array(rs, np.float64)), "rel_t": F.rel_l2(tt, np.array(rt, np.float64)),
           "auto": auto, "seed_seen": F.rel_l2(np.array(other), np.array(rt, np.float64)) > 1e-3, "shape_s": list(ts.shape), "shape_t": list(tt.shape)}
    q = mi.traverse(scene)
    q[red] = torch.tensor([0.4])
    q.update()
    one = integ.render_forward(scene, q, seed=77, spp=16, tangents={red: torch.tensor([0.25])})[1]
    q[red] = torch.tensor([0.4, 0.4, 0.4])
    q.update()
    three = integ.render_forward(scene, q, seed=77, spp=16, tangents={red: torch.tensor([0.25, 0.25, 0.25])})[1]
    out.update(scalar=F.rel_l2(np.array(one), np.array(three, np.float64)), scalar_scale=float(np.abs(np.array(three)).max()))
    return out


def texel_keys():
    """render_forward with tangents on the `.data` keys of TWO bitmaps of different sizes (and a constant key) against
    mtr_render_fwd handed the same texels in the layout of mtr_scene_texture_layout: the Python layer's offsets.  `control`: the
    same comparison with the second bitmap's tangent left out"""
    import torch
    import mitransient_amd.mi as mi
    import test_grad_texture as X
    tmp = GC._tmp()
    X.write_png(tmp / "a.png", 4, 3, seed=1)
    X.write_png(tmp / "b.png", 3, 2, seed=2)

    def edit(d):
        d["back"]["bsdf"] = {"type": "diffuse", "reflectance": X.bitmap(tmp / "a.png")}
        d["floor"]["bsdf"] = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": X.bitmap(tmp / "b.png")}}
    scene = refilm(X.box_scene(tmp, edit))
    keys = scene.texture_keys()
    assert sorted(keys.values()) == [0, 1] and len(scene.data().textures) == 2
    shapes = [tuple(t.shape) for t in scene.data().textures]
    assert shapes[0] != shapes[1]
    rng = np.random.default_rng(5)
    by_tex = [rng.uniform(-0.2, 1.0, sh).astype(np.float32) for sh in shapes]
    red = "red.reflectance.value"
    d_red = np.array([0.3, -0.01, 0.02], np.float32)
    tangents = {k: torch.from_numpy(by_tex[i]) for k, i in keys.items()}
    tangents[red] = torch.from_numpy(d_red)
    p = mi.traverse(scene)
    rs, rt = scene.integrator().render_forward(scene, p, seed=3, spp=8, tangents=tangents)
    tan = F.Tangents(scene, texels=by_tex)
    tan.mats[scene.grad_keys()[red][1]] = d_red
    _, s, t = gpu_fwd(scene, tan)
    without = F.Tangents(scene, texels=[by_tex[0], np.zeros_like(by_tex[1])])
    without.mats[:] = tan.mats
    _, _, t0 = gpu_fwd(scene, without)
    return {"rel_s": F.rel_l2(np.array(rs), s.astype(np.float64)), "rel_t": F.rel_l2(np.array(rt), t.astype(np.float64)),
            "control": F.rel_l2(np.array(rt), t0.astype(np.float64)), "scale": float(np.abs(t).max()),
            "instantiation": GC.instantiation(scene)}


def crop():
    """a 7 x 5 crop window at (3, 2) of the 12 x 10 film: the row store's film addressing against the host build's, the pixels
    outside the window left at the sentinel, and render_forward's (crop_h, crop_w, 3) steady tensor"""
    import mitransient_amd.mi as mi
    scene = refilm(T.cornell(), crop_width=7, crop_height=5, crop_offset_x=3, crop_offset_y=2)
    f = scene.data().film
    assert (f.crop_width, f.crop_height, f.width, f.height) == (7, 5, 12, 10)
    tan = F.random_tangents(scene)
    out = against_host(scene, tan, spp=16, threads=4)
    _, s, t = gpu_fwd(scene, tan, spp=16, prefill=-7.0)
    inside = np.zeros((10, 12), bool)
    inside[:5, :7] = True                                   # (the crop window sits at the top-left corner of the tensors)
    out["outside_untouched"] = bool(np.all(s[~inside] == -7.0) and np.all(t[~inside] == -7.0) and not np.any(t[inside] == -7.0))
    keys = scene.grad_keys()
    tangents = {k: (tan.mats if kind == "material" else tan.ems)[i] for k, (kind, i) in keys.items()}
    rs, rt = scene.integrator().render_forward(scene, mi.traverse(scene), seed=3, spp=16, tangents=tangents)
    out.update(shape_s=list(np.array(rs).shape), py_s=F.rel_l2(np.array(rs), s[:5, :7].astype(np.float64)),
               py_t=F.rel_l2(np.array(rt)[inside], t[inside].astype(np.float64)))
    return out


def sub_range():
    """a sample sub-range is MTR_ERR_UNSUPPORTED and the outputs stay as they were"""
    scene = refilm(T.cornell())
    rc, s, t = gpu_fwd(scene, F.random_tangents(scene), spp=8, s0=0, s1=4, prefill=9.0, check=False)
    return {"status": int(rc), "untouched": bool(np.all(s == 9.0) and np.all(t == 9.0))}


if __name__ == "__main__":
    case = sys.argv[1]
    import torch
    torch.cuda.set_device(0)
    if case in FORMS:
        out = form(case)
    elif case.startswith("rows_"):
        out = rows(int(case[5:]))
    else:
        out = {"many_runs": many_runs, "ranges": ranges, "global": global_tier, "duality": duality, "oracle_linear": oracle_linear,
               "oracle_degree": oracle_degree, "forward_ad": forward_ad, "sub_range": sub_range, "texel_keys": texel_keys,
               "crop": crop}[case]()
    print(json.dumps(out))
