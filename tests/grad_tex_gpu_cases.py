"""One GPU step of tests/test_gpu_grad_texture.py, run in a child process of its own (the test gives each step a time limit):
``python tests/grad_tex_gpu_cases.py <case>`` prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import test_grad as T  # noqa: E402
import test_grad_texture as X  # noqa: E402
from grad_gpu_cases import _tmp, instantiation  # noqa: E402


def slab_lds():
    """test_grad_general.textured: the 8 x 4 bitmap, scene staged in LDS"""
    import test_grad_general as G
    scene = G.textured(_tmp())
    X.set_texels(scene, 0)
    return scene


def textured_staircase(size=(8, 4), tiles=6):
    """the textured staircase stand-in: staircase_like (tables beyond 64 KB: walked in HBM) with a bitmap on its `wall` BSDF"""
    import mitransient_amd.mi as mi
    from mitransient_amd.scenes import staircase_like
    mi.set_variant("llvm_ad_rgb")
    tmp = _tmp()
    X.write_png(tmp / "wall.png", *size)
    d = staircase_like(tiles=tiles, width=16, height=16, temporal_bins=32)
    d["integrator"].update(max_depth=4, rr_depth=5)
    name = [k for k, v in d.items() if isinstance(v, dict) and v.get("type") == "diffuse"][0]
    d[name] = {"type": "diffuse", "reflectance": X.bitmap(tmp / "wall.png")}
    scene = mi.load_dict(d)
    X.set_texels(scene, 0)
    return scene


def cornell_wall(size=(256, 256), **kw):
    """a bitmap on the Cornell box's back wall and floor"""
    scene = X.wall_scene(_tmp(), *size, walls=("back", "floor"), **kw)
    X.set_texels(scene, 0)
    return scene


SCENES = {
    "slab_lds": (slab_lds, "lds,ext", "slab"),
    "slab_hbm": (textured_staircase, "hbm,ext", "slab"),
    "global_wall": (cornell_wall, "lds,ext", "global"),
    "global_staircase": (lambda: textured_staircase((64, 64)), "hbm,ext", "global"),
}


def tex_params(scene, one_per_texture=True):
    """mi.traverse with every differentiable key grad-requiring (one `.data` key per texture)"""
    import torch
    import mitransient_amd.mi as mi
    p = mi.traverse(scene)
    seen = set()
    for k in scene.grad_keys():
        p[k] = torch.tensor(p[k], dtype=torch.float32, requires_grad=True)
    for k, i in scene.texture_keys().items():
        if i not in seen:
            seen.add(i)
            p[k] = torch.tensor(scene.data().textures[i], requires_grad=True)        # (the flattened texels: set in place by the case)
    return p


def upload(scene):
    """the texels the case wrote into the flattened tables go to the device through params.update()"""
    import mitransient_amd.mi as mi
    p = mi.traverse(scene)
    for k, i in scene.texture_keys().items():
        p[k] = scene.data().textures[i].copy()
    p.update()


def rel_errors(got, ref):
    """|got - ref| relative to the largest element of ref (test_gpu_grad.py's bound is 1e-5 of it), at worst"""
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def gpu_vs_host(scene, seed=3, spp=8):
    import torch
    hgt = C.CDLL(X.build_host_grad_tex())
    g_s, g_t = T.upstream(scene, "random")
    upload(scene)
    p = tex_params(scene)
    integ = scene.integrator()
    g = integ.render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=seed, spp=spp)
    torch.cuda.synchronize()
    params = integ.render_params(scene.sensors()[0].film(), seed, spp)
    gm, ge, gx = X.host_grad_tex(hgt, scene, params, g_s, g_t)
    out = {"tier": scene.grad_tex_tier(), "instantiation": instantiation(scene), "finite": True}
    rel_tex = 0.0
    for k, i in scene.texture_keys().items():
        if k in g:
            got = g[k].double().cpu().numpy()
            out["finite"] = out["finite"] and bool(np.all(np.isfinite(got)))
            rel_tex = max(rel_tex, rel_errors(got, gx[i]))
            out["texel_scale"] = float(np.abs(gx[i]).max())
            out["texels_nonzero"] = float(np.mean(gx[i] != 0.0))
            out["same_support"] = bool(np.array_equal(got != 0.0, gx[i] != 0.0))
            out["device_ok"] = g[k].is_cuda and tuple(g[k].shape) == tuple(scene.data().textures[i].shape)
    keys = scene.grad_keys()
    ref = {k: (gm if kind == "material" else ge)[i] for k, (kind, i) in keys.items()}
    scale = max(float(np.abs(v).max()) for v in ref.values())
    out["rel_other"] = max(float(np.max(np.abs(g[k].cpu().numpy() - ref[k]) / np.maximum(np.abs(ref[k]), 1e-9 * scale))) for k in keys)
    out["rel_texels"] = rel_tex
    return out


def grid_stride():
    """k_grad_paths' grid-stride loop over more than two trips with texels on, ragged at both ends (grad_gpu_cases.grid_stride's
    ranges) through mtr_render_grad_tex directly, both tiers, against the host build summed over 16 pixel ranges"""
    from concurrent.futures import ThreadPoolExecutor
    import torch
    import mitransient_amd.mi as mi
    from mitransient_amd.runtime import get_context
    out = {}
    for tier, size in (("slab", (8, 4)), ("global", (32, 32))):
        scene = cornell_wall(size)
        d = scene.dict_
        d["sensor"]["film"].update(width=101, height=97)
        scene = mi.load_dict(d)
        X.set_texels(scene, 0)
        upload(scene)
        integ = scene.integrator()
        film = scene.sensors()[0].film()
        sd = scene.data()
        g_s, g_t = T.upstream(scene, "random")
        p0, p1, s0, s1, spp = 100, 101 * 97, 3, 112, 113
        ctx = get_context()
        h = scene.gpu_handle(ctx, 0)
        gs_dev, gt_dev = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()
        gm = torch.zeros((sd.n_materials, 3), device="cuda")
        ge = torch.zeros((sd.n_emitters, 3), device="cuda")
        gx = torch.full((size[0] * size[1], 3), 7.0, device="cuda")                 # (stored, not added to)
        prm = integ.render_params(film, 3, spp, s0, s1, p0, p1)
        ctx.check(ctx.lib.mtr_render_grad_tex(h, C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()),
                                              C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr()), C.c_void_p(gx.data_ptr())),
                  "mtr_render_grad_tex")
        torch.cuda.synchronize()
        hgt = C.CDLL(X.build_host_grad_tex())
        edges = np.linspace(p0, p1, 17).astype(int)

        def part(i):
            a, b, c = X.host_grad_tex(hgt, scene, integ.render_params(film, 3, spp, s0, s1, int(edges[i]), int(edges[i + 1])), g_s, g_t)
            return np.concatenate([a, b, c[0].reshape(-1, 3)])

        with ThreadPoolExecutor(16) as pool:
            ref = sum(pool.map(part, range(16)))
        got = torch.cat([gm, ge, gx]).double().cpu().numpy()
        n_me = sd.n_materials + sd.n_emitters
        out[tier] = {"tier": scene.grad_tex_tier(), "rel_texels": rel_errors(got[n_me:], ref[n_me:]),
                     "rel_other": rel_errors(got[:n_me], ref[:n_me]), "n_lanes": (p1 - p0) * (s1 - s0),
                     "grid_cap_lanes": torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256}
    return out


def unchanged_entry_point():
    """mtr_render_grad on a textured scene: what mtr_render_grad_tex gives for materials and emitters bit for bit, textured
    materials 0, equal to the host build of the parent's arithmetic (tests/host_grad.cpp, which has no texel hook)"""
    import torch
    from mitransient_amd.runtime import get_context
    scene = slab_lds()
    upload(scene)
    sd = scene.data()
    integ = scene.integrator()
    g_s, g_t = T.upstream(scene, "random")
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    gs_dev, gt_dev = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()
    prm = integ.render_params(scene.sensors()[0].film(), 3, 8)
    res = []
    for with_tex in (False, True, None):
        gm = torch.zeros((sd.n_materials, 3), device="cuda")
        ge = torch.zeros((sd.n_emitters, 3), device="cuda")
        gx = torch.zeros((32, 3), device="cuda")
        args = [h, C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()), C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr())]
        if with_tex is False:
            ctx.check(ctx.lib.mtr_render_grad(*args), "mtr_render_grad")
        else:
            ctx.check(ctx.lib.mtr_render_grad_tex(*args, C.c_void_p(gx.data_ptr()) if with_tex else None), "mtr_render_grad_tex")
        torch.cuda.synchronize()
        res.append((gm.cpu(), ge.cpu(), gx.cpu()))
    tex = [m for m in range(sd.n_materials) if sd.materials[m].albedo_texture]
    hm, he = T.host_grad(C.CDLL(T.build_host_grad()), scene, prm, g_s, g_t)
    ref = np.concatenate([hm, he])
    got = torch.cat(res[0][:2]).double().numpy()
    return {"same_as_tex": bool(torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])),
            "null_is_plain": bool(torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[2][1]) and float(res[2][2].abs().max()) == 0.0),
            "textured_zero": bool(all(float(res[0][0][m].abs().max()) == 0.0 for m in tex)), "n_textured": len(tex),
            "texels_written": float(res[1][2].abs().max()) > 0,
            "rel_host": float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * np.abs(ref).max())))}


def autograd(which):
    """loss.backward() on a `.data` tensor against render_backward at seed_grad / spp_grad: bit for bit on the slab tier, within
    1e-6 of the largest element on the global tier (arrival order of the f64 atomics: the f32 output can round either way)"""
    import torch
    import mitransient_amd.mi as mi
    scene = cornell_wall((8, 4) if which == "slab" else (64, 64))
    f = scene.data().film
    rng = np.random.default_rng(7)
    w_s = torch.from_numpy(rng.standard_normal((f.height, f.width, 3)).astype(np.float32)).cuda()
    w_t = torch.from_numpy(rng.standard_normal((f.temporal_bins,)).astype(np.float32)).cuda()
    key, red = "pattern.reflectance.data", "red.reflectance.value"
    p = mi.traverse(scene)
    x = torch.tensor(scene.data().textures[0], requires_grad=True)                     # a CPU tensor: its gradient arrives on the CPU
    y = torch.tensor([0.5, 0.2, 0.1], requires_grad=True)
    p[key], p[red] = x, y
    p.update()
    steady, transient = mi.render(scene, p, spp=8, seed=11, seed_grad=77, spp_grad=4)
    loss = (steady.torch() * w_s).sum() + (transient.torch() * w_t[None, None, :, None]).sum()
    loss.backward()
    g_t = w_t[None, None, :, None].expand(f.height, f.width, f.temporal_bins, 3)
    ref = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=77, spp=4)
    other = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=78, spp=4)
    a, b = x.grad.double(), ref[key].cpu().double()
    return {"tier": scene.grad_tex_tier(), "equal": bool(torch.equal(x.grad, ref[key].cpu())), "rel": float((a - b).abs().max() / b.abs().max()),
            "shape_ok": tuple(x.grad.shape) == tuple(x.shape) and not x.grad.is_cuda and ref[key].is_cuda,
            "constant_equal": bool(torch.equal(y.grad, ref[red].cpu())), "nonzero": float((x.grad != 0).float().mean()),
            "seed_seen": not torch.equal(ref[key], other[key])}


ADAM = dict(size=(8, 8), res=48, bins=48, spp=16, iters=60, lr=0.05)


def adam():
    """mi.render + torch autograd + Adam on a `.data` tensor: a two-colour checker pattern on the back wall recovered from a
    transient target, starting from uniform grey; the loss (mean squared error over the transient tensor, evaluated before and
    after at the target's own seed and sample count — common random numbers: sampling does not read an albedo, so the loss is the
    texels' misfit without Monte-Carlo noise and exactly 0 at the true pattern) must fall"""
    import torch
    import mitransient_amd.mi as mi
    a = ADAM
    scene = X.wall_scene(_tmp(), *a["size"], walls=("back",), max_depth=4, film=dict(res=a["res"], bins=a["bins"], start_opl=3.5, bin_width=6.0 / a["bins"]))
    key = "pattern.reflectance.data"
    yy, xx = np.mgrid[0:a["size"][1], 0:a["size"][0]]
    true = np.where(((yy // 2 + xx // 2) % 2 == 0)[..., None], np.float32([0.8, 0.2, 0.2]), np.float32([0.2, 0.3, 0.8])).astype(np.float32)
    p = mi.traverse(scene)
    p[key] = true
    p.update()
    _, target = mi.render(scene, spp=64, seed=100)
    target = target.torch().clone()
    x = torch.full(true.shape, 0.5, requires_grad=True)

    def fixed_loss():
        p[key] = x
        p.update()
        _, t = mi.render(scene, spp=64, seed=100)
        return float(torch.mean((t.torch() - target) ** 2))

    first = fixed_loss()
    opt = torch.optim.Adam([x], lr=a["lr"])
    for it in range(a["iters"]):
        opt.zero_grad()
        p[key] = x
        p.update()
        _, t = mi.render(scene, p, spp=a["spp"], seed=it + 1)
        torch.mean((t.torch() - target) ** 2).backward()
        opt.step()
        with torch.no_grad():
            x.clamp_(0.01, 1.0)
    last = fixed_loss()
    err0 = float(np.abs(0.5 - true).mean())
    err1 = float(np.abs(x.detach().numpy() - true).mean())
    return {"tier": scene.grad_tex_tier(), "loss_first": first, "loss_last": last, "factor": first / last, "texel_err_first": err0, "texel_err_last": err1}


if __name__ == "__main__":
    case = sys.argv[1]
    import torch
    torch.cuda.set_device(0)
    if case in SCENES:
        build, inst, tier = SCENES[case]
        out = gpu_vs_host(build())
        out["expected"] = [inst, tier]
    elif case == "grid_stride":
        out = grid_stride()
    elif case == "unchanged":
        out = unchanged_entry_point()
    elif case in ("autograd_slab", "autograd_global"):
        out = autograd(case.split("_")[1])
    elif case == "adam":
        out = adam()
    else:
        raise SystemExit(f"unknown case {case}")
    print(json.dumps(out))
