"""One GPU step of tests/test_gpu_grad_nlos_texture.py, run in a child process of its own (the test gives each step a time limit):
``python tests/grad_nlos_tex_gpu_cases.py <case>`` prints one JSON line."""
import ctypes as C
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import test_grad as T  # noqa: E402
import test_grad_nlos as N  # noqa: E402
import test_grad_nlos_texture as NT  # noqa: E402
from grad_tex_gpu_cases import rel_errors, tex_params, upload  # noqa: E402
from conftest import make_nlos  # noqa: E402


def _tmp():
    return pathlib.Path(tempfile.mkdtemp(prefix="grad_nlos_tex_"))


def instantiation(scene):
    """the k_grad_paths_nlos_tex<TEX> launch_grad picks: every NLOS scene is staged in LDS, a bitmap implies the extended shading
    code (checked against the host scene builder), TEX from the tier the library reports"""
    import __graft_entry__ as g
    from scene_class_cases import host_class
    ext = host_class(C.CDLL(g.build_host_harness()), scene)[1]
    return f"nlos,lds,{'ext' if ext else 'plain'},{scene.grad_tex_tier()}"


def host_all(scene, params, g_s, g_t):
    """the host build's gradients in the layout of the device outputs: materials, the laser, the texels of every texture"""
    hgnt = C.CDLL(NT.build_host_grad_nlos_tex())
    gm, gl, gx = NT.host_grad_nlos_tex(hgnt, scene, params, g_s, g_t)
    return np.concatenate([gm, gl[None]] + [t.reshape(-1, 3) for t in gx])


def call_tex(scene, prm, g_s, g_t, texels=True, entry="tex"):
    """mtr_render_grad_tex (entry "tex"; texels False: a NULL grad_texels) or mtr_render_grad directly: (materials + laser, texels)"""
    import torch
    from mitransient_amd.runtime import get_context
    sd = scene.data()
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    gs_dev, gt_dev = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()
    n_tx = sum(int(t.shape[0] * t.shape[1]) for t in sd.textures)
    gm = torch.zeros((sd.n_materials, 3), device="cuda")
    ge = torch.zeros((1, 3), device="cuda")
    gx = torch.full((n_tx, 3), 7.0 if texels else 0.0, device="cuda")                    # (stored, not added to)
    args = [h, C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()), C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr())]
    if entry == "plain":
        ctx.check(ctx.lib.mtr_render_grad(*args), "mtr_render_grad")
    else:
        ctx.check(ctx.lib.mtr_render_grad_tex(*args, C.c_void_p(gx.data_ptr()) if texels else None), "mtr_render_grad_tex")
    torch.cuda.synchronize()
    return torch.cat([gm, ge]).cpu(), gx.cpu()


def gpu_vs_host(scene, seed=3, spp=8):
    """render_backward over every key against the host build: texels relative to the largest texel gradient, materials and the
    laser element by element (a floor of 1e-9 of the largest)"""
    import torch
    g_s, g_t = T.upstream(scene, "random")
    upload(scene)
    p = tex_params(scene)
    integ = scene.integrator()
    g = integ.render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=seed, spp=spp)
    torch.cuda.synchronize()
    params = integ.render_params(scene.sensors()[0].film(), seed, spp)
    hgnt = C.CDLL(NT.build_host_grad_nlos_tex())
    gm, gl, gx = NT.host_grad_nlos_tex(hgnt, scene, params, g_s, g_t)
    out = {"tier": scene.grad_tex_tier(), "instantiation": instantiation(scene), "finite": True, "rel_texels": 0.0, "n_textures": 0}
    for k, i in scene.texture_keys().items():
        if k in g:
            got = g[k].double().cpu().numpy()
            out["finite"] = out["finite"] and bool(np.all(np.isfinite(got)))
            out["rel_texels"] = max(out["rel_texels"], rel_errors(got, gx[i]))
            out["texel_scale"] = float(np.abs(gx[i]).max())
            out["same_support"] = bool(np.array_equal(got != 0.0, gx[i] != 0.0))
            out["device_ok"] = g[k].is_cuda and tuple(g[k].shape) == tuple(scene.data().textures[i].shape)
            out["n_textures"] += 1
    keys = scene.grad_keys()
    ref = {k: (gm[i] if kind == "material" else gl) for k, (kind, i) in keys.items()}
    scale = max(float(np.abs(v).max()) for v in ref.values())
    out["rel_other"] = max(float(np.max(np.abs(g[k].cpu().numpy() - ref[k]) / np.maximum(np.abs(ref[k]), 1e-9 * scale))) for k in keys)
    return out


def host_cases(w, h, cases):
    return {c: gpu_vs_host(NT.tex_nlos_scene(_tmp(), c, w=w, h=h)) for c in cases}


def grid_stride(w, h):
    """k_grad_paths_nlos_tex's grid-stride loop on a second trip, ragged at both ends — grad_nlos_gpu_cases.grid_stride's lanes: 61 x
    53 pixels, pixels [50, 3233) and samples [3, 236) of 237 — through mtr_render_grad_tex directly, a w x h bitmap on the quad and
    on the wall, against the host build summed over 16 pixel ranges"""
    from concurrent.futures import ThreadPoolExecutor
    import torch
    scene = NT.tex_nlos_scene(_tmp(), "single_hg_wall", on="both", w=w, h=h, sx=61, sy=53, bins=32)
    upload(scene)
    integ = scene.integrator()
    film = scene.sensors()[0].film()
    sd = scene.data()
    g_s, g_t = T.upstream(scene, "random")
    p0, p1, s0, s1, spp = 50, 61 * 53, 3, 236, 237
    me, gx = call_tex(scene, integ.render_params(film, 3, spp, s0, s1, p0, p1), g_s, g_t)
    got = torch.cat([me, gx]).double().numpy()
    edges = np.linspace(p0, p1, 17).astype(int)
    NT.build_host_grad_nlos_tex()

    def part(i):
        return host_all(scene, integ.render_params(film, 3, spp, s0, s1, int(edges[i]), int(edges[i + 1])), g_s, g_t)

    with ThreadPoolExecutor(16) as pool:
        ref = sum(pool.map(part, range(16)))
    n_me = sd.n_materials + 1
    return {"tier": scene.grad_tex_tier(), "instantiation": instantiation(scene), "rel_texels": rel_errors(got[n_me:], ref[n_me:]),
            "rel_other": rel_errors(got[:n_me], ref[:n_me]), "n_lanes": (p1 - p0) * (s1 - s0),
            "grid_cap_lanes": torch.cuda.get_device_properties(0).multi_processor_count * 3 * 256}


def passes():
    """pixel / sample ranges of one render add up to the one-call gradient (texels included); a multi-pass render_backward equals
    the host build summed over the same passes"""
    import torch
    scene = NT.tex_nlos_scene(_tmp(), "confocal_ls_hg", on="both")
    upload(scene)
    g_s, g_t = T.upstream(scene, "random")
    integ = scene.integrator()
    film = scene.sensors()[0].film()

    def call(p0, p1, s0, s1):
        return torch.cat(call_tex(scene, integ.render_params(film, 3, 8, s0, s1, p0, p1), g_s, g_t)).double().numpy()

    one = call(0, 64, 0, 8)
    parts = call(0, 20, 0, 3) + call(0, 20, 3, 8) + call(20, 64, 0, 5) + call(20, 64, 5, 8)
    split_rel = rel_errors(parts, one)
    integ.max_wavefront_size = 256
    integ.pass_wavefront_size = 256
    p = tex_params(scene)
    gs_dev, gt_dev = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()
    g = integ.render_backward(scene, p, grad_in=(gs_dev, gt_dev), seed=5, spp=8)
    sampler = scene.sensors()[0].sampler().clone()
    sampler.set_sample_count(8)
    sampler.set_samples_per_wavefront(8)
    ps = integ._pass_samplers(scene.sensors()[0], sampler, 5, 8, 64)
    ref = sum(host_all(scene, integ.render_params(film, s_i.seed_value(), spp_i, spp_scale=8), g_s, g_t) for s_i, spp_i in ps)
    n_me = scene.data().n_materials + 1
    key = [k for k in scene.texture_keys() if k in g][0]
    got = g[key].double().cpu().numpy().reshape(-1, 3)
    return {"split_rel": split_rel, "multi_rel": rel_errors(got, ref[n_me:]), "n_passes": len(ps), "tier": scene.grad_tex_tier(),
            "nonzero": float(np.abs(one[n_me:]).max()) > 0}


def unchanged_entry_point():
    """mtr_render_grad on a textured NLOS scene: the host build of the walk without a texel hook (tests/host_grad_nlos.cpp, the
    parent's arithmetic), what mtr_render_grad_tex gives for materials and the laser bit for bit, textured materials 0"""
    import torch
    scene = NT.tex_nlos_scene(_tmp(), "single_hg_wall", on="hidden")
    upload(scene)
    sd = scene.data()
    g_s, g_t = T.upstream(scene, "random")
    prm = scene.integrator().render_params(scene.sensors()[0].film(), 3, 8)
    plain = call_tex(scene, prm, g_s, g_t, texels=False, entry="plain")
    tex = call_tex(scene, prm, g_s, g_t)
    null = call_tex(scene, prm, g_s, g_t, texels=False)
    textured = [m for m in range(sd.n_materials) if sd.materials[m].albedo_texture]
    hm, hl = N.host_grad_nlos(C.CDLL(N.build_host_grad_nlos()), scene, prm, g_s, g_t)
    ref = np.concatenate([hm, hl[None]])
    got = plain[0].double().numpy()
    return {"same_as_tex": bool(torch.equal(plain[0], tex[0])), "null_is_plain": bool(torch.equal(plain[0], null[0]) and float(null[1].abs().max()) == 0.0),
            "textured_zero": bool(all(float(plain[0][m].abs().max()) == 0.0 for m in textured)), "n_textured": len(textured),
            "texels_written": bool(float(tex[1].abs().max()) > 0 and not bool((tex[1] == 7.0).any())),
            "rel_host": float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * np.abs(ref).max())))}


def oracle_degree(case, max_depth):
    """(Degree) of test_grad_nlos_texture.py with the kernel's gradients on the left-hand side, the oracle's splat log on the right:
    no mtr_grad.h on the reference's side.  `err`: |lhs - rhs| over 1e-5 |rhs| + 2^-24 * (the sum of |t grad_t| and |a_m grad_m|): each
    f32 output rounds once"""
    import torch
    scene = NT.degree_scene(_tmp(), case, max_depth)
    upload(scene)
    sd = scene.data()
    g_s, g_t = T.upstream(scene, "random")
    g_s[:] = 0
    prm = T.render_params(scene, spp=64)
    me, gx = call_tex(scene, prm, g_s, g_t)
    gm = me[:-1].double().numpy()
    gx = gx.double().numpy()
    per, at = [], 0
    for t in sd.textures:
        k = int(t.shape[0] * t.shape[1])
        per.append(gx[at:at + k].reshape(t.shape))
        at += k
    lhs, rhs, rhs1, tex_part, (d0, d1, n) = NT.degree_check(scene, prm, g_t, gm, per, NT.DEGREE_CASES[case][1])
    mag = sum(np.abs(sd.textures[i].astype(np.float64) * per[i]).sum(axis=(0, 1)) for i in range(len(per))) + \
        sum(np.abs(np.array([sd.materials[m].a[k] for k in range(3)]) * gm[m]) for m in range(sd.n_materials))
    return {"err": float(np.max(np.abs(lhs - rhs) / (1e-5 * np.abs(rhs) + 2.0 ** -24 * mag))), "rel": float(np.max(np.abs(lhs - rhs) / np.abs(rhs))),
            "control": float(np.min(np.abs(lhs - rhs1) / np.abs(rhs1))), "share": float(np.min(np.abs(tex_part) / np.abs(rhs))),
            "n_terms": n, "deepest": d1, "instantiation": instantiation(scene)}


def autograd(which):
    """loss.backward() on a `.data` tensor against render_backward at seed_grad / spp_grad: bit for bit on the slab tier, within
    1e-6 of the largest element on the global tier (arrival order of the f64 atomics: the f32 output can round either way)"""
    import torch
    import mitransient_amd.mi as mi
    scene = NT.tex_nlos_scene(_tmp(), "confocal_ls_hg", w=4 if which == "slab" else 20, h=3 if which == "slab" else 18)
    f = scene.data().film
    rng = np.random.default_rng(7)
    w_s = torch.from_numpy(rng.standard_normal((f.height, f.width, 3)).astype(np.float32)).cuda()
    w_t = torch.from_numpy(rng.standard_normal((f.temporal_bins,)).astype(np.float32)).cuda()
    key, wall, laser = "hidden.bsdf.reflectance.data", "relay_wall.bsdf.reflectance.value", "laser.irradiance.value"
    p = mi.traverse(scene)
    x = torch.tensor(scene.data().textures[0], requires_grad=True)                     # a CPU tensor: its gradient arrives on the CPU
    y = torch.tensor([0.5, 0.2, 0.1], requires_grad=True)
    z = torch.tensor([2.0, 1.0, 3.0], requires_grad=True)
    p[key], p[wall], p[laser] = x, y, z
    p.update()
    steady, transient = mi.render(scene, p, spp=8, seed=11, seed_grad=77, spp_grad=4)
    has_fn = steady.torch().grad_fn is not None and transient.torch().grad_fn is not None
    loss = (steady.torch() * w_s).sum() + (transient.torch() * w_t[None, None, :, None]).sum()
    loss.backward()
    g_t = w_t[None, None, :, None].expand(f.height, f.width, f.temporal_bins, 3)
    ref = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=77, spp=4)
    other = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=78, spp=4)
    a, b = x.grad.double(), ref[key].cpu().double()
    return {"tier": scene.grad_tex_tier(), "equal": bool(torch.equal(x.grad, ref[key].cpu())), "rel": float((a - b).abs().max() / b.abs().max()),
            "shape_ok": tuple(x.grad.shape) == tuple(x.shape) and not x.grad.is_cuda and ref[key].is_cuda, "grad_fn": has_fn,
            "constant_equal": bool(torch.equal(y.grad, ref[wall].cpu()) and torch.equal(z.grad, ref[laser].cpu())),
            "nonzero": float((x.grad != 0).float().mean()), "seed_seen": not torch.equal(ref[key], other[key])}


# the Adam fit: an 8 x 8 two-colour checker on the hidden quad from uniform grey, a Confocal capture of 8 x 8 scanned points x 256
# bins, laser and hidden-geometry sampling on — the size of grad_nlos_gpu_cases.ADAM
ADAM = dict(sx=8, sy=8, bins=256, bin_width=2.0 ** -6, spp=64, capture="confocal", nlos_laser_sampling=True,
            nlos_hidden_geometry_sampling=True, rr_depth=5)
ADAM_SIZE, ADAM_STEPS, ADAM_SPP, ADAM_LR, ADAM_TARGET = (8, 8), 60, 64, 0.01, (100, 256)       # target: (seed, spp)


def adam_true():
    yy, xx = np.mgrid[0:ADAM_SIZE[1], 0:ADAM_SIZE[0]]
    return np.where(((yy // 2 + xx // 2) % 2 == 0)[..., None], np.float32([0.8, 0.2, 0.2]), np.float32([0.2, 0.3, 0.8])).astype(np.float32)


def adam_scene(tmp):
    from test_grad_texture import write_png
    write_png(tmp / "checker.png", *ADAM_SIZE)
    return make_nlos(hidden_bsdf=NT.textured_diffuse(tmp / "checker.png"), **ADAM)


def adam():
    """mi.render + torch autograd + Adam on the `.data` tensor of the hidden quad.  The loss (the squared error summed over the
    transient tensor) is evaluated before and after at the target's own seed and sample count — common random numbers: sampling does
    not read an albedo, so it is the texels' misfit without Monte-Carlo noise, exactly 0 at the true pattern"""
    import torch
    import mitransient_amd.mi as mi
    scene = adam_scene(_tmp())
    key = "hidden.bsdf.reflectance.data"
    true = adam_true()
    p = mi.traverse(scene)
    p[key] = true
    p.update()
    _, target = mi.render(scene, spp=ADAM_TARGET[1], seed=ADAM_TARGET[0])
    target = target.torch().clone()
    x = torch.full(true.shape, 0.5, requires_grad=True)

    def fixed_loss():
        p[key] = x
        p.update()
        _, t = mi.render(scene, spp=ADAM_TARGET[1], seed=ADAM_TARGET[0])
        return float(torch.sum((t.torch() - target) ** 2))

    first = fixed_loss()
    opt = torch.optim.Adam([x], lr=ADAM_LR)
    for it in range(ADAM_STEPS):
        opt.zero_grad()
        p[key] = x
        p.update()
        _, t = mi.render(scene, p, spp=ADAM_SPP, seed=it + 1)
        torch.sum((t.torch() - target) ** 2).backward()
        opt.step()
        with torch.no_grad():
            x.clamp_(0.01, 1.0)
    last = fixed_loss()
    return {"tier": scene.grad_tex_tier(), "loss_first": first, "loss_last": last, "factor": first / last,
            "texel_err_first": float(np.abs(0.5 - true).mean()), "texel_err_last": float(np.abs(x.detach().numpy() - true).mean())}


if __name__ == "__main__":
    case = sys.argv[1]
    import torch
    torch.cuda.set_device(0)
    if case.startswith("host:"):
        _, size, names = case.split(":")
        w, h = (int(v) for v in size.split("x"))
        out = host_cases(w, h, names.split(","))
    elif case.startswith("grid_stride:"):
        w, h = (int(v) for v in case.split(":")[1].split("x"))
        out = grid_stride(w, h)
    elif case == "passes":
        out = passes()
    elif case == "unchanged":
        out = unchanged_entry_point()
    elif case.startswith("oracle_degree:"):
        _, c, d = case.split(":")
        out = oracle_degree(c, int(d))
    elif case in ("autograd_slab", "autograd_global"):
        out = autograd(case.split("_")[1])
    elif case == "adam":
        out = adam()
    else:
        raise SystemExit(f"unknown case {case}")
    print(json.dumps(out))
