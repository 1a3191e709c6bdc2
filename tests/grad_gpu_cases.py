"""One GPU step of tests/test_gpu_grad.py, run in a child process of its own (the test gives each step a time limit):
``python tests/grad_gpu_cases.py <case>`` prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import test_grad as T  # noqa: E402

# case: (cornell() arguments, upstream shape, the red wall's green channel set to 0)
CASES = {
    "random": ({}, "random", False), "one_bin": ({}, "one_bin", False), "steady": ({}, "steady", False),
    "zero_albedo": ({}, "random", True),
    "camera_unwarp": (dict(camera_unwarp=True, start_opl=0.0), "random", False),
    "discard_direct_light": (dict(discard_direct_light=True), "random", False),
    "hide_emitters": (dict(hide_emitters=True), "random", False), "beyond_last_bin": (dict(bins=8), "random", False),
    "crop": (dict(crop=(10, 7, 3, 5)), "random", False), "max_depth_1": (dict(max_depth=1), "random", False),
    "several": (dict(max_depth=5), "random", False), "angular": (dict(angular=True), "random", False),
}
TSHADE_BYTES = 80            # sizeof(TriShade) (mtr_core.h: MTR_TSHADE_QUADS = 5 quads): one shading record per triangle slot


def staircase():
    """a scene whose tables exceed 64 KB: walked in HBM by k_grad_paths (grad_grid stages a scene in LDS only when its tables,
    one TriShade per triangle slot among them, fit 64 KB)"""
    import mitransient_amd.mi as mi
    from mitransient_amd.scenes import staircase_like
    mi.set_variant("llvm_ad_rgb")
    d = staircase_like(tiles=6, width=16, height=16, temporal_bins=32)
    d["integrator"].update(max_depth=4, rr_depth=5)
    scene = mi.load_dict(d)
    n_tris = scene.data().tri_verts.shape[0]
    assert n_tris * TSHADE_BYTES > 64 * 1024, n_tris
    return scene


def all_params(scene):
    import torch
    import mitransient_amd.mi as mi
    p = mi.traverse(scene)
    for k in scene.grad_keys():
        p[k] = torch.tensor(p[k], dtype=torch.float32, requires_grad=True)
    return p


def gpu_vs_host(scene, kind="random", seed=3, spp=8):
    """the worst difference of any gradient element, GPU (render_backward) against the host build (same seed), relative to
    the element itself with a floor of 1e-9 of the largest gradient"""
    import torch
    hg = C.CDLL(T.build_host_grad())
    g_s, g_t = T.upstream(scene, kind)
    p = all_params(scene)
    integ = scene.integrator()
    g = integ.render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=seed, spp=spp)
    torch.cuda.synchronize()
    params = integ.render_params(scene.sensors()[0].film(), seed, spp)
    gm, ge = T.host_grad(hg, scene, params, g_s, g_t)
    keys = scene.grad_keys()
    ref = {k: (gm if kind == "material" else ge)[i] for k, (kind, i) in keys.items()}
    scale = max(float(np.abs(v).max()) for v in ref.values())
    rel = max(float(np.max(np.abs(g[k].cpu().numpy() - ref[k]) / np.maximum(np.abs(ref[k]), 1e-9 * scale))) for k in keys)
    finite = all(bool(np.all(np.isfinite(g[k].cpu().numpy()))) for k in keys)
    return {"rel": rel, "scale": scale, "n_keys": len(keys), "finite": finite,
            "all_zero_materials": all(float(np.abs(ref[k]).max()) == 0.0 for k in keys if keys[k][0] == "material")}


def passes():
    """pixel / sample ranges of one render add up to the one-call gradient; a multi-pass render_backward equals the host build
    summed over the same passes"""
    import torch
    from mitransient_amd.runtime import get_context
    scene = T.cornell()
    g_s, g_t = T.upstream(scene, "random")
    integ = scene.integrator()
    film = scene.sensors()[0].film()
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    sd = scene.data()
    gs_full = torch.from_numpy(np.ascontiguousarray(g_s)).cuda()
    gt = torch.from_numpy(np.ascontiguousarray(g_t)).cuda()

    def call(p0, p1, s0, s1):
        gm = torch.zeros((sd.n_materials, 3), device="cuda")
        ge = torch.zeros((sd.n_emitters, 3), device="cuda")
        prm = integ.render_params(film, 3, 8, s0, s1, p0, p1)
        ctx.check(ctx.lib.mtr_render_grad(h, C.byref(prm), C.c_void_p(gs_full.data_ptr()), C.c_void_p(gt.data_ptr()),
                                          C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr())), "mtr_render_grad")
        return torch.cat([gm, ge]).double().cpu().numpy()

    one = call(0, 256, 0, 8)
    parts = call(0, 100, 0, 3) + call(0, 100, 3, 8) + call(100, 256, 0, 5) + call(100, 256, 5, 8)
    split_rel = float(np.max(np.abs(parts - one) / np.maximum(np.abs(one), 1e-7 * np.abs(one).max())))   # (f32 outputs: each part rounds)
    # a render split into passes of their own seeds (common.py:56-85): 8 spp over 16 x 16 pixels, at most 1024 lanes per pass
    integ.max_wavefront_size = 1024
    integ.pass_wavefront_size = 1024
    p = all_params(scene)
    g = integ.render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=5, spp=8)
    sampler = scene.sensors()[0].sampler().clone()
    sampler.set_sample_count(8)
    sampler.set_samples_per_wavefront(8)
    ps = integ._pass_samplers(scene.sensors()[0], sampler, 5, 8, 256)
    hg = C.CDLL(T.build_host_grad())
    gm = ge = 0
    for s_i, spp_i in ps:
        prm = integ.render_params(film, s_i.seed_value(), spp_i, spp_scale=8)
        a, b = T.host_grad(hg, scene, prm, g_s, g_t)
        gm, ge = gm + a, ge + b
    keys = scene.grad_keys()
    ref = {k: (gm if kind == "material" else ge)[i] for k, (kind, i) in keys.items()}
    scale = max(float(np.abs(v).max()) for v in ref.values())
    multi_rel = max(float(np.max(np.abs(g[k].cpu().numpy() - ref[k]) / np.maximum(np.abs(ref[k]), 1e-9 * scale))) for k in keys)
    # params.update() re-uploads the colour tables of the device scene: a render equals one of a scene loaded with the new colours
    import mitransient_amd.mi as mi
    integ.max_wavefront_size, integ.pass_wavefront_size = 2 ** 32, 2 ** 26 - 1
    h_before = scene.gpu_handle(ctx, 0).value
    q = mi.traverse(scene)
    q["red.reflectance.value"] = [0.2, 0.6, 0.3]
    q["light.emitter.radiance.value"] = [5.0, 6.0, 7.0]
    q.update()
    _, t_upd = mi.render(scene, spp=8, seed=4)
    kept = scene.gpu_handle(ctx, 0).value == h_before
    fresh = T.cornell()
    d = fresh.dict_
    d["red"]["reflectance"] = dict(type="rgb", value=[0.2, 0.6, 0.3])
    d["light"]["emitter"]["radiance"] = dict(type="rgb", value=[5.0, 6.0, 7.0])
    fresh = mi.load_dict(d)
    _, t_new = mi.render(fresh, spp=8, seed=4)
    a, b = t_upd.torch().double(), t_new.torch().double()
    update_rel = float((a - b).norm() / b.norm())
    return {"split_rel": split_rel, "multi_rel": multi_rel, "n_passes": len(ps), "update_rel": update_rel, "handle_kept": kept}


def adam():
    """mi.render + torch autograd + Adam: the red wall's reflectance from 0.2 back to the Cornell box's value, with a loss on a
    time window of the transient tensor"""
    import torch
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=64, height=64, temporal_bins=64, start_opl=3.5, bin_width_opl=6.0 / 64)
    scene = mi.load_dict(d)
    key = "red.reflectance.value"
    p = mi.traverse(scene)
    true = list(p[key])
    _, target = mi.render(scene, spp=64, seed=100)
    target = target.torch()[:, :, 8:40].clone()
    x = torch.tensor([0.2, 0.2, 0.2], requires_grad=True)
    opt = torch.optim.Adam([x], lr=0.05)
    hist = []
    for it in range(40):
        opt.zero_grad()
        p[key] = x
        p.update()
        _, t = mi.render(scene, p, spp=16, seed=it + 1)
        loss = torch.mean((t.torch()[:, :, 8:40] - target) ** 2)
        loss.backward()
        opt.step()
        with torch.no_grad():
            x.clamp_(0.0, 1.0)
        hist.append(float(x[0]))
    return {"final": [float(v) for v in x.detach()], "true": true, "history": hist}


if __name__ == "__main__":
    case = sys.argv[1]
    import torch
    torch.cuda.set_device(0)
    if case in CASES:
        kw, kind, zero = CASES[case]
        scene = T.cornell(**kw)
        if zero:
            import mitransient_amd.mi as mi
            p = mi.traverse(scene)
            p["red.reflectance.value"] = [0.57, 0.0, 0.04]
            p.update()
        out = gpu_vs_host(scene, kind)
    elif case == "hbm":
        out = gpu_vs_host(staircase())
    elif case == "passes":
        out = passes()
    elif case == "adam":
        out = adam()
    else:
        raise SystemExit(f"unknown case {case}")
    print(json.dumps(out))
