"""One GPU step of tests/test_gpu_grad_nlos.py, run in a child process of its own (the test gives each step a time limit):
``python tests/grad_nlos_gpu_cases.py <case>`` prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import test_grad as T  # noqa: E402
import test_grad_nlos as N  # noqa: E402
from grad_gpu_cases import all_params  # noqa: E402


def instantiation(scene):
    """the k_grad_paths_nlos<EXT> launch_grad picks: every NLOS scene is staged in LDS; EXT from the host scene builder"""
    import __graft_entry__ as g
    from scene_class_cases import host_class
    ext = host_class(C.CDLL(g.build_host_harness()), scene)[1]
    return f"nlos,lds,{'ext' if ext else 'plain'}"


def gpu_grads(scene, g_s, g_t, seed=3, spp=8):
    import torch
    p = all_params(scene)
    integ = scene.integrator()
    g = integ.render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=seed, spp=spp)
    torch.cuda.synchronize()
    return {k: v.double().cpu().numpy() for k, v in g.items()}, integ.render_params(scene.sensors()[0].film(), seed, spp)


def host_reference(scene, params, g_s, g_t):
    hgn = C.CDLL(N.build_host_grad_nlos())
    gm, gl = N.host_grad_nlos(hgn, scene, params, g_s, g_t)
    return {k: (gm[i] if kind == "material" else gl) for k, (kind, i) in scene.grad_keys().items()}


def worst(g, ref):
    scale = max(float(np.abs(v).max()) for v in ref.values())
    return max(float(np.max(np.abs(g[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-9 * scale))) for k in ref), scale


def gpu_vs_host(scene, spp=8):
    g_s, g_t = T.upstream(scene, "random")
    g, params = gpu_grads(scene, g_s, g_t, spp=spp)
    ref = host_reference(scene, params, g_s, g_t)
    rel, scale = worst(g, ref)
    return {"rel": rel, "scale": scale, "n_keys": len(ref), "finite": all(bool(np.all(np.isfinite(v))) for v in g.values()),
            "laser": any(k.endswith(".irradiance.value") for k in ref), "instantiation": instantiation(scene)}


def zero_albedo():
    scene = N.nlos_scene("confocal_ls_hg")
    N.set_albedo(scene, N.relay_material(scene), [0.8, 0.0, 0.7])
    out = gpu_vs_host(scene)
    return out


def grid_stride():
    """more than two trips of the grid-stride loop, ragged at both ends: 61 x 53 pixels, pixels [50, 3233) and samples [3, 236) of
    237 through mtr_render_grad directly, against the host build summed over 16 pixel ranges"""
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from mitransient_amd.runtime import get_context
    scene = N.nlos_scene("single_hg_wall", sx=61, sy=53, bins=32)
    integ = scene.integrator()
    film = scene.sensors()[0].film()
    sd = scene.data()
    g_s, g_t = T.upstream(scene, "random")
    p0, p1, s0, s1, spp = 50, 61 * 53, 3, 236, 237
    n_lanes = (p1 - p0) * (s1 - s0)
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 3 * 256       # kGradNlosPerCu workgroups of 256 lanes
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    gs_dev, gt_dev = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()
    gm = torch.zeros((sd.n_materials, 3), device="cuda")
    ge = torch.zeros((1, 3), device="cuda")
    prm = integ.render_params(film, 3, spp, s0, s1, p0, p1)
    ctx.check(ctx.lib.mtr_render_grad(h, C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()),
                                      C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr())), "mtr_render_grad")
    torch.cuda.synchronize()
    got = torch.cat([gm, ge]).double().cpu().numpy()
    hgn = C.CDLL(N.build_host_grad_nlos())
    edges = np.linspace(p0, p1, 17).astype(int)

    def part(i):
        a, b = N.host_grad_nlos(hgn, scene, integ.render_params(film, 3, spp, s0, s1, int(edges[i]), int(edges[i + 1])), g_s, g_t)
        return np.concatenate([a, b[None]])

    with ThreadPoolExecutor(16) as pool:
        ref = sum(pool.map(part, range(16)))
    rel = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * np.abs(ref).max())))
    return {"rel": rel, "scale": float(np.abs(ref).max()), "n_lanes": n_lanes, "grid_cap_lanes": cap, "instantiation": instantiation(scene)}


def passes():
    """pixel / sample ranges of one render add up to the one-call gradient; a multi-pass render_backward equals the host build
    summed over the same passes"""
    import torch
    from mitransient_amd.runtime import get_context
    scene = N.nlos_scene("confocal_ls_hg")
    g_s, g_t = T.upstream(scene, "random")
    integ = scene.integrator()
    film = scene.sensors()[0].film()
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    sd = scene.data()
    gs_dev, gt_dev = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()

    def call(p0, p1, s0, s1):
        gm = torch.zeros((sd.n_materials, 3), device="cuda")
        ge = torch.zeros((1, 3), device="cuda")
        prm = integ.render_params(film, 3, 8, s0, s1, p0, p1)
        ctx.check(ctx.lib.mtr_render_grad(h, C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()),
                                          C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr())), "mtr_render_grad")
        return torch.cat([gm, ge]).double().cpu().numpy()

    one = call(0, 64, 0, 8)
    parts = call(0, 20, 0, 3) + call(0, 20, 3, 8) + call(20, 64, 0, 5) + call(20, 64, 5, 8)
    split_rel = float(np.max(np.abs(parts - one) / np.maximum(np.abs(one), 1e-7 * np.abs(one).max())))
    integ.max_wavefront_size = 256
    integ.pass_wavefront_size = 256
    p = all_params(scene)
    g = integ.render_backward(scene, p, grad_in=(gs_dev, gt_dev), seed=5, spp=8)
    g = {k: v.double().cpu().numpy() for k, v in g.items()}
    sampler = scene.sensors()[0].sampler().clone()
    sampler.set_sample_count(8)
    sampler.set_samples_per_wavefront(8)
    ps = integ._pass_samplers(scene.sensors()[0], sampler, 5, 8, 64)
    hgn = C.CDLL(N.build_host_grad_nlos())
    gm = gl = 0
    for s_i, spp_i in ps:
        a, b = N.host_grad_nlos(hgn, scene, integ.render_params(film, s_i.seed_value(), spp_i, spp_scale=8), g_s, g_t)
        gm, gl = gm + a, gl + b
    ref = {k: (gm[i] if kind == "material" else gl) for k, (kind, i) in scene.grad_keys().items()}
    multi_rel, _ = worst(g, ref)
    return {"split_rel": split_rel, "multi_rel": multi_rel, "n_passes": len(ps)}


def autograd():
    """loss.backward() through mi.render is render_backward at seed_grad / spp_grad with the loss's upstream gradients, bit for bit"""
    import torch
    import mitransient_amd.mi as mi
    scene = N.nlos_scene("confocal_ls_hg")
    f = scene.data().film
    rng = np.random.default_rng(7)
    w_s = torch.from_numpy(rng.standard_normal((f.height, f.width, 3)).astype(np.float32)).cuda()
    w_t = torch.from_numpy(rng.standard_normal((f.temporal_bins,)).astype(np.float32)).cuda()
    hid, laser = "hidden.bsdf.reflectance.value", "laser.irradiance.value"
    p = mi.traverse(scene)
    x = torch.tensor([0.5, 0.2, 0.1], requires_grad=True)
    y = torch.tensor([2.0, 1.0, 3.0], requires_grad=True)
    p[hid], p[laser] = x, y
    p.update()
    steady, transient = mi.render(scene, p, spp=8, seed=11, seed_grad=77, spp_grad=4)
    loss = (steady.torch() * w_s).sum() + (transient.torch() * w_t[None, None, :, None]).sum()
    loss.backward()
    g_t = w_t[None, None, :, None].expand(f.height, f.width, f.temporal_bins, 3)
    ref = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=77, spp=4)
    other = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=78, spp=4)
    return {"vector_equal": bool(torch.equal(x.grad, ref[hid].cpu()) and torch.equal(y.grad, ref[laser].cpu())),
            "nonzero": bool(x.grad.abs().min() > 0 and y.grad.abs().min() > 0), "seed_seen": not torch.equal(ref[hid], other[hid])}


def oracle_laser(case):
    """the kernel's laser gradient against the oracle's linear coefficients (no mtr_grad.h on the reference's side), roulette
    active.  `err`: |gpu - ref| / (1e-5 |ref| + 2^-24 |ref|) at worst — the tolerance plus the rounding of the f32 output"""
    scene = N.nlos_scene(case, max_depth=8, rr_depth=2)
    scene.emitters()[0].irradiance = [3.0, 0.0, 1.5]
    g_s, g_t = T.upstream(scene, "random")
    g, params = gpu_grads(scene, g_s, g_t)
    got = g["laser.irradiance.value"]
    ref = N.laser_coefficients(scene, params, g_s, g_t)
    err = np.abs(got - ref) / ((1e-5 + 2.0 ** -24) * np.abs(ref))
    return {"err": float(err.max()), "rel": float(np.max(np.abs(got - ref) / np.abs(ref))), "nonzero": bool(np.all(ref != 0)),
            "instantiation": instantiation(scene)}


def oracle_degree(case, max_depth):
    """(RR-degree) of test_grad_nlos.py with the kernel's grad_materials on the left-hand side.  `err`: |lhs - rhs| over
    1e-5 |rhs| + 2^-24 * n_materials * max |a_m grad_m| (each f32 output rounds once)"""
    scene = N.degree_scene(case, max_depth)
    sd = scene.data()
    g_s, g_t = T.upstream(scene, "random")
    g_s[:] = 0
    g, params = gpu_grads(scene, g_s, g_t, spp=64)
    mats = {i: k for k, (kind, i) in scene.grad_keys().items() if kind == "material"}
    gm = np.array([g[mats[m]] for m in range(sd.n_materials)])
    ls = N.DEGREE_CASES[case]
    lhs, rhs, part, (d0, d1, n) = N.degree_sides(scene, params, g_t, gm, ls)
    _, rhs1, _, _ = N.degree_sides(scene, params, g_t, gm, ls, offset=1)
    return {"err": float(np.max(np.abs(lhs - rhs) / (1e-5 * np.abs(rhs) + 2.0 ** -24 * sd.n_materials * part))),
            "rel": float(np.max(np.abs(lhs - rhs) / np.abs(rhs))), "control": float(np.min(np.abs(lhs - rhs1) / np.abs(rhs1))),
            "n_terms": n, "deepest": d1, "instantiation": instantiation(scene)}


ADAM = dict(sx=8, sy=8, bins=256, bin_width=2.0 ** -6, spp=64)
ADAM_TRUE, ADAM_START, ADAM_STEPS, ADAM_SPP, ADAM_LR = [0.6, 0.4, 0.8], [0.2, 0.2, 0.2], 60, 64, 0.03


def adam_scene():
    import pathlib
    import tempfile
    return N.make_nlos_z(pathlib.Path(tempfile.mkdtemp(prefix="grad_nlos_")), **ADAM)


def adam(render_and_grad=None):
    """mi.render + torch autograd + Adam: the hidden Z's albedo from 0.2 back to ADAM_TRUE from a confocal transient of
    make_nlos_z at 8 x 8.  render_and_grad: test_gpu_grad_nlos's CPU rehearsal passes the oracle / host build in its place"""
    import torch
    import mitransient_amd.mi as mi
    scene = adam_scene()
    key = "Z.bsdf.reflectance.value"
    p = mi.traverse(scene)
    p[key] = ADAM_TRUE
    p.update()
    _, target = mi.render(scene, spp=256, seed=100)
    target = target.torch().clone()
    x = torch.tensor(ADAM_START, requires_grad=True)
    opt = torch.optim.Adam([x], lr=ADAM_LR)
    hist, losses = [], []
    for it in range(ADAM_STEPS):
        opt.zero_grad()
        p[key] = x
        p.update()
        _, t = mi.render(scene, p, spp=ADAM_SPP, seed=it + 1)
        loss = torch.sum((t.torch() - target) ** 2)
        loss.backward()
        opt.step()
        with torch.no_grad():
            x.clamp_(0.01, 1.0)
        hist.append([float(v) for v in x.detach()])
        losses.append(float(loss))
    return {"final": hist[-1], "true": ADAM_TRUE, "history": hist, "losses": losses}


if __name__ == "__main__":
    case = sys.argv[1]
    import torch
    torch.cuda.set_device(0)
    if case.startswith("host:"):
        out = gpu_vs_host(N.nlos_scene(case[5:]))
    elif case == "zero_albedo":
        out = zero_albedo()
    elif case == "grid_stride":
        out = grid_stride()
    elif case == "passes":
        out = passes()
    elif case == "autograd":
        out = autograd()
    elif case.startswith("oracle_laser:"):
        out = oracle_laser(case.split(":")[1])
    elif case.startswith("oracle_degree:"):
        _, c, d = case.split(":")
        out = oracle_degree(c, int(d))
    elif case == "adam":
        out = adam()
    else:
        raise SystemExit(f"unknown case {case}")
    print(json.dumps(out))
