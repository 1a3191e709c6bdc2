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


def rough_staircase():
    """staircase() with the rough materials of test_gpu_rough.py's test_rough_materials_scene_in_hbm: the extended code in HBM"""
    import mitransient_amd.mi as mi
    from mitransient_amd.scenes import staircase_like
    mi.set_variant("llvm_ad_rgb")
    d = staircase_like(tiles=6, width=16, height=16, temporal_bins=32)
    d["integrator"].update(max_depth=4, rr_depth=5)
    d["wood"] = {"type": "roughplastic", "distribution": "ggx", "alpha": 0.1, "int_ior": 1.5, "ext_ior": 1.0, "nonlinear": True,
                 "diffuse_reflectance": {"type": "rgb", "value": [0.42, 0.26, 0.13]}}
    d["steel"] = {"type": "roughconductor", "distribution": "ggx", "alpha": 0.1, "eta": [2.76, 2.54, 2.27], "k": [3.83, 3.43, 3.04]}
    d["brass"] = {"type": "twosided", "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": 0.2,
                                               "eta": [0.44, 0.53, 1.03], "k": [3.7, 2.77, 1.97]}}
    return mi.load_dict(d)


def roulette_staircase():
    """staircase_like with its own integrator (max_depth 65, rr_depth 5): roulette active, the plain code in HBM"""
    import mitransient_amd.mi as mi
    from mitransient_amd.scenes import staircase_like
    mi.set_variant("llvm_ad_rgb")
    return mi.load_dict(staircase_like(tiles=6, width=16, height=16, temporal_bins=32))


def instantiation(scene):
    """the k_grad_paths<SCENE_LDS, EXT> launch_grad picks for `scene`, from what the host scene builder reports: EXT is the
    extended shading code of its classification (scene_class_cases.host_class), SCENE_LDS whether the tables fit 64 KB.  One
    TriShade per triangle slot alone exceeds that for "hbm" (staircase()'s rule); a scene counts as "lds" here only when four
    times that (two slots per triangle, its pair record and its share of the 8-wide tree) stays below"""
    import __graft_entry__ as g
    from scene_class_cases import host_class
    ext = host_class(C.CDLL(g.build_host_harness()), scene)[1]
    n_tris = scene.data().tri_verts.shape[0]
    if n_tris * TSHADE_BYTES > 64 * 1024:
        where = "hbm"
    else:
        assert 4 * n_tris * TSHADE_BYTES <= 64 * 1024, n_tris
        where = "lds"
    return f"{where},{'ext' if ext else 'plain'}"


def _tmp():
    import pathlib
    import tempfile
    return pathlib.Path(tempfile.mkdtemp(prefix="grad_gpu_"))


# case: (scene builder, the instantiation of k_grad_paths it must run)
def _general():
    import test_grad_general as G
    cases = {f"ext_{i}": ((lambda d=d: G.rough_scene(d)), "lds,ext") for i, d in zip(("ggx", "beckmann", "aniso", "glass", "plastic"), G.ROUGH)}
    cases.update({
        "ext_textured": (lambda: G.textured(_tmp()), "lds,ext"), "ext_smooth": (lambda: G.smooth(_tmp()), "lds,ext"),
        "hbm_ext": (rough_staircase, "hbm,ext"), "hbm_rr": (roulette_staircase, "hbm,plain"),
        "rr_12": (lambda: G.degree_scene(12, 64), "lds,plain"), "rr_inf": (lambda: G.degree_scene(-1, 256), "lds,plain"),
    })
    return cases


GENERAL = ["ext_ggx", "ext_beckmann", "ext_aniso", "ext_glass", "ext_plastic", "ext_textured", "ext_smooth", "hbm_ext", "hbm_rr",
           "rr_12", "rr_inf"]


def gpu_grads(scene, g_s, g_t, seed=3, spp=8):
    """render_backward's gradients of every key as f64 arrays, and the render parameters of the same lanes"""
    import torch
    p = all_params(scene)
    integ = scene.integrator()
    g = integ.render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=seed, spp=spp)
    torch.cuda.synchronize()
    return {k: v.double().cpu().numpy() for k, v in g.items()}, integ.render_params(scene.sensors()[0].film(), seed, spp)


def oracle_emitters():
    """the kernel's emitter gradients against the oracle's linear coefficients (no mtr_grad.h on the reference's side):
    microfacet lobes, an angulararea light, roulette active.  `err` is |gpu - ref| / (1e-5 |ref| + 2^-24 |ref| + 1e-9) at worst:
    the tolerance of test_grad.py plus the rounding of the f32 output"""
    import test_grad_general as G
    scene = G.rough_scene("ggx", max_depth=6, rr_depth=2, angular=True)
    g_s, g_t = T.upstream(scene, "random")
    g, params = gpu_grads(scene, g_s, g_t)
    ref = T.emitter_coefficients(scene, params, g_s, g_t)
    keys = {k: i for k, (kind, i) in scene.grad_keys().items() if kind == "emitter"}
    got = np.array([g[k] for k, i in sorted(keys.items(), key=lambda kv: kv[1])])
    err = np.abs(got - ref) / ((1e-5 + 2.0 ** -24) * np.abs(ref) + 1e-9)
    return {"err": float(err.max()), "rel": float(np.max(np.abs(got - ref) / np.abs(ref))), "n_emitters": len(keys),
            "nonzero": bool(np.all(ref != 0)), "instantiation": instantiation(scene)}


def oracle_degree(max_depth, bins):
    """(RR-degree) of test_grad_general.py with the kernel's grad_materials on the left-hand side.  `err`: |lhs - rhs| over
    1e-5 |rhs| + 2^-24 * n_materials * max |a_m grad_m| (each f32 output rounds once), at worst over the three upstream shapes; `control`: the smallest
    relative difference when every vertex count is off by one"""
    import test_grad_general as G
    scene = G.degree_scene(max_depth, bins)
    sd = scene.data()
    mats = {i: k for k, (kind, i) in scene.grad_keys().items() if kind == "material"}
    assert sorted(mats) == list(range(sd.n_materials))
    err, rel, control = 0.0, 0.0, np.inf
    for kind in ("random", "one_bin", "steady"):
        g_s, g_t = G.degree_upstream(scene, kind)
        g, params = gpu_grads(scene, g_s, g_t)
        gm = np.array([g[mats[m]] for m in range(sd.n_materials)])
        lhs, rhs, part, _ = G.degree_sides(scene, params, g_s, g_t, gm)
        _, rhs1, _, _ = G.degree_sides(scene, params, g_s, g_t, gm, offset=1)
        err = max(err, float(np.max(np.abs(lhs - rhs) / (1e-5 * np.abs(rhs) + 2.0 ** -24 * sd.n_materials * part))))
        rel = max(rel, float(np.max(np.abs(lhs - rhs) / np.abs(rhs))))
        control = min(control, float(np.min(np.abs(lhs - rhs1) / np.abs(rhs1))))
    return {"err": err, "rel": rel, "control": control, "instantiation": instantiation(scene)}


def grid_stride():
    """k_grad_paths' grid-stride loop over more than two trips, ragged at both ends: 101 x 97 pixels, pixels [100, 9797) and
    samples [3, 112) of 113 through mtr_render_grad directly (1 056 973 lanes; the grid is capped at 8 workgroups of 256 lanes
    per compute unit) against the host build summed over 16 pixel ranges on 16 threads (measured: 1.7 s on 8 cores)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from mitransient_amd.runtime import get_context
    scene = T.cornell(res=16)
    d = scene.dict_
    d["sensor"]["film"].update(width=101, height=97)
    import mitransient_amd.mi as mi
    scene = mi.load_dict(d)
    integ = scene.integrator()
    film = scene.sensors()[0].film()
    sd = scene.data()
    g_s, g_t = T.upstream(scene, "random")
    p0, p1, s0, s1, spp = 100, 101 * 97, 3, 112, 113
    n_lanes = (p1 - p0) * (s1 - s0)
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    gs_dev, gt_dev = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()
    gm = torch.zeros((sd.n_materials, 3), device="cuda")
    ge = torch.zeros((sd.n_emitters, 3), device="cuda")
    prm = integ.render_params(film, 3, spp, s0, s1, p0, p1)
    ctx.check(ctx.lib.mtr_render_grad(h, C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()),
                                      C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr())), "mtr_render_grad")
    torch.cuda.synchronize()
    got = torch.cat([gm, ge]).double().cpu().numpy()
    hg = C.CDLL(T.build_host_grad())
    edges = np.linspace(p0, p1, 17).astype(int)
    t0 = time.time()

    def part(i):
        a, b = T.host_grad(hg, scene, integ.render_params(film, 3, spp, s0, s1, int(edges[i]), int(edges[i + 1])), g_s, g_t)
        return np.concatenate([a, b])

    with ThreadPoolExecutor(16) as pool:
        ref = sum(pool.map(part, range(16)))
    host_s = time.time() - t0
    rel = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * np.abs(ref).max())))
    return {"rel": rel, "scale": float(np.abs(ref).max()), "n_lanes": n_lanes, "grid_cap_lanes": cap, "host_seconds": host_s,
            "instantiation": instantiation(scene)}


def autograd():
    """loss.backward() through mi.render is render_backward at seed_grad / spp_grad with the loss's upstream gradients, bit for
    bit; two keys at once; a 1-element tensor on a reflectance key receives the sum of the three channels' gradients"""
    import torch
    import mitransient_amd.mi as mi
    scene = T.cornell()
    f = scene.data().film
    rng = np.random.default_rng(7)
    w_s = torch.from_numpy(rng.standard_normal((f.height, f.width, 3)).astype(np.float32)).cuda()
    w_t = torch.from_numpy(rng.standard_normal((f.temporal_bins,)).astype(np.float32)).cuda()        # a weight per time bin
    red, light = "red.reflectance.value", "light.emitter.radiance.value"
    p = mi.traverse(scene)
    x = torch.tensor([0.5, 0.2, 0.1], requires_grad=True)
    y = torch.tensor([10.0, 8.0, 6.0], requires_grad=True)
    p[red], p[light] = x, y
    p.update()
    steady, transient = mi.render(scene, p, spp=8, seed=11, seed_grad=77, spp_grad=4)
    loss = (steady.torch() * w_s).sum() + (transient.torch() * w_t[None, None, :, None]).sum()
    loss.backward()
    g_t = w_t[None, None, :, None].expand(f.height, f.width, f.temporal_bins, 3)
    ref = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=77, spp=4)
    other = scene.integrator().render_backward(scene, p, grad_in=(w_s, g_t), seed=78, spp=4)       # the seed is seen
    out = {"vector_equal": bool(torch.equal(x.grad, ref[red].cpu()) and torch.equal(y.grad, ref[light].cpu())),
           "nonzero": bool(x.grad.abs().min() > 0 and y.grad.abs().min() > 0),
           "seed_seen": not torch.equal(ref[red], other[red])}
    # the scalar branch: one value for the three channels
    q = mi.traverse(scene)
    z = torch.tensor([0.4], requires_grad=True)
    q[red] = z
    q.update()
    steady, transient = mi.render(scene, q, spp=8, seed=11, seed_grad=77, spp_grad=4)
    ((steady.torch() * w_s).sum() + (transient.torch() * w_t[None, None, :, None]).sum()).backward()
    v = mi.traverse(scene)
    v[red] = torch.tensor([0.4, 0.4, 0.4], requires_grad=True)
    v.update()
    g3 = scene.integrator().render_backward(scene, v, grad_in=(w_s, g_t), seed=77, spp=4)[red]
    out.update(scalar_equal=bool(z.grad.shape == (1,) and torch.equal(z.grad, g3.sum().reshape(1).cpu())),
               scalar=float(z.grad[0]), vector_sum=float(g3.sum()))
    return out


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
    return {"rel": rel, "scale": scale, "n_keys": len(keys), "finite": finite, "instantiation": instantiation(scene),
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
    elif case in GENERAL:
        out = gpu_vs_host(_general()[case][0]())
        out["expected"] = _general()[case][1]
    elif case == "grid_stride":
        out = grid_stride()
    elif case == "oracle_emitters":
        out = oracle_emitters()
    elif case in ("oracle_degree_12", "oracle_degree_inf"):
        out = oracle_degree(12, 64) if case.endswith("12") else oracle_degree(-1, 256)
    elif case == "autograd":
        out = autograd()
    elif case == "passes":
        out = passes()
    elif case == "adam":
        out = adam()
    else:
        raise SystemExit(f"unknown case {case}")
    print(json.dumps(out))
