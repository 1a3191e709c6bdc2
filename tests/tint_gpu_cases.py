"""One GPU step of tests/test_gpu_grad_tint.py, run in a child process of its own (the test gives each step a time limit):
``python tests/tint_gpu_cases.py <case> [argument]`` prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import test_grad as T  # noqa: E402
import test_grad_tint as TT  # noqa: E402
from grad_gpu_cases import instantiation  # noqa: E402

TINT = dict(type="rgb", value=[0.8, 0.9, 0.6])


def tinted_staircase(rough):
    """grad_gpu_cases.staircase() / rough_staircase() with the tints of steel, brass and glass set: the tables exceed 64 KB, so the
    kernels walk the scene in HBM"""
    import mitransient_amd.mi as mi
    from mitransient_amd.scenes import staircase_like
    mi.set_variant("llvm_ad_rgb")
    d = staircase_like(tiles=6, width=16, height=16, temporal_bins=32)
    d["integrator"].update(max_depth=4, rr_depth=5)
    if rough:
        d["steel"] = {"type": "roughconductor", "distribution": "ggx", "alpha": 0.1, "eta": [2.76, 2.54, 2.27], "k": [3.83, 3.43, 3.04]}
        d["glass"] = {"type": "roughdielectric", "distribution": "beckmann", "alpha": 0.2, "int_ior": 1.5, "ext_ior": 1.0}
    d["steel"]["specular_reflectance"] = TINT
    d["brass"]["bsdf"]["specular_reflectance"] = dict(type="rgb", value=[0.9, 0.7, 0.5])
    d["glass"].update(specular_reflectance=dict(type="rgb", value=[0.9, 0.7, 0.5]), specular_transmittance=dict(type="rgb", value=[0.6, 0.8, 0.95]))
    return mi.load_dict(d)


# case: (scene builder, the instantiation of the kernels it must run)
SCENES = {
    "smooth": (lambda: TT.tint_scene("smooth"), "lds,plain"), "ggx": (lambda: TT.tint_scene("ggx"), "lds,ext"),
    "beckmann": (lambda: TT.tint_scene("beckmann"), "lds,ext"), "pane": (lambda: TT.tint_scene("pane"), "lds,ext"),
    "hbm_plain": (lambda: tinted_staircase(False), "hbm,plain"), "hbm_ext": (lambda: tinted_staircase(True), "hbm,ext"),
}


def ht():
    return C.CDLL(TT.build_host_tint())


def device_grad(scene, prm, g_s, g_t, tints=True):
    """mtr_render_grad_tint itself: (grad_materials, grad_emitters, grad_tints) as f64 arrays"""
    import torch
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    sd = scene.data()
    gs_full, gt = TT._ptrs(scene, g_s, g_t)
    gs_dev, gt_dev = torch.from_numpy(gs_full).cuda(), torch.from_numpy(gt).cuda()
    gm = torch.zeros((max(1, sd.n_materials), 3), device="cuda")
    ge = torch.zeros((max(1, sd.n_emitters), 3), device="cuda")
    gx = torch.full((max(1, scene.n_tint_slots()), 3), -7.0, device="cuda")
    ctx.check(ctx.lib.mtr_render_grad_tint(h, C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()),
                                           C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr()), None,
                                           C.c_void_p(gx.data_ptr()) if tints else None), "mtr_render_grad_tint")
    torch.cuda.synchronize()
    return tuple(x.double().cpu().numpy() for x in (gm[:sd.n_materials], ge[:sd.n_emitters], gx[:scene.n_tint_slots()]))


def device_fwd(scene, prm, tm, te, tt, sentinel=0.0):
    """mtr_render_fwd_tint itself: (steady (H, W, 3), transient (H, W, T, 3)) as f32 arrays, the outputs pre-filled"""
    import torch
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    f = scene.data().film
    d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in (tm, te, tt)]
    steady = torch.full((f.height, f.width, 3), sentinel, device="cuda")
    transient = torch.full((f.height, f.width, f.temporal_bins, 3), sentinel, device="cuda")
    ctx.check(ctx.lib.mtr_render_fwd_tint(h, C.byref(prm), C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()), None,
                                          C.c_void_p(d[2].data_ptr()), C.c_void_p(steady.data_ptr()), C.c_void_p(transient.data_ptr())),
              "mtr_render_fwd_tint")
    torch.cuda.synchronize()
    return steady.cpu().numpy(), transient.cpu().numpy()


def tangents(scene, seed=5):
    sd = scene.data()
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((max(1, sd.n_materials), 3)).astype(np.float32),
            rng.standard_normal((max(1, sd.n_emitters), 3)).astype(np.float32),
            rng.standard_normal((max(1, scene.n_tint_slots()), 3)).astype(np.float32))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def kernels(name):
    """both kernels against the host build at the same seed, and the device-side duality:  `rev`: the largest |difference| of
    grad_materials / grad_emitters / grad_tints over the largest element of the host build's; `fwd_s`, `fwd_t`: relative L2 of the
    two tangent tensors; `dual`: |sum g . J v - sum J^T g . v| over sum |g . J v|"""
    build, inst = SCENES[name]
    scene = build()
    assert instantiation(scene) == inst, (instantiation(scene), inst)
    sd = scene.data()
    lib = ht()
    prm = T.render_params(scene, spp=8)
    g_s, g_t = T.upstream(scene, "random")
    ref = np.concatenate(TT.host_grad_tint(lib, scene, prm, g_s, g_t)[:3])
    got = device_grad(scene, prm, g_s, g_t)
    tm, te, tt = tangents(scene)
    h_s, h_t = TT.host_fwd_tint(lib, scene, prm, tm, te, tt)
    d_s, d_t = device_fwd(scene, prm, tm, te, tt)
    gs_full, gt = TT._ptrs(scene, g_s, g_t)
    parts = np.concatenate([(gs_full.astype(np.float64) * d_s).reshape(-1), (gt.astype(np.float64) * d_t).reshape(-1)])
    rhs = float((got[0] * tm[:sd.n_materials]).sum() + (got[1] * te[:sd.n_emitters]).sum() + (got[2] * tt[:len(got[2])]).sum())
    # a null tint pointer: the existing entry's bits
    import torch
    from mitransient_amd.runtime import get_context
    plain = device_grad(scene, prm, g_s, g_t, tints=False)
    ctx = get_context()
    gm = torch.zeros((max(1, sd.n_materials), 3), device="cuda")
    ge = torch.zeros((max(1, sd.n_emitters), 3), device="cuda")
    gs_dev, gt_dev = torch.from_numpy(gs_full).cuda(), torch.from_numpy(gt).cuda()
    ctx.check(ctx.lib.mtr_render_grad(scene.gpu_handle(ctx, 0), C.byref(prm), C.c_void_p(gs_dev.data_ptr()), C.c_void_p(gt_dev.data_ptr()),
                                      C.c_void_p(gm.data_ptr()), C.c_void_p(ge.data_ptr())), "mtr_render_grad")
    same = bool(np.array_equal(plain[0], gm[:sd.n_materials].double().cpu().numpy()) and
                np.array_equal(plain[1], ge[:sd.n_emitters].double().cpu().numpy()) and np.all(plain[2] == -7.0))
    return {"rev": float(np.abs(np.concatenate(got) - ref).max() / np.abs(ref).max()), "tint_scale": float(np.abs(got[2]).max()),
            "fwd_s": rel_l2(d_s, h_s), "fwd_t": rel_l2(d_t, h_t), "fwd_scale": float(np.abs(h_t).max()),
            "dual": float(abs(parts.sum() - rhs) / np.abs(parts).sum()), "null_pointer_same": same, "instantiation": instantiation(scene)}


def grid_cap_lanes():
    """the most lanes one trip of a gradient or global-tier grid holds: grad_grid / fwd_plan cap the grid at 8 workgroups of 256
    lanes per compute unit"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


def host_in_ranges(fn, scene, seed, spp, p0, p1, n=16):
    """sum of fn(render parameters of a pixel range) over n ranges of [p0, p1) on n threads (the host build runs one lane at a time)"""
    from concurrent.futures import ThreadPoolExecutor
    integ, film = scene.integrator(), scene.sensors()[0].film()
    edges = np.linspace(p0, p1, n + 1).astype(int)
    with ThreadPoolExecutor(n) as pool:
        return sum(pool.map(lambda i: fn(integ.render_params(film, seed, spp, 0, spp, int(edges[i]), int(edges[i + 1]))), range(n)))


def grid_stride():
    """more lanes than one trip of the grid, ragged at both ends: 61 x 53 pixels and the first sample count whose lanes exceed the
    grid's cap (164 spp on 256 compute units), so k_grad_paths_tint's lanes stride the grid; below 256 spp a rows-tier run is one
    pixel, so k_fwd_paths_tint's 3233 runs stride its grid of at most 3 workgroups per compute unit.  Reverse: two pixel ranges
    times two sample passes sum to the whole, and the whole is the host build's.  Forward: the whole is the host build's, a pixel
    range stores its rows and leaves every other pixel at the sentinel."""
    import time
    import torch
    scene = TT.tint_scene("ggx", width=61, height=53)
    integ, film = scene.integrator(), scene.sensors()[0].film()
    g_s, g_t = T.upstream(scene, "random")
    n_pix, cap = 61 * 53, grid_cap_lanes()
    spp = cap // n_pix + 2
    assert n_pix * spp > cap and spp < 256
    n_runs, run_cap = n_pix, torch.cuda.get_device_properties(0).multi_processor_count * 3
    assert n_runs > run_cap
    s_mid = spp // 3
    whole = np.concatenate(device_grad(scene, integ.render_params(film, 3, spp), g_s, g_t))
    parts = sum(np.concatenate(device_grad(scene, integ.render_params(film, 3, spp, s0, s1, p0, p1), g_s, g_t))
                for p0, p1 in ((0, 1237), (1237, n_pix)) for s0, s1 in ((0, s_mid), (s_mid, spp)))
    lib = ht()
    t0 = time.time()
    ref = host_in_ranges(lambda prm: np.concatenate(TT.host_grad_tint(lib, scene, prm, g_s, g_t)[:3]), scene, 3, spp, 0, n_pix)
    tm, te, tt = tangents(scene)
    h_t = host_in_ranges(lambda prm: TT.host_fwd_tint(lib, scene, prm, tm, te, tt)[1], scene, 3, spp, 0, n_pix)
    host_s = time.time() - t0
    f_s, f_t = device_fwd(scene, integ.render_params(film, 3, spp), tm, te, tt, sentinel=-3.0)
    p0, p1 = 1237, 2903
    r_s, r_t = device_fwd(scene, integ.render_params(film, 3, spp, 0, spp, p0, p1), tm, te, tt, sentinel=-3.0)
    inside = np.zeros(n_pix, bool)
    inside[p0:p1] = True
    r_t2, f_t2 = r_t.reshape(n_pix, -1), f_t.reshape(n_pix, -1)
    return {"parts": float(np.abs(parts - whole).max() / np.abs(whole).max()), "host": float(np.abs(whole - ref).max() / np.abs(ref).max()),
            "fwd_host": rel_l2(f_t, h_t),
            # (f32 LDS atomics arrive in any order: the rows of two launches agree to rounding, not to the bit)
            "range_rows": max(rel_l2(r_t2[inside], f_t2[inside].astype(np.float64)),
                              rel_l2(r_s.reshape(n_pix, 3)[inside], f_s.reshape(n_pix, 3)[inside].astype(np.float64))),
            "others_at_sentinel": bool(np.all(r_t2[~inside] == -3.0) and np.all(r_s.reshape(n_pix, 3)[~inside] == -3.0)),
            "whole_written": bool(np.all(f_t != -3.0)), "n_lanes": n_pix * spp, "grid_cap_lanes": cap, "n_runs": n_runs,
            "run_cap": run_cap, "host_seconds": host_s, "instantiation": instantiation(scene)}


def fwd_tier(which):
    """the forward kernel's tiers against the host build: the rows tier below and above 256 samples per pixel, the global tier on
    a 4 x 4 film of 16384 bins with the first sample count whose lanes exceed one trip of its grid (its grid-stride loop)"""
    from mitransient_amd import _cabi
    from mitransient_amd.runtime import get_context
    film = dict(width=4, height=4)
    spp = {"rows_8": 8, "rows_300": 300, "global": grid_cap_lanes() // 16 + 3}[which]
    if which == "global":
        film.update(temporal_bins=16384, bin_width_opl=6.0 / 16384)
    scene = TT.tint_scene("ggx", **film)
    prm = T.render_params(scene, spp=spp)
    ctx = get_context()
    t = C.c_uint32(0)
    ctx.check(ctx.lib.mtr_render_fwd_tier(scene.gpu_handle(ctx, 0), C.byref(prm), C.byref(t)), "mtr_render_fwd_tier")
    tm, te, tt = tangents(scene)
    lib = ht()
    if which == "global":
        assert 16 * spp > grid_cap_lanes()
        both = host_in_ranges(lambda q: np.concatenate([x.reshape(-1) for x in TT.host_fwd_tint(lib, scene, q, tm, te, tt)]),
                              scene, 3, spp, 0, 16)
        h_s, h_t = both[:4 * 4 * 3].reshape(4, 4, 3), both[4 * 4 * 3:].reshape(4, 4, -1, 3)
    else:
        h_s, h_t = TT.host_fwd_tint(lib, scene, prm, tm, te, tt)
    d_s, d_t = device_fwd(scene, prm, tm, te, tt, sentinel=-3.0)
    return {"n_lanes": 16 * spp, "tier": {_cabi.MTR_FWD_ROWS: "rows", _cabi.MTR_FWD_GLOBAL: "global"}[int(t.value)], "fwd_s": rel_l2(d_s, h_s),
            "fwd_t": rel_l2(d_t, h_t), "scale": float(np.abs(h_t).max())}


def autograd():
    """loss.backward() through mi.render is render_backward at seed_grad / spp_grad bit for bit on a tint key (3-vector and 1-element
    value), and forward_ad through mi.render is render_forward"""
    import torch
    import torch.autograd.forward_ad as fwAD
    import mitransient_amd.mi as mi
    scene = TT.tint_scene("ggx")
    integ = scene.integrator()
    k3, k1 = "large-box.bsdf.specular_transmittance.value", "small-box.bsdf.specular_reflectance.value"
    params = mi.traverse(scene)
    v3 = torch.tensor(params[k3], dtype=torch.float32, requires_grad=True)
    v1 = torch.tensor([0.8], dtype=torch.float32, requires_grad=True)
    params[k3], params[k1] = v3, v1
    params.update()
    g_s, g_t = T.upstream(scene, "random")
    gs, gt = torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()
    s, t = mi.render(scene, params, seed=1, seed_grad=9, spp=8, spp_grad=8)
    ((s.torch() * gs).sum() + (t.torch() * gt).sum()).backward()
    ref = integ.render_backward(scene, params, grad_in=(gs, gt), seed=9, spp=8)
    back = bool(torch.equal(v3.grad.cuda(), ref[k3]) and torch.equal(v1.grad.cuda(), ref[k1].sum().reshape(1)) and
                float(v3.grad.abs().max()) > 0 and float(v1.grad.abs().max()) > 0)
    tan = torch.tensor([0.3, -0.2, 0.5])
    with fwAD.dual_level():
        params[k3] = fwAD.make_dual(v3.detach(), tan)
        params[k1] = v1.detach()
        s, t = mi.render(scene, params, seed=1, seed_grad=9, spp=8, spp_grad=8)
        j_s, j_t = fwAD.unpack_dual(s.torch()).tangent, fwAD.unpack_dual(t.torch()).tangent
    r_s, r_t = integ.render_forward(scene, params, seed=9, spp=8, tangents={k3: tan})
    fwd = bool(torch.equal(j_s, r_s.torch()) and torch.equal(j_t, r_t.torch()) and float(j_t.abs().max()) > 0)
    return {"backward_equal": back, "forward_equal": fwd}


def update():
    """params.update() of a tint on a scene that is on the device: the render of a fresh load of the same values, bit for bit"""
    import torch
    import mitransient_amd.mi as mi
    scene = TT.tint_scene("ggx")
    before = mi.render(scene, seed=3, spp=8)[1].torch().clone()
    params = mi.traverse(scene)
    params["large-box.bsdf.specular_transmittance.value"] = [0.3, 0.5, 0.7]
    params.update()
    after = mi.render(scene, seed=3, spp=8)[1].torch().clone()
    fresh = TT.tint_scene("ggx")
    fresh.dict_["large-box"]["bsdf"]["specular_transmittance"] = dict(type="rgb", value=[0.3, 0.5, 0.7])
    fresh = mi.load_dict(fresh.dict_)
    ref = mi.render(fresh, seed=3, spp=8)[1].torch()
    return {"equal": bool(torch.equal(after, ref)), "changed": bool(not torch.equal(after, before))}


ADAM_KEY = "mirror.specular_reflectance.value"
ADAM_TRUE, ADAM_START, ADAM_STEPS, ADAM_SPP, ADAM_LR = [0.9, 0.6, 0.3], [0.5, 0.5, 0.5], 60, 64, 0.03


def adam_scene():
    """the Cornell box at 16 x 16 pixels and 64 bins whose two boxes and back wall are one top-level `conductor`, "mirror", grey"""
    import mitransient_amd as mitr
    d = mitr.cornell_box()
    d["integrator"].update(max_depth=5, rr_depth=6)
    d["sensor"]["film"].update(width=16, height=16, temporal_bins=64, start_opl=3.5, bin_width_opl=6.0 / 64)
    d["mirror"] = dict(type="conductor", **TT.COPPER, specular_reflectance=dict(type="rgb", value=list(ADAM_START)))
    for name in ("small-box", "large-box", "back"):
        d[name]["bsdf"] = dict(type="ref", id="mirror")
    return T._mi().load_dict(d)


def adam():
    """mi.render + torch autograd + Adam: the mirror's tint from grey to ADAM_TRUE from a transient target (the README's example) rendered at the
    primal's own seed — the loss is exactly 0 at the true tint — with a fresh gradient seed every step;
    test_grad_tint.py rehearses it on the CPU with the oracle as primal and the host build as render_backward"""
    import torch
    import mitransient_amd.mi as mi
    scene = adam_scene()
    p = mi.traverse(scene)
    p[ADAM_KEY] = ADAM_TRUE
    p.update()
    _, target = mi.render(scene, spp=ADAM_SPP, seed=100)
    target = target.torch().clone()
    x = torch.tensor(ADAM_START, requires_grad=True)
    opt = torch.optim.Adam([x], lr=ADAM_LR)
    hist, losses = [], []
    for it in range(ADAM_STEPS):
        opt.zero_grad()
        p[ADAM_KEY] = x
        p.update()
        _, t = mi.render(scene, p, spp=ADAM_SPP, seed=100, seed_grad=it + 1)
        loss = torch.sum((t.torch() - target) ** 2)
        loss.backward()
        opt.step()
        with torch.no_grad():
            x.clamp_(0.01, 1.0)
        hist.append([float(v) for v in x.detach()])
        losses.append(float(loss))
    return {"final": hist[-1], "true": ADAM_TRUE, "losses_thirds": [float(np.mean(losses[i:i + 20])) for i in (0, 20, 40)]}


if __name__ == "__main__":
    case = sys.argv[1]
    fn = {"kernels": kernels, "grid_stride": grid_stride, "fwd_tier": fwd_tier, "autograd": autograd, "update": update, "adam": adam}[case]
    print(json.dumps(fn(*sys.argv[2:])))
