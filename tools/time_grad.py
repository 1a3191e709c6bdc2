"""Time mtr_render_grad (integrator.render_backward) against the primal render of the same Cornell box, the fused and the
wavefront organisation, on cuda:0.  One JSON line per size:

    python tools/time_grad.py [--sizes 256x256x400x64,512x512x1024x1024] [--reps 3] [--textures 8x4,256x256]

Size = width x height x temporal_bins x spp (the second default is BASELINE config 2).  The upstream gradients are random; the
backward pass differentiates every key of mi.traverse (three albedos, one radiance).  Times are medians of wall-clock time
around a synchronised call, after one warm-up call.  --textures: per bitmap size W x H, the same box with that bitmap on its back
wall and floor — the backward pass with the constant keys alone (mtr_render_grad on the textured scene) and with the texels
as well (mtr_render_grad_tex; the tier it ran is reported).
--scene nlos: scenes.nlos_z (confocal; default size 256x256x4096x512, BASELINE config 4's per-GPU share) instead of the Cornell box:
render_backward over the two albedos and the laser's irradiance against the primal (fused, the NLOS tier's organisation).
--forward: the forward mode instead (mtr_render_fwd, integrator.render_forward with a tangent on every key) against the wavefront
primal and render_backward of the same build: the three are called in turn, --reps rounds after one warm-up round, medians.
--tints: the mirror-and-glass Cornell box (a tinted `conductor` small box, a tinted `dielectric` large box) instead: the fused primal,
render_backward over the albedo and radiance keys alone (mtr_render_grad), with the tint keys as well (mtr_render_grad_tint) and
render_forward with a tangent on every key (mtr_render_fwd_tint), called in turn as --forward does; the backward / primal and
forward / backward ratios of the tint-enabled calls."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x256x400x64,512x512x1024x1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--textures", default="")
    ap.add_argument("--scene", default="cornell", choices=["cornell", "nlos"])
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--tints", action="store_true")
    args = ap.parse_args()
    if args.scene == "nlos":
        return main_nlos(args)
    if args.tints:
        return main_tints(args)
    import torch
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    torch.cuda.set_device(0)
    mi.set_variant("llvm_ad_rgb")
    for size in args.sizes.split(","):
        W, H, T, spp = (int(x) for x in size.split("x"))
        d = mitr.cornell_box()
        d["sensor"]["film"].update(width=W, height=H, temporal_bins=T, start_opl=3.5, bin_width_opl=6.0 / T)
        scene = mi.load_dict(d)
        integ = scene.integrator()
        g = torch.Generator(device="cuda").manual_seed(0)
        g_s = torch.randn((H, W, 3), device="cuda", generator=g)
        g_t = torch.randn((H, W, T, 3), device="cuda", generator=g)
        p = mi.traverse(scene)
        for k in scene.grad_keys():
            p[k] = torch.tensor(p[k], requires_grad=True)
        res = {"size": size}
        if args.forward:
            tan = {k: p[k].detach() * 0.5 for k in scene.grad_keys()}
            integ.amd_mode = "wavefront"
            legs = {"primal_wavefront_ms": lambda: integ.render(scene, spp=spp, seed=0),
                    "grad_ms": lambda: integ.render_backward(scene, p, grad_in=(g_s, g_t), seed=1, spp=spp),
                    "forward_ms": lambda: integ.render_forward(scene, p, seed=1, spp=spp, tangents=tan)}
            ts = {k: [] for k in legs}
            for rep in range(args.reps + 1):                    # (round 0 warms up)
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep:
                        ts[k].append((time.perf_counter() - t0) * 1e3)
            res.update({k: statistics.median(v) for k, v in ts.items()})
            res["forward_over_grad"] = res["forward_ms"] / res["grad_ms"]
            res["forward_over_primal_wavefront"] = res["forward_ms"] / res["primal_wavefront_ms"]
            print(json.dumps(res), flush=True)
            del g_t
            continue
        for mode in ("fused", "wavefront"):
            integ.amd_mode = mode
            res[f"primal_{mode}_ms"] = timed(lambda: integ.render(scene, spp=spp, seed=0), args.reps)
        integ.amd_mode = "auto"
        res["grad_ms"] = timed(lambda: integ.render_backward(scene, p, grad_in=(g_s, g_t), seed=1, spp=spp), args.reps)
        res["ratio_vs_fused"] = res["grad_ms"] / res["primal_fused_ms"]
        res["ratio_vs_wavefront"] = res["grad_ms"] / res["primal_wavefront_ms"]
        print(json.dumps(res), flush=True)
        for tex in [t for t in args.textures.split(",") if t]:
            import tempfile
            import numpy as np
            from PIL import Image
            tw, th = (int(x) for x in tex.split("x"))
            png = os.path.join(tempfile.mkdtemp(prefix="time_grad_"), "wall.png")
            Image.fromarray(np.random.default_rng(0).integers(40, 250, (th, tw, 3), dtype=np.uint8)).save(png)
            d = mitr.cornell_box()
            d["sensor"]["film"].update(width=W, height=H, temporal_bins=T, start_opl=3.5, bin_width_opl=6.0 / T)
            d["pattern"] = dict(type="diffuse", reflectance=dict(type="bitmap", filename=png))
            d["back"]["bsdf"] = d["floor"]["bsdf"] = dict(type="ref", id="pattern")
            ts = mi.load_dict(d)
            ti = ts.integrator()
            q = mi.traverse(ts)
            for k in ts.grad_keys():
                q[k] = torch.tensor(q[k], requires_grad=True)
            r2 = {"size": size, "texture": tex, "tier": ts.grad_tex_tier()}
            r2["primal_fused_ms"] = timed(lambda: ti.render(ts, spp=spp, seed=0), args.reps)
            r2["grad_constant_keys_ms"] = timed(lambda: ti.render_backward(ts, q, grad_in=(g_s, g_t), seed=1, spp=spp), args.reps)
            q["pattern.reflectance.data"] = torch.tensor(q["pattern.reflectance.data"], requires_grad=True)
            r2["grad_with_texels_ms"] = timed(lambda: ti.render_backward(ts, q, grad_in=(g_s, g_t), seed=1, spp=spp), args.reps)
            r2["texels_over_constant"] = r2["grad_with_texels_ms"] / r2["grad_constant_keys_ms"]
            print(json.dumps(r2), flush=True)
        del g_t


def main_tints(args):
    import torch
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    torch.cuda.set_device(0)
    mi.set_variant("llvm_ad_rgb")
    for size in args.sizes.split(","):
        W, H, T, spp = (int(x) for x in size.split("x"))
        d = mitr.cornell_box()
        d["sensor"]["film"].update(width=W, height=H, temporal_bins=T, start_opl=3.5, bin_width_opl=6.0 / T)
        d["small-box"]["bsdf"] = dict(type="conductor", eta=[0.2, 0.92, 1.1], k=[3.9, 2.45, 2.14],
                                      specular_reflectance=dict(type="rgb", value=[0.8, 0.9, 0.6]))
        d["large-box"]["bsdf"] = dict(type="dielectric", int_ior=1.5, specular_reflectance=dict(type="rgb", value=[0.9, 0.7, 0.5]),
                                      specular_transmittance=dict(type="rgb", value=[0.6, 0.8, 0.95]))
        scene = mi.load_dict(d)
        integ = scene.integrator()
        g = torch.Generator(device="cuda").manual_seed(0)
        g_s = torch.randn((H, W, 3), device="cuda", generator=g)
        g_t = torch.randn((H, W, T, 3), device="cuda", generator=g)
        p, q = mi.traverse(scene), mi.traverse(scene)
        for k in scene.grad_keys():
            p[k] = torch.tensor(p[k], requires_grad=True)
            q[k] = torch.tensor(q[k], requires_grad=True)
        for k in scene.tint_keys():
            q[k] = torch.tensor(q[k], requires_grad=True)
        tan = {k: q[k].detach() * 0.5 for k in list(scene.grad_keys()) + list(scene.tint_keys())}
        legs = {"primal_fused_ms": lambda: integ.render(scene, spp=spp, seed=0),
                "grad_constant_keys_ms": lambda: integ.render_backward(scene, p, grad_in=(g_s, g_t), seed=1, spp=spp),
                "grad_with_tints_ms": lambda: integ.render_backward(scene, q, grad_in=(g_s, g_t), seed=1, spp=spp),
                "forward_with_tints_ms": lambda: integ.render_forward(scene, q, seed=1, spp=spp, tangents=tan)}
        ts = {k: [] for k in legs}
        for rep in range(args.reps + 1):                    # (round 0 warms up)
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        res = {"scene": "mirror-and-glass cornell", "size": size, "tint_keys": sorted(scene.tint_keys())}
        res.update({k: statistics.median(v) for k, v in ts.items()})
        res["tints_over_constant"] = res["grad_with_tints_ms"] / res["grad_constant_keys_ms"]
        res["backward_over_primal"] = res["grad_with_tints_ms"] / res["primal_fused_ms"]
        res["forward_over_backward"] = res["forward_with_tints_ms"] / res["grad_with_tints_ms"]
        print(json.dumps(res), flush=True)
        del g_t


def main_nlos(args):
    import torch
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    torch.cuda.set_device(0)
    mi.set_variant("llvm_ad_rgb")
    sizes = args.sizes if args.sizes != "256x256x400x64,512x512x1024x1024" else "256x256x4096x512"
    for size in sizes.split(","):
        W, H, T, spp = (int(x) for x in size.split("x"))
        from mitransient_amd.scenes import nlos_z
        scene = nlos_z(width=W, height=H, temporal_bins=T, bin_width_opl=8.0 / T, spp=spp)
        integ = scene.integrator()
        g = torch.Generator(device="cuda").manual_seed(0)
        g_s = torch.randn((H, W, 3), device="cuda", generator=g)
        g_t = torch.randn((H, W, T, 3), device="cuda", generator=g)
        p = mi.traverse(scene)
        for k in scene.grad_keys():
            p[k] = torch.tensor(p[k], requires_grad=True)
        res = {"scene": "nlos_z", "size": size, "keys": sorted(scene.grad_keys())}
        res["primal_ms"] = timed(lambda: integ.render(scene, spp=spp, seed=0), args.reps)
        res["grad_ms"] = timed(lambda: integ.render_backward(scene, p, grad_in=(g_s, g_t), seed=1, spp=spp), args.reps)
        res["ratio"] = res["grad_ms"] / res["primal_ms"]
        print(json.dumps(res), flush=True)
        del g_t


if __name__ == "__main__":
    main()
