"""Times the polarization notebook's render (cornell-box/cbox_polarized.xml: 256 x 256, 400 bins, max_depth 5, 4096 spp),
polarized (llvm_ad_mono_polarized) and as llvm_ad_mono, both in the wavefront organisation, and prints one JSON line.
The scene's `Au` is substituted as in tests/test_polarized.py (an explicit gold-like eta / k).  Wrap it in
`rocprofv3 --kernel-trace --stats -- python tools/time_polarized.py` to see where the time goes.

    python tools/time_polarized.py [--spp 4096] [--reps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4096)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    import mitransient_amd.mi as mi
    from test_polarized import CBOX, cbox_polarized_dict
    out = {"spp": args.spp, "res": args.res}
    for variant in ("llvm_ad_mono_polarized", "llvm_ad_mono"):
        mi.set_variant(variant)
        scene = mi.load_dict(cbox_polarized_dict(res=args.res), base_dir=CBOX)
        integ = scene.integrator()
        integ.amd_mode = "wavefront"
        ms = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s, t = integ.render(scene, spp=args.spp)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        integ.collect_stats = True
        integ.render(scene, spp=args.spp)
        torch.cuda.synchronize()
        out[variant] = {"ms": ms, "median_ms": sorted(ms)[len(ms) // 2], "counters": {k: v for k, v in integ.last_counters.items() if k != "reserved"},
                        "kernel_times": dict(integ.last_times)}
    out["ratio"] = out["llvm_ad_mono_polarized"]["median_ms"] / out["llvm_ad_mono"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
