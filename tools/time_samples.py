#!/usr/bin/env python
"""Times the three kernel organisations on films of very few pixels with very many samples: the Cornell
box with 4096 time bins, 1 x 1 and 4 x 4 `perspective` films at 2^20 and 2^22 samples per pixel, MTR_MODE_FUSED, _WAVEFRONT and
_SAMPLES of one build.  Per case: one warm-up render, then `--reps` timed ones, the modes alternating inside a repetition; the
time of a render is mtr_render's own (device events around the launches, mtr_kernel_times.total_ms) with the host's wall clock
around the synchronised call beside it.  The median is reported; a mode that cannot run a size is recorded with its error.

    python tools/time_samples.py [--reps 3] [--out profiles/samples_mode_times.txt] [--log2-spp 20 22] [--films 1 4] [--rough]

--rough: the small box a `roughconductor`, so that every mode runs its kernels with the extended shading code.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ["fused", "wavefront", "samples"]


def scene_for(side, mode, bins, rough=False):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["integrator"]["amd_mode"] = mode
    if rough:
        d["small-box"]["bsdf"] = dict(type="roughconductor", distribution="ggx", alpha=0.2)
    d["sensor"]["film"].update(width=side, height=side, temporal_bins=bins, start_opl=3.5, bin_width_opl=6.0 / bins)
    return mi.load_dict(d)


def render_once(scene, spp):
    import torch
    integ = scene.integrator()
    integ.collect_stats = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steady, transient = integ.render(scene, seed=1, spp=spp)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return float(integ.total_times["total_ms"]), wall, float(transient.torch().sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--log2-spp", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--films", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samples_mode_times.txt"))
    ap.add_argument("--rough", action="store_true", help="a roughconductor small box: the extended shading code")
    ap.add_argument("--slow-ms", type=float, default=30000.0, help="a mode whose warm-up took longer is timed once more only")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_samples.py needs the GPU (no number is taken on a CPU)"
    rows = []
    for side in a.films:
        for lg in a.log2_spp:
            spp = 1 << lg
            scenes, times, walls, sums, errors = {}, {}, {}, {}, {}
            for m in MODES:
                try:
                    scenes[m] = scene_for(side, m, a.bins, a.rough)
                    dev, wall, total = render_once(scenes[m], spp)                  # warm-up (code objects, workspaces)
                    times[m], walls[m], sums[m] = [], [], total
                    if dev > a.slow_ms:
                        times[m], walls[m] = [dev], [wall]                            # (counted: one more below)
                except Exception as e:                                                # the mode cannot run this size
                    errors[m] = f"{type(e).__name__}: {e}"
                    scenes.pop(m, None)
            for rep in range(a.reps):
                for m in MODES:
                    if m not in scenes or (rep > 0 and len(times[m]) >= 2 and max(times[m]) > a.slow_ms):
                        continue
                    dev, wall, _ = render_once(scenes[m], spp)
                    times[m].append(dev)
                    walls[m].append(wall)
            for m in MODES:
                row = {"film": f"{side}x{side}", "spp": f"2^{lg}", "mode": m}
                if m in errors:
                    row["error"] = errors[m]
                else:
                    row.update(device_ms=statistics.median(times[m]), wall_ms=statistics.median(walls[m]), n=len(times[m]),
                               min_ms=min(times[m]), max_ms=max(times[m]), film_sum=sums[m])
                rows.append(row)
                print(json.dumps(row), flush=True)
    lines = [f"# tools/time_samples.py: Cornell box, {a.bins} bins, median of the timed renders after one warm-up ({torch.cuda.get_device_name(0)})",
             "# film  spp   mode       device ms (min .. max, n)      wall ms     film sum"]
    for r in rows:
        if "error" in r:
            lines.append(f"{r['film']:5} {r['spp']:5} {r['mode']:10} {r['error']}")
        else:
            lines.append(f"{r['film']:5} {r['spp']:5} {r['mode']:10} {r['device_ms']:10.2f} ({r['min_ms']:.2f} .. {r['max_ms']:.2f}, {r['n']})"
                         f" {r['wall_ms']:10.2f}  {r['film_sum']:.6g}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
