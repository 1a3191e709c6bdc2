#!/usr/bin/env python
"""Times nlos.forward_project (mtr_forward_project, csrc/mtr_forward_project.hip) against the same scatter written in torch ops on
the same GPU — chunked index arithmetic plus index_add_, what a user of the project would write without it — and beside
nlos.backproject on the same shape.

  python tools/forward_project_bench.py [--workload small|config4|all] [--interpolation nearest|linear] [--kernel-only]
                                        [--reps N] [--fill F]

  small     64^3 voxels into a Confocal 64 x 64 x 1024 capture        (1.07e9 (voxel, row) pairs)
  config4   128^3 voxels into BASELINE config 4's 256 x 256 x 4096    (1.37e11 pairs; the capture is 1 GiB)

The volumes are random (seeded) and dense unless --fill F keeps a fraction F of the voxels and zeroes the rest (the kernel
skips zeros; the baseline does not).  Every time is taken with device events around calls that were warmed up; one JSON line per
workload: kernel ms (median, min), adds / s, backproject's ms on the same shape, baseline ms, the baseline's / kernel's time, and
the rel-L2 between the two captures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from backproject_bench import BOX, CHUNK, WORKLOADS, geometry, timed  # noqa: E402


def torch_forward_project(x, g, T, linear, chunks=None):
    """the baseline: (S, T) from a (nz, ny, nx) volume in torch ops, CHUNK (voxel, pair) elements at a time (`chunks`: stop after
    that many — a warm-up)"""
    import torch
    dev = x.device
    res = x.shape[0]
    S = g.sensor_points.shape[0] * g.sensor_points.shape[1]
    sp = torch.from_numpy(g.sensor_points.reshape(-1, 3).astype(np.float32)).to(dev)
    off = torch.from_numpy((g.sensor_offset.reshape(-1) + g.laser_offset).astype(np.float32)).to(dev)
    ax = [BOX[0][k] + (torch.arange(res, device=dev, dtype=torch.float32) + 0.5) * ((BOX[1][k] - BOX[0][k]) / res) for k in range(3)]
    vz, vy, vx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    v = torch.stack([vx.reshape(-1), vy.reshape(-1), vz.reshape(-1)], dim=1)
    xs = x.reshape(-1)
    row0 = (torch.arange(S, device=dev, dtype=torch.int64) * T)[None, :]
    out = torch.zeros(S * T, device=dev, dtype=torch.float32)
    step = max(1, CHUNK // S)

    def add(b, val):
        ok = (b >= 0) & (b < T)
        out.index_add_(0, (row0 + b.clamp(0, T - 1)).reshape(-1), torch.where(ok, val, torch.zeros((), device=dev)).reshape(-1))
    for n, v0 in enumerate(range(0, v.shape[0], step)):
        if chunks is not None and n >= chunks:
            break
        c = v[v0:v0 + step]
        dx, dy, dz = sp[None, :, 0] - c[:, 0:1], sp[None, :, 1] - c[:, 1:2], sp[None, :, 2] - c[:, 2:3]
        r = torch.sqrt(dx * dx + dy * dy + dz * dz)
        u = ((r + r) + off[None, :] - g.start_opl) / g.bin_width_opl
        val = xs[v0:v0 + step, None].expand_as(u)
        if linear:
            u = u - 0.5
            b0 = torch.floor(u)
            w = u - b0
            b0 = b0.to(torch.int64)
            add(b0, (1.0 - w) * val)
            add(b0 + 1, w * val)
        else:
            add(torch.floor(u).to(torch.int64), torch.where((u >= 0) & (u < T), val, torch.zeros((), device=dev)))
    return out.reshape(S, T)


def run(name, interpolation, kernel_only, reps, fill):
    import torch
    from mitransient_amd.nlos import backproject, forward_project
    w = WORKLOADS[name]
    g = geometry(w)
    S, T, res = w["scan"] ** 2, w["T"], w["res"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((res, res, res), device="cuda", generator=gen)
    if fill < 1.0:
        x = torch.where(torch.rand((res, res, res), device="cuda", generator=gen) < fill, x, torch.zeros((), device="cuda"))
    linear = interpolation == "linear"

    def kernel():
        return forward_project(x, g, BOX[0], BOX[1], interpolation=interpolation)
    cap = kernel()                                                   # warm-up: code object, workspace
    torch.cuda.synchronize()
    reps = reps or w["reps"]
    k_ms = timed(kernel, reps)
    bp_ms = timed(lambda: backproject(cap, g, BOX[0], BOX[1], res, interpolation=interpolation), reps + 1)[1:]
    adds = float(S) * res ** 3 * (2 if linear else 1)
    out = {"workload": name, "interpolation": interpolation, "scan_points": S, "temporal_bins": T, "voxels": res ** 3, "fill": fill,
           "adds": adds, "kernel_ms_median": statistics.median(k_ms), "kernel_ms_min": min(k_ms), "kernel_reps": reps,
           "adds_per_s": adds / (statistics.median(k_ms) * 1e-3), "backproject_ms_median": statistics.median(bp_ms), "device": torch.cuda.get_device_name(0)}
    if not kernel_only:
        torch_forward_project(x, g, T, linear, chunks=2)             # warm-up
        torch.cuda.synchronize()
        base = []
        b_ms = timed(lambda: base.append(torch_forward_project(x, g, T, linear)), w["base_reps"])
        ref = base[-1].double()
        out.update({"baseline_ms_median": statistics.median(b_ms), "baseline_reps": w["base_reps"],
                    "baseline_over_kernel": statistics.median(b_ms) / statistics.median(k_ms),
                    "rel_l2_kernel_vs_baseline": float(torch.linalg.norm(cap.reshape(S, T).double() - ref) / torch.linalg.norm(ref))})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["small", "config4", "all"])
    ap.add_argument("--interpolation", default="nearest", choices=["nearest", "linear"])
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--fill", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("forward_project_bench: no GPU (a time taken anywhere else says nothing)")
    for name in (["small", "config4"] if a.workload == "all" else [a.workload]):
        run(name, a.interpolation, a.kernel_only, a.reps, a.fill)
