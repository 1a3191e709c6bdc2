#!/usr/bin/env python
"""Times nlos.backproject (mtr_backproject, csrc/mtr_backproject.hip) against the same sum written in torch ops on the same GPU —
chunked index arithmetic plus a gather, what a user of the project would write without it.

  python tools/backproject_bench.py [--workload small|config4|all] [--interpolation nearest|linear] [--kernel-only] [--reps N]

  small     a Confocal 64 x 64 x 1024 capture into 64^3 voxels        (1.07e9 gathers)
  config4   BASELINE config 4's 256 x 256 x 4096 capture into 128^3   (1.37e11 gathers; the capture is 1 GiB)

The captures are random (seeded): the cost of a backprojection does not depend on what the bins hold.  Every time is taken
with device events around calls that were warmed up; one JSON line per workload: kernel ms (median, min), baseline ms,
gathers / s, the baseline's / kernel's time, and the rel-L2 between the two volumes.  --kernel-only runs the kernel alone
(one warm-up, then --reps calls): the form a `rocprofv3 --pmc FETCH_SIZE` pass of its own wraps (WRITE_SIZE does not fit the
same pass)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WORKLOADS = {"small": dict(scan=64, T=1024, res=64, start=1.0, bin_width=0.006, reps=50, base_reps=3),
             "config4": dict(scan=256, T=4096, res=128, start=1.85, bin_width=2.0 ** -11, reps=5, base_reps=1)}
BOX = ((-1.0, -1.0, 0.5), (1.0, 1.0, 1.5))
CHUNK = 1 << 25                 # (voxel, pair) elements of the baseline's index tensors per chunk


def geometry(w):
    from mitransient_amd.nlos import CaptureGeometry
    n = w["scan"]
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    pts = np.zeros((n, n, 3))
    pts[..., 0], pts[..., 1] = c[None, :], c[:, None]
    return CaptureGeometry(2, pts, pts.reshape(-1, 3), np.zeros((n, n)), np.zeros(n * n), w["start"], w["bin_width"], w["T"])


def torch_backproject(cap, g, res, linear):
    """the baseline: (nz, ny, nx) from a (S, T) capture in torch ops, CHUNK (voxel, pair) elements at a time"""
    import torch
    dev = cap.device
    S, T = cap.shape
    sp = torch.from_numpy(g.sensor_points.reshape(-1, 3).astype(np.float32)).to(dev)
    off = torch.from_numpy((g.sensor_offset.reshape(-1) + g.laser_offset).astype(np.float32)).to(dev)
    ax = [BOX[0][k] + (torch.arange(res, device=dev, dtype=torch.float32) + 0.5) * ((BOX[1][k] - BOX[0][k]) / res) for k in range(3)]
    vz, vy, vx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    v = torch.stack([vx.reshape(-1), vy.reshape(-1), vz.reshape(-1)], dim=1)
    flat = cap.reshape(-1)
    row0 = (torch.arange(S, device=dev, dtype=torch.int64) * T)[None, :]
    out = torch.empty(v.shape[0], device=dev, dtype=torch.float32)
    step = max(1, CHUNK // S)

    def tap(b):
        ok = (b >= 0) & (b < T)
        return torch.where(ok, flat[row0 + b.clamp(0, T - 1)], torch.zeros((), device=dev))
    for v0 in range(0, v.shape[0], step):
        c = v[v0:v0 + step]
        dx, dy, dz = sp[None, :, 0] - c[:, 0:1], sp[None, :, 1] - c[:, 1:2], sp[None, :, 2] - c[:, 2:3]
        r = torch.sqrt(dx * dx + dy * dy + dz * dz)
        u = ((r + r) + off[None, :] - g.start_opl) / g.bin_width_opl
        if linear:
            u = u - 0.5
            b0 = torch.floor(u)
            w = u - b0
            b0 = b0.to(torch.int64)
            val = (1.0 - w) * tap(b0) + w * tap(b0 + 1)
        else:
            val = torch.where((u >= 0) & (u < T), tap(torch.floor(u).to(torch.int64)), torch.zeros((), device=dev))
        out[v0:v0 + step] = val.sum(dim=1)
    return out.reshape(res, res, res)


def timed(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def run(name, interpolation, kernel_only, reps):
    import torch
    from mitransient_amd.nlos import backproject
    w = WORKLOADS[name]
    g = geometry(w)
    S, T, res = w["scan"] ** 2, w["T"], w["res"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.rand((w["scan"], w["scan"], T), device="cuda", generator=gen)
    linear = interpolation == "linear"

    def kernel():
        return backproject(cap, g, BOX[0], BOX[1], res, interpolation=interpolation)
    vol = kernel()                                                   # warm-up: code object, workspace
    torch.cuda.synchronize()
    reps = reps or w["reps"]
    k_ms = timed(kernel, reps)
    gathers = float(S) * res ** 3 * (2 if linear else 1)
    out = {"workload": name, "interpolation": interpolation, "scan_points": S, "temporal_bins": T, "voxels": res ** 3,
           "gathers": gathers, "kernel_ms_median": statistics.median(k_ms), "kernel_ms_min": min(k_ms), "kernel_reps": reps,
           "gathers_per_s": gathers / (statistics.median(k_ms) * 1e-3), "device": torch.cuda.get_device_name(0)}
    if not kernel_only:
        base = torch_backproject(cap.reshape(S, T), g, res, linear)  # warm-up (and the volume to compare)
        torch.cuda.synchronize()
        b_ms = timed(lambda: torch_backproject(cap.reshape(S, T), g, res, linear), w["base_reps"])
        ref = base.double()
        out.update({"baseline_ms_median": statistics.median(b_ms), "baseline_reps": w["base_reps"],
                    "baseline_over_kernel": statistics.median(b_ms) / statistics.median(k_ms),
                    "rel_l2_kernel_vs_baseline": float(torch.linalg.norm(vol.double() - ref) / torch.linalg.norm(ref))})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["small", "config4", "all"])
    ap.add_argument("--interpolation", default="nearest", choices=["nearest", "linear"])
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--reps", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("backproject_bench: no GPU (a time taken anywhere else says nothing)")
    for name in (["small", "config4"] if a.workload == "all" else [a.workload]):
        run(name, a.interpolation, a.kernel_only, a.reps)
