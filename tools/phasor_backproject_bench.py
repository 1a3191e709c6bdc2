#!/usr/bin/env python
"""Times nlos.phasor_backproject (mtr_phasor_backproject, csrc/mtr_phasor_backproject.hip) against the same sum written in torch
ops on the same GPU — chunked over voxels, exp(i 2 pi f tau) materialised for every (voxel, pair, frequency), what a user of the
project would write without it.

  python tools/phasor_backproject_bench.py [--workload small|config4|all] [--weights none|gaussian] [--kernel-only] [--reps N]

  small     a Confocal 64 x 64 scan, F = 28, into 64^3 voxels      (3.01e10 terms)
  config4   BASELINE config 4's 256 x 256 scan, F = 28, into 128^3   (3.85e12 terms)

The table is the F = 28 uniform one of a phasor_hdr_film (temporal_bins 256, bin_width_opl 0.02, wl_mean 0.2, wl_sigma 0.2); the
phasors are random (seeded): the cost does not depend on what they hold.  Every time is taken with device events around calls
that were warmed up; one JSON line per workload: kernel ms (median, min), terms / s = voxels x pairs x F / time, that rate over the
f32 vector bound (157.3e12 FLOP/s / 16 FLOP per term: a term is 8 FMA-class operations), baseline ms, the baseline's / kernel's
time and the rel-L2 between the two volumes.  The baseline of `config4` runs on the first `base_slices` z-slices of the volume and
its time is scaled to the whole (it is linear in the voxels); the JSON line says so."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WORKLOADS = {"small": dict(scan=64, res=64, start=1.0, reps=20, base_reps=2, base_slices=64),
             "config4": dict(scan=256, res=128, start=1.85, reps=3, base_reps=1, base_slices=2)}
BOX = ((-1.0, -1.0, 0.5), (1.0, 1.0, 1.5))
FILM = dict(temporal_bins=256, bin_width_opl=0.02, wl_mean=0.2, wl_sigma=0.2)
CHUNK = 1 << 25                 # (voxel, pair, frequency) elements of the baseline's tensors per chunk
BOUND_TERMS_PER_S = 157.3e12 / 16.0


def frequencies():
    span = FILM["temporal_bins"] * FILM["bin_width_opl"]
    mean, sigma = span / FILM["wl_mean"], span / (FILM["wl_sigma"] * 6)
    lo, hi = max(0, int(np.floor(mean - 3 * sigma))), min(FILM["temporal_bins"] // 2, int(np.ceil(mean + 3 * sigma)))
    return np.fft.fftfreq(FILM["temporal_bins"], d=FILM["bin_width_opl"])[lo:hi + 1].astype(np.float32)


def gaussian(freq):
    return np.exp(-0.5 * ((freq.astype(np.float64) - 1.0 / FILM["wl_mean"]) * (6.0 * FILM["wl_sigma"])) ** 2).astype(np.float32)


def geometry(w):
    from mitransient_amd.nlos import CaptureGeometry
    n = w["scan"]
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    pts = np.zeros((n, n, 3))
    pts[..., 0], pts[..., 1] = c[None, :], c[:, None]
    return CaptureGeometry(2, pts, pts.reshape(-1, 3), np.zeros((n, n)), np.zeros(n * n), w["start"], FILM["bin_width_opl"],
                           FILM["temporal_bins"])


def torch_phasor_backproject(ph, g, freq, weights, res, slices):
    """the baseline: the first `slices` z-slices (slices, ny, nx) complex64 from (S, F, 2) phasors in torch ops, CHUNK elements at a time"""
    import torch
    dev = ph.device
    S, F = ph.shape[:2]
    sp = torch.from_numpy(g.sensor_points.reshape(-1, 3).astype(np.float32)).to(dev)
    off = torch.from_numpy((g.sensor_offset.reshape(-1) + g.laser_offset).astype(np.float32)).to(dev)
    f = torch.from_numpy(freq).to(dev) * (2.0 * np.pi)
    a, b = ph[..., 0], ph[..., 1]
    if weights is not None:
        wt = torch.from_numpy(weights).to(dev)
        a, b = wt[None, :] * a, wt[None, :] * b
    ax = [BOX[0][k] + (torch.arange(res, device=dev, dtype=torch.float32) + 0.5) * ((BOX[1][k] - BOX[0][k]) / res) for k in range(3)]
    vz, vy, vx = torch.meshgrid(ax[2][:slices], ax[1], ax[0], indexing="ij")
    v = torch.stack([vx.reshape(-1), vy.reshape(-1), vz.reshape(-1)], dim=1)
    out = torch.empty((v.shape[0], 2), device=dev, dtype=torch.float32)
    step = max(1, CHUNK // (S * F))
    for v0 in range(0, v.shape[0], step):
        c = v[v0:v0 + step]
        dx, dy, dz = sp[None, :, 0] - c[:, 0:1], sp[None, :, 1] - c[:, 1:2], sp[None, :, 2] - c[:, 2:3]
        r = torch.sqrt(dx * dx + dy * dy + dz * dz)
        tau = (r + r) + off[None, :] - g.start_opl
        phase = tau[:, :, None] * f[None, None, :]
        zr, zi = torch.cos(phase), torch.sin(phase)
        out[v0:v0 + step, 0] = (a[None] * zr - b[None] * zi).sum(dim=(1, 2))
        out[v0:v0 + step, 1] = (a[None] * zi + b[None] * zr).sum(dim=(1, 2))
    return torch.view_as_complex(out).reshape(slices, res, res)


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


def run(name, weights, kernel_only, reps):
    import torch
    from mitransient_amd.nlos import phasor_backproject, uniform_frequency_step
    w = WORKLOADS[name]
    g = geometry(w)
    freq = frequencies()
    S, F, res = w["scan"] ** 2, len(freq), w["res"]
    wts = gaussian(freq) if weights == "gaussian" else None
    gen = torch.Generator(device="cuda").manual_seed(1)
    ph = torch.randn((w["scan"], w["scan"], F, 2), device="cuda", generator=gen)

    def kernel():
        return phasor_backproject(ph, g, freq, BOX[0], BOX[1], res, weights=wts)
    vol = kernel()                                                   # warm-up: code object, workspace
    torch.cuda.synchronize()
    reps = reps or w["reps"]
    k_ms = timed(kernel, reps)
    terms = float(S) * res ** 3 * F
    rate = terms / (statistics.median(k_ms) * 1e-3)
    out = {"workload": name, "weights": weights, "scan_points": S, "frequencies": F, "uniform_step": uniform_frequency_step(freq),
           "voxels": res ** 3, "terms": terms, "kernel_ms_median": statistics.median(k_ms), "kernel_ms_min": min(k_ms),
           "kernel_reps": reps, "terms_per_s": rate, "fraction_of_f32_vector_bound": rate / BOUND_TERMS_PER_S,
           "device": torch.cuda.get_device_name(0)}
    if not kernel_only:
        sl = w["base_slices"]
        base = torch_phasor_backproject(ph.reshape(S, F, 2), g, freq, wts, res, sl)      # warm-up (and the volume to compare)
        torch.cuda.synchronize()
        b_ms = timed(lambda: torch_phasor_backproject(ph.reshape(S, F, 2), g, freq, wts, res, sl), w["base_reps"])
        scaled = statistics.median(b_ms) * (res / sl)
        ref = base.to(torch.complex128)
        out.update({"baseline_slices_timed": sl, "baseline_ms_median_scaled_to_the_volume": scaled, "baseline_reps": w["base_reps"],
                    "baseline_over_kernel": scaled / statistics.median(k_ms),
                    "rel_l2_kernel_vs_baseline": float(torch.linalg.norm(vol[:sl].to(torch.complex128) - ref) / torch.linalg.norm(ref))})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["small", "config4", "all"])
    ap.add_argument("--weights", default="none", choices=["none", "gaussian"])
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--reps", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("phasor_backproject_bench: no GPU (a time taken anywhere else says nothing)")
    for name in (["small", "config4"] if a.workload == "all" else [a.workload]):
        run(name, a.weights, a.kernel_only, a.reps)
