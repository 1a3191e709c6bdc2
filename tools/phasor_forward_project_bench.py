#!/usr/bin/env python
"""Times nlos.phasor_forward_project (mtr_phasor_forward_project, csrc/mtr_phasor_forward_project.hip) against the same sum
written in torch ops on the same GPU — chunked over voxels, exp(-i 2 pi f tau) materialised for every (voxel, pair, frequency) —
and nlos.phasor_backproject on the same shape in the same run.

  python tools/phasor_forward_project_bench.py [--workload small|config4|all] [--weights none|gaussian] [--kernel-only] [--reps N]

The workloads, the table, the geometry and the bound are tools/phasor_backproject_bench.py's (small: Confocal 64 x 64, F = 28,
64^3, 3.01e10 terms; config4: 256 x 256, F = 28, 128^3, 3.85e12 terms); the volume is random complex (seeded).  Every time is
taken with device events around calls that were warmed up; one JSON line per workload: kernel ms (median, min), terms / s, that
rate over the f32 vector bound, phasor_backproject's ms and rate, baseline ms, the baseline's / kernel's time and the rel-L2
between the two results.  The baseline of `config4` sums the first `base_slices` z-slices of the volume and its time is scaled
to the whole (it is linear in the voxels); the kernel is compared on a volume that is zero outside those slices."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from phasor_backproject_bench import BOUND_TERMS_PER_S, BOX, CHUNK, WORKLOADS, frequencies, gaussian, geometry, timed  # noqa: E402


def torch_phasor_forward_project(u, g, freq, weights, res, slices):
    """the baseline: (S, F) complex64 from the first `slices` z-slices of a (nz, ny, nx, 2) volume in torch ops, CHUNK elements at a time"""
    import torch
    dev = u.device
    sp = torch.from_numpy(g.sensor_points.reshape(-1, 3).astype(np.float32)).to(dev)
    S, F = sp.shape[0], len(freq)
    off = torch.from_numpy((g.sensor_offset.reshape(-1) + g.laser_offset).astype(np.float32)).to(dev)
    f = torch.from_numpy(freq).to(dev) * (2.0 * np.pi)
    ax = [BOX[0][k] + (torch.arange(res, device=dev, dtype=torch.float32) + 0.5) * ((BOX[1][k] - BOX[0][k]) / res) for k in range(3)]
    vz, vy, vx = torch.meshgrid(ax[2][:slices], ax[1], ax[0], indexing="ij")
    v = torch.stack([vx.reshape(-1), vy.reshape(-1), vz.reshape(-1)], dim=1)
    uv = u[:slices].reshape(-1, 2)
    out = torch.zeros((S, F, 2), device=dev, dtype=torch.float32)
    step = max(1, CHUNK // (S * F))
    for v0 in range(0, v.shape[0], step):
        c = v[v0:v0 + step]
        a, b = uv[v0:v0 + step, 0][:, None, None], uv[v0:v0 + step, 1][:, None, None]
        dx, dy, dz = sp[None, :, 0] - c[:, 0:1], sp[None, :, 1] - c[:, 1:2], sp[None, :, 2] - c[:, 2:3]
        r = torch.sqrt(dx * dx + dy * dy + dz * dz)
        tau = (r + r) + off[None, :] - g.start_opl
        phase = tau[:, :, None] * f[None, None, :]
        zr, zi = torch.cos(phase), torch.sin(phase)
        out[..., 0] += (a * zr + b * zi).sum(dim=0)
        out[..., 1] += (b * zr - a * zi).sum(dim=0)
    if weights is not None:
        out *= torch.from_numpy(weights).to(dev)[None, :, None]
    return torch.view_as_complex(out)


def run(name, weights, kernel_only, reps):
    import torch
    from mitransient_amd.nlos import phasor_backproject, phasor_forward_project, uniform_frequency_step
    w = WORKLOADS[name]
    g = geometry(w)
    freq = frequencies()
    S, F, res = w["scan"] ** 2, len(freq), w["res"]
    wts = gaussian(freq) if weights == "gaussian" else None
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = torch.randn((res, res, res, 2), device="cuda", generator=gen)
    ph = torch.randn((w["scan"], w["scan"], F, 2), device="cuda", generator=gen)

    def kernel():
        return phasor_forward_project(u, g, freq, BOX[0], BOX[1], weights=wts)

    def partner():
        return phasor_backproject(ph, g, freq, BOX[0], BOX[1], res, weights=wts)
    kernel(), partner()                                              # warm-up: code objects, workspace
    torch.cuda.synchronize()
    reps = reps or w["reps"]
    k_ms, p_ms = timed(kernel, reps), timed(partner, reps)
    terms = float(S) * res ** 3 * F
    rate, p_rate = terms / (statistics.median(k_ms) * 1e-3), terms / (statistics.median(p_ms) * 1e-3)
    out = {"workload": name, "weights": weights, "scan_points": S, "frequencies": F, "uniform_step": uniform_frequency_step(freq),
           "voxels": res ** 3, "terms": terms, "kernel_ms_median": statistics.median(k_ms), "kernel_ms_min": min(k_ms),
           "kernel_reps": reps, "terms_per_s": rate, "fraction_of_f32_vector_bound": rate / BOUND_TERMS_PER_S,
           "phasor_backproject_ms_median": statistics.median(p_ms), "phasor_backproject_terms_per_s": p_rate,
           "kernel_over_phasor_backproject": statistics.median(k_ms) / statistics.median(p_ms),
           "device": torch.cuda.get_device_name(0)}
    if not kernel_only:
        sl = w["base_slices"]
        base = torch_phasor_forward_project(u, g, freq, wts, res, sl)      # warm-up (and the phasors to compare)
        torch.cuda.synchronize()
        b_ms = timed(lambda: torch_phasor_forward_project(u, g, freq, wts, res, sl), w["base_reps"])
        scaled = statistics.median(b_ms) * (res / sl)
        part = u.clone()
        part[sl:] = 0.0
        got = phasor_forward_project(part, g, freq, BOX[0], BOX[1], weights=wts).reshape(S, F).to(torch.complex128)
        ref = base.to(torch.complex128)
        out.update({"baseline_slices_timed": sl, "baseline_ms_median_scaled_to_the_volume": scaled, "baseline_reps": w["base_reps"],
                    "baseline_over_kernel": scaled / statistics.median(k_ms),
                    "rel_l2_kernel_vs_baseline": float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))})
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
        sys.exit("phasor_forward_project_bench: no GPU (a time taken anywhere else says nothing)")
    for name in (["small", "config4"] if a.workload == "all" else [a.workload]):
        run(name, a.weights, a.kernel_only, a.reps)
