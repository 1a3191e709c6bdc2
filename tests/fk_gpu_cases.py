"""One GPU step of tests/test_gpu_fk_migration.py, run in a child process of its own (the test gives each step a time limit):
``python tests/fk_gpu_cases.py <case>`` prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import fk_cases as K  # noqa: E402


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def kernel_shape(name):
    """(capture, shift, desc) of a kernel-edge case: the smallest shapes at which each kernel takes another path"""
    rng = np.random.default_rng(17)
    if name in ("ragged", "q3"):               # H != W, neither a power of two; ragged shifts of both signs; q = 3: a ragged last group
        Y, g, d = K.ragged_case()
        q = 3 if name == "q3" else 1
        Tp = K.next_5_smooth(-(-(50 + int(d.max())) // q))
        return Y - np.float32(0.1), d, K.make_desc(6, 10, 50, q, Tp, 0, Tp, 0.3 * q, 0.2 * q)
    if name == "long":                         # T' = 1200: 2T' / 512 outputs per trip, more than four trips of a workgroup
        Y = rng.random((2, 3, 1190), dtype=np.float32)
        return Y, rng.integers(-3, 9, size=(2, 3)), K.make_desc(2, 3, 1190, 1, 1200, 0, 1200, 0.05, 0.07)
    if name == "unstaged":                     # T' = 9000: a spectrum row longer than the 4096 elements staged in LDS
        Y = rng.random((2, 2, 8990), dtype=np.float32)
        return Y, rng.integers(0, 9, size=(2, 2)), K.make_desc(2, 2, 8990, 1, 9000, 0, 9000, 0.011, 0.013)
    if name == "range":                        # two tiles along x and along depth, the kept rows starting and ending mid-tile
        Y = rng.random((3, 70, 150), dtype=np.float32)
        return Y, rng.integers(-2, 3, size=(3, 70)), K.make_desc(3, 70, 150, 1, 160, 13, 101, 0.4, 0.6)
    raise SystemExit(f"unknown kernel shape {name}")


def kernels(name):
    """each kernel against the host build of the same text, bit for bit, on the same inputs (the FFTs between them are torch's, on
    the device; every output starts as NaN, so an element a kernel leaves out shows)"""
    import torch
    from mitransient_amd.runtime import get_context
    Y, shift, d = kernel_shape(name)
    ctx = get_context()
    dev = torch.device("cuda", ctx.device_index)
    H, W, Tp = d.height, d.width, d.depth_bins

    def launch(entry, *tensors):
        ctx.bind_current_stream()
        ctx.check(getattr(ctx.lib, entry)(ctx.handle, C.byref(d), *(C.c_void_p(x.data_ptr()) for x in tensors)), entry)

    capture = torch.from_numpy(np.ascontiguousarray(Y, np.float32)).to(dev)
    shift_d = torch.from_numpy(np.ascontiguousarray(shift, np.int32)).to(dev)
    padded = torch.full((2 * H, 2 * W, 2 * Tp), float("nan"), dtype=torch.float32, device=dev)
    launch("mtr_fk_prepare", capture, shift_d, padded)
    spectrum = torch.fft.rfftn(padded).contiguous()
    resampled = torch.full((2 * H, 2 * W, 2 * Tp), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev)
    launch("mtr_fk_stolt", spectrum, resampled)
    field = torch.fft.ifftn(resampled).contiguous()
    volume = torch.full((d.nz, H, W), float("nan"), dtype=torch.float32, device=dev)
    launch("mtr_fk_finish", field, volume)
    torch.cuda.synchronize()
    out = {"staged": Tp + 1 <= 4096, "trips": 2.0 * Tp / 512.0}
    out["prepare"] = same_bits(padded.cpu().numpy(), K.host_prepare(d, Y, shift))
    host_g = K.host_stolt(d, spectrum.cpu().numpy())
    out["stolt"] = same_bits(resampled.cpu().numpy().view(np.float32), host_g.view(np.float32))
    out["stolt_nonzero"] = int(np.count_nonzero(host_g))
    host_v = K.host_finish(d, field.cpu().numpy())
    out["finish"] = same_bits(volume.cpu().numpy(), host_v)
    out["finite"] = bool(np.all(np.isfinite(host_v)) and np.count_nonzero(host_v) > 0)
    return out


def fft_error(capture, g):
    """torch.fft on the device against np.fft in f64 on the same padded input (the one mtr_fk_prepare wrote): rel-L2 of the spectrum"""
    import torch
    from mitransient_amd.nlos import _fk_plan
    plan = _fk_plan("fft_error", g)
    padded = K.host_prepare(plan.desc(), capture, plan.shift)
    raw = torch.fft.rfftn(torch.from_numpy(padded).cuda())
    got = raw.cpu().numpy().astype(np.complex128)
    want = np.fft.rfftn(padded.astype(np.float64))
    return float(np.linalg.norm(got - want) / np.linalg.norm(want)), bool(raw.is_contiguous())


def e2e(name):
    """fk_migration on the device against the f64 reference, on the CPU tests' cases (the rendered ones: mi.render on the device)"""
    import torch
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    out = {}
    if name == "points":
        Y, g = K.point_case()
        capture = Y
    else:
        scene = K.render_scene(name)
        _, transient = mi.render(scene, spp=K.RENDER_SPP, seed=0)
        g = mitr.nlos.capture_geometry(scene)
        capture = transient                                    # the tensor where it lies
        Y = np.array(transient)[..., 0].astype(np.float32)
    V = mitr.nlos.fk_migration(capture, g, channel=None if name == "points" else 0)
    again = mitr.nlos.fk_migration(capture, g, channel=None if name == "points" else 0)
    torch.cuda.synchronize()
    out["device"] = bool(V.is_cuda and V.dtype == torch.float32)
    V, again = V.cpu().numpy(), again.cpu().numpy()
    ref = K.reference(Y, g)
    out["shape"] = list(V.shape)
    out["depths"] = len(mitr.nlos.fk_depths(g))
    out["rel"] = K.rel_l2(V, ref)
    out["rel_host"] = K.rel_l2(V, K.host_volume(Y, g))
    out["fft_rel"], out["rfftn_contiguous"] = fft_error(Y, g)          # (the second: whether torch hands the spectrum back as it is read)
    out["same_bits"] = same_bits(V, again)
    out["peaks"] = [list(p) for p in K.two_peaks(V)]
    profile = V.astype(np.float64).sum(axis=(1, 2))
    k = int(np.argmax(profile))
    out["brightest"] = k
    out["share"] = float(V[k, 4:12, 4:12].sum() / V[k].sum()) if name != "points" else None
    part = mitr.nlos.fk_migration(capture, g, depth_range=(0.5, None), bin_factor=1, channel=None if name == "points" else 0).cpu().numpy()
    z = mitr.nlos.fk_depths(g)
    out["range_rows"] = same_bits(part, V[z >= 0.5])
    return out


if __name__ == "__main__":
    case = sys.argv[1]
    import torch
    torch.cuda.set_device(0)
    kind, name = case.split(":")
    if kind == "kernels":
        out = kernels(name)
    elif kind == "e2e":
        out = e2e(name)
    else:
        raise SystemExit(f"unknown case {case}")
    print(json.dumps(out))
