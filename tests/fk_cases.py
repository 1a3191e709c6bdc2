"""What the f-k migration tests share (tests/test_fk_migration.py on the CPU, tests/fk_gpu_cases.py on the GPU): an independent
f64 NumPy reference written from the operator's definition (not from csrc/mtr_fk.h), the host build of mtr_fk.h
(tests/host_fk.cpp) behind ctypes, the host pipeline (host stages around torch's CPU FFT in f32) and the synthetic cases."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFOCAL = 2


# ---------------------------------------------------------------- the host build
def build_host_fk():
    """tests/host_fk.cpp with the flags of test_grad_nlos.build_host_grad_nlos()"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_fk.so")
    srcs = [os.path.join(ROOT, "tests", "host_fk.cpp")]
    deps = srcs + [os.path.join(ROOT, "mitransient_amd", "csrc", "mtr_fk.h"), os.path.join(ROOT, "include", "mitransient_amd.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-o", tmp] + srcs,
                       check=True)
        os.replace(tmp, out)
    return out


_lib = None


def host_lib():
    global _lib
    if _lib is None:
        from mitransient_amd import _cabi
        lib = C.CDLL(build_host_fk())
        vp, dp = C.c_void_p, C.POINTER(_cabi.mtr_fk_desc)
        lib.hfk_desc_size.restype = C.c_int
        lib.hfk_check.restype = C.c_char_p
        lib.hfk_check.argtypes = [dp, vp, vp]
        lib.hfk_prepare.argtypes = [dp, vp, vp, vp]
        lib.hfk_stolt.argtypes = [dp, vp, vp]
        lib.hfk_finish.argtypes = [dp, vp, vp]
        _lib = lib
    return _lib


def make_desc(H, W, T, q, Tp, z0, nz, ax, ay):
    from mitransient_amd import _cabi
    d = _cabi.mtr_fk_desc()
    d.height, d.width, d.temporal_bins, d.bin_factor, d.depth_bins, d.z_begin, d.nz = H, W, T, q, Tp, z0, nz
    d.ax, d.ay = np.float32(ax), np.float32(ay)
    return d


def host_prepare(d, capture, shift):
    capture, shift = np.ascontiguousarray(capture, np.float32), np.ascontiguousarray(shift, np.int32)
    out = np.full((2 * d.height, 2 * d.width, 2 * d.depth_bins), np.nan, np.float32)
    host_lib().hfk_prepare(C.byref(d), capture.ctypes.data, shift.ctypes.data, out.ctypes.data)
    return out


def host_stolt(d, spectrum):
    spectrum = np.ascontiguousarray(spectrum, np.complex64)
    assert spectrum.shape == (2 * d.height, 2 * d.width, d.depth_bins + 1)
    out = np.full((2 * d.height, 2 * d.width, 2 * d.depth_bins), np.nan, np.complex64)
    host_lib().hfk_stolt(C.byref(d), spectrum.ctypes.data, out.ctypes.data)
    return out


def host_finish(d, field):
    field = np.ascontiguousarray(field, np.complex64)
    assert field.shape == (2 * d.height, 2 * d.width, 2 * d.depth_bins)
    out = np.full((d.nz, d.height, d.width), np.nan, np.float32)
    host_lib().hfk_finish(C.byref(d), field.ctypes.data, out.ctypes.data)
    return out


def host_volume(capture, geometry, depth_range=None, bin_factor=1):
    """fk_migration with the host build in place of the kernels and torch's CPU FFT (f32) in place of the device's"""
    import torch
    from mitransient_amd.nlos import _fk_plan
    plan = _fk_plan("host_volume", geometry, depth_range, bin_factor)
    d = plan.desc()
    padded = host_prepare(d, capture, plan.shift)
    spectrum = torch.fft.rfftn(torch.from_numpy(padded)).numpy()
    field = torch.fft.ifftn(torch.from_numpy(host_stolt(d, spectrum))).numpy()
    return host_finish(d, field)


# ---------------------------------------------------------------- the f64 reference
def next_5_smooth(n):
    n = max(int(n), 1)
    while True:
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def signed(n2):
    """signed FFT indices of an axis of n2 points: 0 .. n2/2 - 1, -n2/2 .. -1"""
    i = np.arange(n2)
    return np.where(i < n2 // 2, i, i - n2).astype(np.float64)


def stolt_f64(F, H, W, Tp, ax, ay, misread=None):
    """the Stolt resampling of a (2H, 2W, T' + 1) half spectrum in f64; returns (G, p) with p the fractional source index"""
    F = np.asarray(F, np.complex128)
    ky, kx, kz = signed(2 * H)[:, None, None] / H, signed(2 * W)[None, :, None] / W, signed(2 * Tp)[None, None, :] / Tp
    kp = np.sqrt((ax * kx) ** 2 + (ay * ky) ** 2 + kz ** 2)
    p = kp * Tp
    i0 = np.floor(p).astype(np.int64)
    w = p - i0
    valid = (kz > 0) & ((i0 <= Tp) if misread == "edge" else (i0 + 1 <= Tp))
    Fz = np.concatenate([F, np.zeros(F.shape[:2] + (1,), F.dtype)], axis=2)          # (only the "edge" misreading reads the zero)
    ic = np.clip(i0, 0, Tp)
    G = (1.0 - w) * np.take_along_axis(Fz, ic, 2) + w * np.take_along_axis(Fz, ic + 1, 2)
    if misread != "jacobian":
        with np.errstate(invalid="ignore", divide="ignore"):
            G = G * (kz / kp)
    return np.where(valid, G, 0.0), p


def reference(capture, geometry, depth_range=None, bin_factor=1, misread=None):
    """The operator in f64 NumPy, (nz, H, W).  misread: None, or one of the wrong readings the tests hold the product away from —
    "spacing" (the lateral spacing doubled), "shift" (the capture one bin late), "jacobian" (kz / k' left out), "edge" (the tap
    pair allowed to leave the half spectrum by one)."""
    g = geometry
    Y = np.asarray(capture, np.float64)
    H, W, T = Y.shape
    q, bw = int(bin_factor), float(g.bin_width_opl)
    P = g.sensor_points
    dx, dy = np.linalg.norm(P[0, 1] - P[0, 0]), np.linalg.norm(P[1, 0] - P[0, 0])
    if misread == "spacing":
        dx, dy = 2.0 * dx, 2.0 * dy
    off = g.sensor_offset.reshape(H, W) + g.laser_offset.reshape(H, W)
    shift = np.rint((g.start_opl - off) / bw).astype(np.int64)
    n = -(-(T + max(int(shift.max()), 0)) // q)
    zmin, zmax = (0.0, np.inf) if depth_range is None else (0.0 if depth_range[0] is None else depth_range[0],
                                                            np.inf if depth_range[1] is None else depth_range[1])
    if np.isfinite(zmax):
        n = min(n, int(math.ceil(2.0 * zmax / (q * bw))))
    Tp = next_5_smooth(n)
    if misread == "shift":
        shift = shift + 1
    fine = np.zeros((H, W, Tp * q))
    for y in range(H):
        for x in range(W):
            j = np.arange(T) + shift[y, x]
            ok = (j >= 0) & (j < Tp * q)
            fine[y, x, j[ok]] = Y[y, x, ok]
    S = fine.reshape(H, W, Tp, q).sum(axis=-1)
    padded = np.zeros((2 * H, 2 * W, 2 * Tp))
    padded[:H, :W, :Tp] = np.sqrt(np.maximum(S, 0.0)) * ((np.arange(Tp) + 0.5) / Tp)
    dz = q * bw / 2.0
    G, _ = stolt_f64(np.fft.rfftn(padded), H, W, Tp, dz / dx, dz / dy, misread)
    field = np.fft.ifftn(G)
    V = np.transpose(np.abs(field[:H, :W, :Tp]) ** 2, (2, 0, 1))
    z = (np.arange(Tp) + 0.5) * dz
    return V[(z >= zmin) & (z <= zmax)]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---------------------------------------------------------------- cases
def grid_geometry(H, W, dx, dy, T, bin_width, start=0.0, offset=None):
    """a Confocal CaptureGeometry on the wall z = 0, centred on the origin, x right and y up; offset (H, W): the sensor legs"""
    from mitransient_amd.nlos import CaptureGeometry
    pts = np.zeros((H, W, 3))
    pts[..., 0] = ((np.arange(W) + 0.5) - W / 2.0)[None, :] * dx
    pts[..., 1] = ((np.arange(H) + 0.5) - H / 2.0)[:, None] * dy
    so = np.zeros((H, W)) if offset is None else np.asarray(offset, np.float64)
    return CaptureGeometry(CONFOCAL, pts, pts.reshape(-1, 3).copy(), so, np.zeros(H * W), start, bin_width, T)


POINTS = ((0.3, -0.2, 1.0, 1.0), (-0.4, 0.5, 0.6, 0.5))


def point_case():
    """two point scatterers seen by a 32 x 32 confocal scan of a 2 x 2 wall: Y[y, x, floor(2 r / bin_width)] += a / r^4"""
    H = W = 32
    T, bw = 256, 0.02
    g = grid_geometry(H, W, 1.0 / 16, 1.0 / 16, T, bw)
    Y = np.zeros((H, W, T), np.float32)
    for (px, py, pz, a) in POINTS:
        r = np.sqrt((g.sensor_points[..., 0] - px) ** 2 + (g.sensor_points[..., 1] - py) ** 2 + pz ** 2)
        b = np.floor(2.0 * r / bw).astype(np.int64)
        yy, xx = np.nonzero(b < T)
        np.add.at(Y, (yy, xx, b[yy, xx]), (a / r ** 4)[yy, xx].astype(np.float32))
    return Y, g


def ragged_case(H=6, W=10, T=50, seed=3):
    """a random capture whose scan points start at ragged whole-bin offsets on both sides of the wall-to-wall origin"""
    rng = np.random.default_rng(seed)
    bw = 0.03125
    d = rng.integers(-7, 9, size=(H, W))
    g = grid_geometry(H, W, 0.07, 0.05, T, bw, start=0.25, offset=0.25 - d * bw)     # shift = d
    return rng.random((H, W, T), dtype=np.float32), g, d


def two_peaks(V):
    """(argmax, argmax with the first one's 5-voxel neighbourhood zeroed) of a (nz, ny, nx) volume"""
    V = np.array(V, np.float64)
    first = np.unravel_index(int(np.argmax(V)), V.shape)
    lo = [max(c - 5, 0) for c in first]
    V[lo[0]:first[0] + 6, lo[1]:first[1] + 6, lo[2]:first[2] + 6] = 0.0
    return tuple(int(c) for c in first), tuple(int(c) for c in np.unravel_index(int(np.argmax(V)), V.shape))


def render_scene(hidden):
    """the 16 x 16 confocal scene of the rendered-capture tests: a quad or a 'Z' one unit behind the wall"""
    from conftest import make_nlos
    return make_nlos(sx=16, sy=16, capture="confocal", bins=128, bin_width=0.03, start=1.85, spp=64, max_depth=3, hidden=hidden)


RENDER_SPP = 64
Z1_SAMPLE = 1.0 / 0.015 - 0.5            # the (fractional) depth sample of z = 1: 66.17
