"""Shared by tests/test_backproject.py (CPU) and tests/test_gpu_backproject.py: the host build of mtr_backproject.h
(tests/host_backproject.cpp), an independent numpy f64 restatement of the sum, the tiny geometry of the parity cases and the
scenes of the end-to-end check (render a quad at z = 1, backproject, the depth profile peaks at z = 1)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                  # rel-L2, the bar of every parity test here
SINGLE, CONFOCAL, EXHAUSTIVE = 1, 2, 3
ORIGIN = (-0.5, 0.0, 0.25)                  # sensor and laser origin of the offsets


def build_host_backproject():
    """tests/host_backproject.cpp with the flags of build_host_harness() (__graft_entry__.py)"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_backproject.so")
    src = os.path.join(ROOT, "tests", "host_backproject.cpp")
    deps = [src, os.path.join(ROOT, "mitransient_amd", "csrc", "mtr_backproject.h"), os.path.join(ROOT, "include", "mitransient_amd.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-o", tmp, src],
                       check=True)
        os.replace(tmp, out)
    return out


_host = None


def host_lib():
    global _host
    if _host is None:
        _host = C.CDLL(build_host_backproject())
        _host.hb_check.restype = C.c_char_p
    return _host


# ---------------------------------------------------------------- cases
def wall_points(w, h):
    """(h, w, 3) f32: the pixel centres of the wall [-1, 1]^2 x {0} in film order [y][x]"""
    x = (np.arange(w) + 0.5) / w * 2.0 - 1.0
    y = (np.arange(h) + 0.5) / h * 2.0 - 1.0
    p = np.zeros((h, w, 3), np.float32)
    p[..., 0], p[..., 1] = x[None, :], y[:, None]
    return p


def make_case(capture_type, sensor_points, laser_points, T=64, start=1.2, bin_width=0.04, vmin=(-1, -1, 0.5), vmax=(1, 1, 1.5),
              res=(6, 6, 6), offsets=False, interpolation="nearest", capture="smooth", seed=0):
    """one call's inputs, f32 as the C-ABI takes them; `capture`: "smooth", "spiky" or the (rows, T) array itself"""
    sp = np.ascontiguousarray(sensor_points, np.float32).reshape(-1, 3)
    lp = np.ascontiguousarray(laser_points, np.float32).reshape(-1, 3)
    S, L = len(sp), len(lp)
    o = np.asarray(ORIGIN, np.float64)
    so = np.linalg.norm(o - sp, axis=-1).astype(np.float32) if offsets else np.zeros(S, np.float32)
    lo = np.linalg.norm(o - lp, axis=-1).astype(np.float32) if offsets else np.zeros(L, np.float32)
    rows = S * L if capture_type == EXHAUSTIVE else S
    if isinstance(capture, str):
        if capture == "smooth":
            cap = 1.0 + 0.5 * np.sin(0.2 * np.arange(T)[None, :] + 0.37 * np.arange(rows)[:, None])
        else:
            cap = np.random.default_rng(seed).random((rows, T)) ** 8
    else:
        cap = np.asarray(capture).reshape(rows, T)
    return dict(capture_type=capture_type, sp=sp, lp=lp, so=so, lo=lo, S=S, L=L, T=int(T), start=np.float32(start),
                bin_width=np.float32(bin_width), vmin=np.asarray(vmin, np.float32), vmax=np.asarray(vmax, np.float32),
                res=tuple(int(v) for v in res), linear=interpolation == "linear", capture=np.ascontiguousarray(cap, np.float32))


def tiny_case(kind, interpolation="nearest", offsets=False, capture="smooth", **kw):
    """the tiny geometry used throughout: 8 x 8 scan points, T = 64 from 1.2 in bins of 0.04, 6^3 voxels in [-1, 1]^2 x [0.5, 1.5];
    Single: the laser point at the origin; Exhaustive: L = 3 x 2 laser points at the pixel centres of a 3 x 2 grid on the wall"""
    sp = wall_points(8, 8)
    if kind == CONFOCAL:
        lp = sp
    elif kind == SINGLE:
        lp = np.zeros((1, 3), np.float32)
    else:
        g = wall_points(2, 3)                   # [laser_x = 0..2][laser_y = 0..1], l = laser_x * 2 + laser_y
        lp = np.stack([g[..., 1], g[..., 0], g[..., 2]], axis=-1)
    return make_case(kind, sp, lp, interpolation=interpolation, offsets=offsets, capture=capture, **kw)


TINY = [(k, i, o) for k in (CONFOCAL, SINGLE, EXHAUSTIVE) for i in ("nearest", "linear") for o in (False, True)]


def pairs(case):
    """(sensor index, laser index) of every capture row, ascending"""
    S, L = case["S"], case["L"]
    if case["capture_type"] == EXHAUSTIVE:
        return np.repeat(np.arange(S), L), np.tile(np.arange(L), S)
    if case["capture_type"] == CONFOCAL:
        return np.arange(S), np.arange(S)
    return np.arange(S), np.zeros(S, np.int64)


def centres(case, dtype):
    out = []
    for k in range(3):
        n = case["res"][k]
        lo, hi = dtype(case["vmin"][k]), dtype(case["vmax"][k])
        out.append(lo + (np.arange(n).astype(dtype) + dtype(0.5)) * ((hi - lo) / dtype(n)))
    vz, vy, vx = np.meshgrid(out[2], out[1], out[0], indexing="ij")
    return np.stack([vx, vy, vz], axis=-1).reshape(-1, 3)


def positions(case, dtype):
    """u = (d - start) / bin_width of every (voxel, pair), in `dtype` with the operation order of mtr_backproject.h"""
    si, li = pairs(case)
    v = centres(case, dtype)[:, None, :]
    a = case["sp"].astype(dtype)[si][None] - v
    b = v - case["lp"].astype(dtype)[li][None]
    r1 = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
    r2 = np.sqrt((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2])
    d = ((r1 + r2) + case["so"].astype(dtype)[si][None]) + case["lo"].astype(dtype)[li][None]
    return (d - dtype(case["start"])) / dtype(case["bin_width"])


def reference(case, dtype=np.float64):
    """the backprojection restated in numpy (f64 unless told otherwise): (nz, ny, nx)"""
    u = positions(case, dtype)
    T, rows = case["T"], case["capture"].astype(dtype)
    p = np.arange(rows.shape[0])[None, :]

    def tap(b):
        ok = (b >= 0) & (b < T)
        return np.where(ok, rows[p, np.clip(b, 0, T - 1).astype(np.int64)], dtype(0))
    if case["linear"]:
        u = u - dtype(0.5)
        b0 = np.floor(u)
        w = u - b0
        val = (dtype(1) - w) * tap(b0) + w * tap(b0 + 1)
    else:
        val = np.where((u >= 0) & (u < T), tap(np.floor(u)), dtype(0))
    nx, ny, nz = case["res"]
    return val.sum(axis=1).reshape(nz, ny, nx)


def bin_disagreements(case):
    """(voxel, pair) combinations whose `nearest` bin (or in-window decision) differs between f32 and f64 arithmetic"""
    u32, u64 = positions(case, np.float32), positions(case, np.float64)
    T = case["T"]
    in32, in64 = (u32 >= 0) & (u32 < T), (u64 >= 0) & (u64 < T)
    return int(np.count_nonzero((in32 != in64) | (in32 & in64 & (np.floor(u32) != np.floor(u64)))))


def desc_of(case, sp, lp, so, lo):
    """mtr_backproject_desc of a case; sp .. lo: the addresses of the four arrays (host or device)"""
    from mitransient_amd import _cabi
    d = _cabi.mtr_backproject_desc()
    d.capture_type, d.interpolation = case["capture_type"], 1 if case["linear"] else 0
    d.n_sensor, d.n_laser, d.temporal_bins = case["S"], case["L"], case["T"]
    d.start_opl, d.bin_width_opl = case["start"], case["bin_width"]
    for k in range(3):
        d.volume_min[k], d.volume_max[k] = case["vmin"][k], case["vmax"][k]
    d.nx, d.ny, d.nz = case["res"]
    d.sensor_points, d.laser_points, d.sensor_offset, d.laser_offset = sp, lp, so, lo
    return d


def host_backproject(case, expect=0, fill=None):
    """the host build's volume (nz, ny, nx) f32"""
    nx, ny, nz = case["res"]
    vol = np.full((nz, ny, nx), np.nan if fill is None else fill, np.float32)
    d = desc_of(case, case["sp"].ctypes.data, case["lp"].ctypes.data, case["so"].ctypes.data, case["lo"].ctypes.data)
    rc = host_lib().hb_backproject(C.byref(d), C.c_void_p(case["capture"].ctypes.data), C.c_void_p(vol.ctypes.data))
    assert rc == expect, rc
    return vol


# ---------------------------------------------------------------- end to end
E2E = {"confocal": dict(capture="confocal"), "single": dict(capture="single"),
       "confocal_first_last": dict(capture="confocal", account_first_and_last_bounces=True, start=1.7)}
E2E_BOX = ((-1.0, -1.0, 0.5), (1.0, 1.0, 1.5), 16)
E2E_SPP = 64


def e2e_scene(name):
    from conftest import make_nlos
    kw = dict(sx=16, sy=16, bins=128, bin_width=0.02, start=1.2, max_depth=3, spp=E2E_SPP)
    kw.update(E2E[name])
    return make_nlos(**kw)


def depth_peak(volume):
    """z of the maximum of the depth profile summed over the central 4 x 4 columns of a (16, 16, 16) volume of E2E_BOX"""
    v = np.asarray(volume, np.float64)
    assert v.shape == (16, 16, 16)
    prof = v[:, 6:10, 6:10].sum(axis=(1, 2))
    return 0.5 + (int(np.argmax(prof)) + 0.5) / 16.0, prof
