"""Shared by tests/test_forward_project.py (CPU) and tests/test_gpu_forward_project.py: the host build of mtr_forward_project.h
(tests/host_forward_project.cpp), an independent numpy f64 restatement of the transpose A^T of the backprojection — a scatter
with np.add.at that calls none of the code under test — the volumes of the parity cases, and a dense CGLS over any pair of
(forward, back) callables."""
import ctypes as C
import os
import subprocess

import numpy as np

from backproject_cases import CONFOCAL, ROOT, TOL, desc_of, positions, tiny_case  # noqa: F401  (TOL: the bar of every parity test)


def build_host_forward_project():
    """tests/host_forward_project.cpp with the flags of build_host_backproject()"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_forward_project.so")
    src = os.path.join(ROOT, "tests", "host_forward_project.cpp")
    deps = [src, os.path.join(ROOT, "include", "mitransient_amd.h")] + [os.path.join(ROOT, "mitransient_amd", "csrc", h)
                                                                       for h in ("mtr_forward_project.h", "mtr_backproject.h")]
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
        _host = C.CDLL(build_host_forward_project())
        _host.hf_plan.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
    return _host


def host_plan(nx, ny, nz, rows, T, n_cu=256):
    """fp_plan through the host build: dict(windows, slabs, slab_len, window, cap), or None when there is no plan"""
    out = (C.c_uint64 * 5)()
    if host_lib().hf_plan(nx, ny, nz, rows, T, n_cu, out) != 1:
        return None
    return dict(zip(("windows", "slabs", "slab_len", "window", "cap"), (int(v) for v in out)))


def rows_of(case):
    return case["capture"].shape[0]


def make_volume(case, kind="smooth", seed=0):
    """(nz, ny, nx) f32: "smooth" uniform random, "spiky" random^8"""
    nx, ny, nz = case["res"]
    v = np.random.default_rng(seed + 11).random((nz, ny, nx))
    return np.ascontiguousarray(v if kind == "smooth" else v ** 8, np.float32)


def reference_T(case, volume, dtype=np.float64):
    """A^T restated in numpy (f64 unless told otherwise): the (rows, T) capture a volume scatters into"""
    u = positions(case, dtype)                                   # (voxels, rows)
    T, rows = case["T"], rows_of(case)
    x = np.broadcast_to(np.asarray(volume).astype(dtype).reshape(-1, 1), u.shape)
    p = np.broadcast_to(np.arange(rows)[None, :], u.shape)
    out = np.zeros((rows, T), dtype)

    def scatter(b, val, ok):
        ok = ok & (b >= 0) & (b < T)
        np.add.at(out, (p[ok], b[ok].astype(np.int64)), val[ok])
    if case["linear"]:
        u = u - dtype(0.5)
        b0 = np.floor(u)
        w = u - b0
        both = (u >= -1) & (u < T)
        scatter(b0, (dtype(1) - w) * x, both)
        scatter(b0 + 1, w * x, both)
    else:
        scatter(np.floor(u), x, (u >= 0) & (u < T))
    return out


def host_forward_project(case, volume, expect=0, fill=np.nan):
    """the host build's capture (rows, T) f32; the output is pre-filled (NaN: every cell must be written)"""
    out = np.full((rows_of(case), case["T"]), fill, np.float32)
    vol = np.ascontiguousarray(volume, np.float32)
    d = desc_of(case, case["sp"].ctypes.data, case["lp"].ctypes.data, case["so"].ctypes.data, case["lo"].ctypes.data)
    rc = host_lib().hf_forward_project(C.byref(d), C.c_void_p(vol.ctypes.data), C.c_void_p(out.ctypes.data))
    assert rc == expect, rc
    return out


def adjoint_gap(a, x, y, b):
    """(|<a, x> - <y, b>|, TOL (|a||x| + |y||b|)) in f64 for a = A y, b = A^T x: each operator within TOL of the f64 one bounds
    the first by the second"""
    a, x, y, b = (np.asarray(v, np.float64).reshape(-1) for v in (a, x, y, b))
    return abs(a @ x - y @ b), TOL * (np.linalg.norm(a) * np.linalg.norm(x) + np.linalg.norm(y) * np.linalg.norm(b))


# ---------------------------------------------------------------- CGLS
def cgls(forward, back, y, iterations):
    """CGLS on min |A^T x - y| from x = 0 with forward = A^T and back = A (numpy arrays in and out, f64 scalars):
    (x, [|r_k| / |y| for k = 0 .. iterations])"""
    y = np.asarray(y)
    r = y.copy()
    s = back(r)
    x = np.zeros_like(s)
    p = s.copy()
    gamma = float(np.vdot(s.astype(np.float64), s.astype(np.float64)))
    ny = float(np.linalg.norm(y.astype(np.float64)))
    res = [1.0]
    for _ in range(iterations):
        if gamma == 0.0:
            res.append(res[-1])
            continue
        q = forward(p)
        alpha = gamma / float(np.vdot(q.astype(np.float64), q.astype(np.float64)))
        x = x + x.dtype.type(alpha) * p
        r = r - r.dtype.type(alpha) * q
        s = back(r)
        g2 = float(np.vdot(s.astype(np.float64), s.astype(np.float64)))
        p = s + s.dtype.type(g2 / gamma) * p
        gamma = g2
        res.append(float(np.linalg.norm(r.astype(np.float64))) / ny)
    return x, res


def cgls_case():
    """the synthetic fit: the tiny Confocal `linear` case, x0 a 4 x 4 patch in plane iz = 3 with one voxel doubled"""
    case = tiny_case(CONFOCAL, "linear")
    x0 = np.zeros((6, 6, 6), np.float32)
    x0[3, 1:5, 1:5] = 1.0
    x0[3, 2, 3] = 2.0
    return case, x0
