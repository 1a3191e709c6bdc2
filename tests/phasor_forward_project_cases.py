"""Shared by tests/test_phasor_forward_project.py (CPU) and tests/test_gpu_phasor_forward_project.py: the host build of
mtr_phasor_forward_project.h (tests/host_phasor_forward_project.cpp), an independent numpy f64 restatement of the sum
Q[p, k] = w_k sum over v of M(v, p) U(v) exp(-i 2 pi f_k tau), a numpy f32 restatement in the header's operation order, the dense
operator of a tiny case and the CGLS yardstick on it.  Geometry, tables and the bar are phasor_backproject_cases.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import phasor_backproject_cases as pc
from phasor_backproject_cases import ANCHOR, CONFOCAL, EXHAUSTIVE, PARITY, PB_TOL, SINGLE  # noqa: F401  (re-exported)

ROOT = pc.ROOT
# The bar of every parity test here is PB_TOL = 1e-4, rel-L2 over the rows: the terms are the z of phasor_backproject, whose f32
# phase rounding set that bar.  Measured before relying on it (test_f32_restatement_is_within_the_bar): the numpy f32 restatement
# (reference_f32) against f64 over the parity grid in both forms with random complex volumes is at worst 2.30e-5 (F = 151; the host build 2.30e-5 as
# well) — below PB_TOL / 4 = 2.5e-5, the figure the test holds the restatement to.
F32_WORST = PB_TOL / 4
# the bound of the adjoint identity, forward_project's form: |<A y, x> - <y, A^H x>| <= ADJOINT_TOL (|Ay| |x| + |y| |A^H x|)
ADJOINT_TOL = 1e-5


def build_host_phasor_forward_project():
    """tests/host_phasor_forward_project.cpp with the flags of build_host_phasor_backproject()"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_phasor_forward_project.so")
    src = os.path.join(ROOT, "tests", "host_phasor_forward_project.cpp")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "mitransient_amd.h")] + [os.path.join(csrc, h) for h in (
        "mtr_phasor_forward_project.h", "mtr_phasor_backproject.h", "mtr_backproject.h", "mtr_core.h", "mtr_flat_prims.h",
        "mtr_shadow_hull.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-o", tmp, src],
                       check=True)
        os.replace(tmp, out)
    return out


_host = None
PLAN_ARGS = [C.c_uint32] * 3 + [C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]


def host_lib():
    global _host
    if _host is None:
        _host = C.CDLL(build_host_phasor_forward_project())
        _host.hpf_check.restype = C.c_char_p
        _host.hpf_plan.argtypes = PLAN_ARGS
    return _host


def plan_of(fn, nx, ny, nz, rows, F, n_cu):
    """(n_blocks, n_slabs, slab_len) of pf_plan through `fn` (the host build's hpf_plan or the library's hook), or None"""
    out = (C.c_uint32 * 5)()
    if fn(nx, ny, nz, rows, F, n_cu, out) != 1:
        return None
    assert out[4] == ANCHOR
    return out[0], out[1], out[2] | (out[3] << 32)


# ---------------------------------------------------------------- cases
def rows_of(case):
    return case["S"] * case["L"] if case["capture_type"] == EXHAUSTIVE else case["S"]


def random_volume(case, seed=0):
    """a random complex volume as (nz, ny, nx, 2) f32"""
    nx, ny, nz = case["res"]
    return np.ascontiguousarray(np.random.default_rng(1000 + seed).standard_normal((nz, ny, nx, 2)), np.float32)


def with_volume(case, volume=None, seed=0):
    c = dict(case)
    c["volume"] = random_volume(case, seed) if volume is None else np.ascontiguousarray(volume, np.float32)
    return c


def tiny_case(kind, volume=None, seed=0, **kw):
    """phasor_backproject_cases.tiny_case with a complex volume beside its phasors"""
    return with_volume(pc.tiny_case(kind, seed=seed, **kw), volume, seed)


def make_case(kind, sp, lp, volume=None, seed=0, **kw):
    return with_volume(pc.make_case(kind, sp, lp, seed=seed, **kw), volume, seed)


def parity_case(kind, offsets, F, weights, form="uniform"):
    """the geometry, table and weights of phasor_backproject_cases.parity_case (its phasors are kept for the adjoint identity),
    with a random complex volume"""
    return with_volume(pc.parity_case(kind, offsets, F, weights, form), seed=F)


def with_form(case, form):
    return pc.with_form(case, form)


def one_hot_volume(case, voxel):
    """1 + 0i in voxel (ix, iy, iz), 0 elsewhere"""
    nx, ny, nz = case["res"]
    v = np.zeros((nz, ny, nx, 2), np.float32)
    v[voxel[2], voxel[1], voxel[0], 0] = 1.0
    return v


def one_hot_phasors(case, p, k):
    ph = np.zeros((rows_of(case), case["F"], 2), np.float32)
    ph[p, k, 0] = 1.0
    return ph


def volume_complex(case, dtype=np.float64):
    v = case["volume"]
    return (v[..., 0].astype(dtype) + 1j * v[..., 1].astype(dtype)).reshape(-1)


# ---------------------------------------------------------------- references
def reference(case):
    """the sum restated in numpy f64, independent of the header: complex (rows, F)"""
    t = pc.taus(case, np.float64)                               # (voxels, rows)
    gate = pc.in_window(case, np.float64)
    t = np.where(gate, t, 0.0)
    with np.errstate(invalid="ignore"):
        u = np.where(gate, volume_complex(case)[:, None], 0.0)  # (a NaN voxel stays out of the rows it does not reach)
    out = np.empty((t.shape[1], case["F"]), np.complex128)
    for k, f in enumerate(case["freq"].astype(np.float64)):
        out[:, k] = (u * np.exp(-2j * np.pi * f * t)).sum(axis=0)
    if case["weights"] is not None:
        out *= case["weights"].astype(np.float64)[None, :]
    return out


def dense_operator(case):
    """A^H of a case as a dense f64 matrix (rows * F, voxels): Q = (A^H u) reshaped (rows, F); phasor_backproject is its
    conjugate transpose"""
    t = pc.taus(case, np.float64)
    gate = pc.in_window(case, np.float64)
    f = case["freq"].astype(np.float64)
    w = np.ones(len(f)) if case["weights"] is None else case["weights"].astype(np.float64)
    m = np.where(gate.T[:, None, :], w[None, :, None] * np.exp(-2j * np.pi * f[None, :, None] * np.where(gate, t, 0.0).T[:, None, :]), 0.0)
    return m.reshape(t.shape[1] * len(f), t.shape[0])


def reference_f32(case):
    """the sum restated in numpy f32 in the header's operation order — z as phasor_backproject_cases.reference_f32 forms it (table
    form, or anchors every ANCHOR frequencies with z <- z r in between), the voxels added in ascending order as a sequential f32
    sum of the f32 products ur zr, ui zi / ui zr, -(ur zi) (np.cumsum), where the header's fmaf skips the product's rounding.
    complex (rows, F)"""
    f32 = np.float32
    tau, gate = pc.taus(case, f32), pc.in_window(case, f32)     # (voxels, rows)
    t = np.where(gate, tau, f32(0))
    F, freq, step = case["F"], case["freq"], f32(case["freq_step"])
    if step == 0:
        c, s = pc.phasor_term_f32(freq[None, None, :], t[..., None])
        zr, zi = c, -s
    else:
        anchors = np.arange(0, F, ANCHOR)
        c, s = pc.phasor_term_f32(freq[anchors][None, None, :], t[..., None])
        cr, sr = pc.phasor_term_f32(step, t)
        rr, ri = cr[..., None], -sr[..., None]
        zr, zi = np.empty(t.shape + (F,), f32), np.empty(t.shape + (F,), f32)
        cur_r, cur_i = c, -s
        for j in range(ANCHOR):
            ok = anchors + j < F
            zr[..., (anchors + j)[ok]], zi[..., (anchors + j)[ok]] = cur_r[..., ok], cur_i[..., ok]
            cur_r, cur_i = pc._fma(cur_r, rr, -(cur_i * ri)), pc._fma(cur_r, ri, cur_i * rr)
    v = case["volume"].reshape(-1, 2)
    ur, ui = v[:, 0][:, None, None], v[:, 1][:, None, None]
    g = gate[..., None, None]
    re = np.where(g, np.stack([ur * zr, ui * zi], axis=-1), f32(0))          # (voxels, rows, F, 2)
    im = np.where(g, np.stack([ui * zr, -(ur * zi)], axis=-1), f32(0))
    n_vox, rows = t.shape

    def total(x):
        x = np.moveaxis(x, 0, 2).reshape(rows, F, n_vox * 2)                # per (row, k): voxels ascending, the two products of each
        return np.cumsum(x, axis=2, dtype=f32)[:, :, -1]
    qr, qi = total(re), total(im)
    if case["weights"] is not None:
        w = case["weights"][None, :]
        qr, qi = w * qr, w * qi
    return qr.astype(np.float64) + 1j * qi.astype(np.float64)


def rel_l2(a, b):
    return pc.rel_l2(a, b)


def as_complex(rows):
    r = np.asarray(rows)
    return r[..., 0].astype(np.float64) + 1j * r[..., 1].astype(np.float64)


def host_phasor_forward_project(case, expect=0, fill=None):
    """the host build's phasors, complex (rows, F) — or, refused, the untouched (rows, F, 2) f32 array"""
    out = np.full((max(rows_of(case), 1), max(case["F"], 1), 2), np.nan if fill is None else fill, np.float32)
    w = case["weights"]
    d = pc.desc_of(case, *(case[k].ctypes.data for k in ("sp", "lp", "so", "lo", "freq")), None if w is None else w.ctypes.data)
    rc = host_lib().hpf_forward_project(C.byref(d), C.c_void_p(case["volume"].ctypes.data), C.c_void_p(out.ctypes.data))
    assert rc == expect, rc
    return as_complex(out) if expect == 0 else out


def inner(a, b):
    """<a, b> = sum of conj(a) b, in f64"""
    return complex(np.vdot(np.asarray(a, np.complex128).reshape(-1), np.asarray(b, np.complex128).reshape(-1)))


def adjoint_gap(Ay, x, y, AHx):
    """(|<A y, x> - <y, A^H x>|, the bound ADJOINT_TOL (|Ay| |x| + |y| |A^H x|)), inner products in f64"""
    gap = abs(inner(Ay, x) - inner(y, AHx))
    n = np.linalg.norm
    bound = ADJOINT_TOL * (n(np.ravel(Ay)) * n(np.ravel(x)) + n(np.ravel(y)) * n(np.ravel(AHx)))
    return float(gap), float(bound)


# ---------------------------------------------------------------- the CGLS yardstick
# The Confocal tiny case with F = 28 (no weights, no window), x_true = 1 on [iz = 3, iy 2:4, ix 2:4], y = A^H x_true.  CGLS in
# numpy f64 on the dense operator (test_cgls_on_the_dense_operator): |r_k| / |y| = 4.6e-3 at k = 10 and 2.1e-6 at k = 20, the
# volume recovered to 2.9e-6 (rel-L2) at k = 20; the operator's condition number is 6.2.  The GPU test holds
# phasor_reconstruct_cgls to 2 x the k = 10 figure.
CGLS_R10 = 4.6e-3
CGLS_R20 = 2.1e-6
CGLS_X20 = 2.9e-6
CGLS_COND = 6.2


def cgls_case():
    case = pc.tiny_case(CONFOCAL, F=28)
    x = np.zeros((6, 6, 6), np.float64)
    x[3, 2:4, 2:4] = 1.0
    return case, x


def cgls_dense(M, y, iterations):
    """CGLS on min |M x - y| from x = 0 in f64: (x, residuals)"""
    r = y.copy()
    s = M.conj().T @ r
    x, p = np.zeros(M.shape[1], np.complex128), s.copy()
    gamma, norm_y = np.vdot(s, s).real, np.linalg.norm(y)
    residuals = [1.0]
    for _ in range(iterations):
        q = M @ p
        alpha = gamma / np.vdot(q, q).real
        x += alpha * p
        r -= alpha * q
        s = M.conj().T @ r
        gamma, last = np.vdot(s, s).real, gamma
        p = s + (gamma / last) * p
        residuals.append(float(np.linalg.norm(r) / norm_y))
    return x, residuals
