"""ctypes wrapper of the CPU oracle (TEST INFRASTRUCTURE — never imported by mitransient_amd/).

Only tests/, ``__graft_entry__.smoke()`` and bench.py's ``cpu_baseline`` leg load this.
PARITY UNPINNED against real Mitsuba (see mtr_oracle.c header).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from mitransient_amd import _cabi   # POD struct definitions of the boundary only

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "libmtr_oracle.so")
_lib = None


class orc_splat_rec(C.Structure):
    _fields_ = [("lane", C.c_uint32), ("depth_kind", C.c_uint32), ("pixel", C.c_uint32), ("bin", C.c_uint32),
                ("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("opl", C.c_float)]


def build(force=False):
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(os.path.join(_HERE, "mtr_oracle.c")):
        subprocess.check_call(["make", "-C", _HERE, "-s"] + (["-B"] if force else []))
    return LIB


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            build()
        L = C.CDLL(LIB)
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        L.orc_render.argtypes = [C.POINTER(_cabi.mtr_scene_desc), C.POINTER(_cabi.mtr_render_params), fp, fp,
                                 C.POINTER(_cabi.mtr_counters), C.c_int, C.c_int,
                                 C.POINTER(orc_splat_rec), C.c_uint64, C.POINTER(C.c_uint64)]
        L.orc_render.restype = C.c_int
        L.orc_render_ex.argtypes = L.orc_render.argtypes + [C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
        L.orc_render_ex.restype = C.c_int
        L.orc_angular_falloff.argtypes = [C.POINTER(_cabi.mtr_emitter), C.c_uint32, fp, C.POINTER(C.c_double)]
        L.orc_angular_falloff.restype = None
        L.orc_render_polarized.argtypes = [C.POINTER(_cabi.mtr_scene_desc), C.POINTER(_cabi.mtr_render_params), fp, fp,
                                           C.POINTER(_cabi.mtr_counters), C.c_int, C.c_int, C.POINTER(C.c_uint8)]
        L.orc_render_polarized.restype = C.c_int
        dp = C.POINTER(C.c_double)
        L.orc_polar_reflection.argtypes = [C.c_double, C.c_double, C.c_double, dp]
        L.orc_polar_transmission.argtypes = [C.c_double, C.c_double, dp]
        L.orc_polar_rotate_basis.argtypes = [dp, dp, dp, dp]
        L.orc_polar_stokes_basis.argtypes = [dp, dp]
        L.orc_polar_to_world_mueller.argtypes = [dp, dp, dp, dp, dp]
        for n in ("reflection", "transmission", "rotate_basis", "stokes_basis", "to_world_mueller"):
            getattr(L, "orc_polar_" + n).restype = None
        L.orc_develop.argtypes = [C.POINTER(_cabi.mtr_film_desc), fp, fp, fp, fp]
        L.orc_develop.restype = None
        L.orc_splat_add.argtypes = [C.POINTER(_cabi.mtr_film_desc), C.c_uint64, u32p, fp, fp, fp, fp, fp, u32p, u32p]
        L.orc_splat_add.restype = None
        L.orc_bin_index.argtypes = [C.c_float, C.c_float, C.c_float, C.c_uint32]
        L.orc_bin_index.restype = C.c_int
        L.orc_intersect.argtypes = [C.POINTER(_cabi.mtr_scene_desc), C.c_uint32, fp, fp, fp, C.c_int, fp,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]
        L.orc_intersect.restype = None
        L.orc_camera_ray.argtypes = [C.POINTER(_cabi.mtr_scene_desc), C.c_uint32, C.c_uint32, C.c_float, C.c_float, fp, fp, fp]
        L.orc_camera_ray.restype = None
        L.orc_pcg32_stream.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, u32p, fp]
        L.orc_pcg32_stream.restype = None
        L.orc_sampler_stream.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, fp]
        L.orc_sampler_stream.restype = None
        L.orc_tea32.argtypes = [C.c_uint32, C.c_uint32, C.c_int, u32p]
        L.orc_tea32.restype = None
        L.orc_sincos_q.argtypes = [C.c_float, fp, fp]
        L.orc_sincos_q.restype = None
        L.orc_square_to_cos_hemi.argtypes = [C.c_float, C.c_float, fp]
        L.orc_square_to_cos_hemi.restype = None
        L.orc_num_threads.restype = C.c_int
        L.orc_phasor_term.argtypes = [C.c_float, C.c_float, fp, fp]
        L.orc_phasor_term.restype = None
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def film_shape(f):
    """raw tensor shape: (H,W,T,4), or (H,W,Lh,Lw,T,4) for an exhaustive_scan film (transient_image_block.py:63-68)"""
    if f.n_frequencies:                         # phasor_hdr_film: (H, W, 2F+1)
        return (f.height, f.width, 2 * f.n_frequencies + 1)
    if f.laser_scan_width and f.laser_scan_height:
        return (f.height, f.width, f.laser_scan_height, f.laser_scan_width, f.temporal_bins, 4)
    return (f.height, f.width, f.temporal_bins, 4)


def alloc_film(film_desc, prefault=False):
    f = film_desc
    t4 = np.zeros(film_shape(f), np.float32)
    s4 = np.zeros((f.height, f.width, 4), np.float32)
    if prefault:          # touch every page now (np.zeros maps lazily): keeps page faults out of timed regions
        t4.fill(0.0)
        s4.fill(0.0)
    return t4, s4


def render(scene_data, params: _cabi.mtr_render_params, n_threads=0, use_bvh=False, log_capacity=0, out=None, near=False):
    """Returns (transient (H,W,T,4) f32, steady (H,W,4) f32, counters dict[, log ndarray][, near]).
    ``out=(t4, s4)`` accumulates into existing buffers.  ``near=True`` appends the angulararea near-threshold report
    ``(map (H,W) bool, total)``: the pixels, and the number of falloff evaluations, where the cosine sat within 4 ulps of
    cos_cutoff / cos_beam or cutoff - acos(cos) within 4 ulps of 0 — an f32 falloff may take the other side of `> 0` there."""
    f = scene_data.film
    t4, s4 = out if out is not None else alloc_film(f)
    cnt = _cabi.mtr_counters()
    d = scene_data.desc()
    log = None
    n_log = C.c_uint64(0)
    if log_capacity:
        log = (orc_splat_rec * log_capacity)()
    args = (C.byref(d), C.byref(params), _fp(t4), _fp(s4), C.byref(cnt), n_threads, int(use_bvh), log, log_capacity,
            C.byref(n_log))
    if near:
        near_map = np.zeros((f.height, f.width), np.uint8)
        near_total = C.c_uint64(0)
        rc = lib().orc_render_ex(*args, near_map.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(near_total))
    else:
        rc = lib().orc_render(*args)
    if rc != 0:
        raise RuntimeError(f"orc_render failed ({rc})")
    res = (t4, s4, cnt.as_dict())
    if log_capacity:
        n = min(int(n_log.value), log_capacity)
        arr = np.frombuffer(log, dtype=np.dtype([("lane", "u4"), ("depth_kind", "u4"), ("pixel", "u4"), ("bin", "u4"),
                                                  ("r", "f4"), ("g", "f4"), ("b", "f4"), ("opl", "f4")]))[:n].copy()
        res += (arr,)
    if near:
        res += ((near_map.astype(bool), int(near_total.value)),)
    return res


def render_polarized(scene_data, params: _cabi.mtr_render_params, n_threads=0, use_bvh=False, out=None):
    """The polarized render (f64 Mueller algebra over the f32 path): (transient (H,W,T,4) = S0..S3, steady (H,W,4) = (S0, S1,
    S2, weight), counters dict, rr_near (H,W) bool — the pixels where a Russian-roulette draw lay within 1e-5 of rr_prob, whose
    f32 decision may differ).  ``out=(t4, s4)`` accumulates into existing buffers."""
    f = scene_data.film
    t4, s4 = out if out is not None else alloc_film(f)
    cnt = _cabi.mtr_counters()
    near = np.zeros((f.height, f.width), np.uint8)
    d = scene_data.desc()
    rc = lib().orc_render_polarized(C.byref(d), C.byref(params), _fp(t4), _fp(s4), C.byref(cnt), n_threads, int(use_bvh),
                                    near.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise RuntimeError(f"orc_render_polarized failed ({rc})")
    return t4, s4, cnt.as_dict(), near.astype(bool)


def _d(a, n):
    a = np.ascontiguousarray(a, np.float64).reshape(n)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _out(n):
    a = np.zeros(n, np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def polar_reflection(cos_i, eta):
    """f64 Mueller matrix of specular reflection; eta complex (conductor) or real (dielectric, cos_i < 0 inside)"""
    eta = complex(eta)
    o, op = _out(16)
    lib().orc_polar_reflection(float(cos_i), eta.real, eta.imag, op)
    return o.reshape(4, 4)


def polar_transmission(cos_i, eta):
    o, op = _out(16)
    lib().orc_polar_transmission(float(cos_i), float(eta), op)
    return o.reshape(4, 4)


def polar_rotate_basis(fwd, cur, tgt):
    (f, fp_), (c, cp), (t, tp) = _d(fwd, 3), _d(cur, 3), _d(tgt, 3)
    o, op = _out(16)
    lib().orc_polar_rotate_basis(fp_, cp, tp, op)
    return o.reshape(4, 4)


def polar_stokes_basis(w):
    a, ap = _d(w, 3)
    o, op = _out(3)
    lib().orc_polar_stokes_basis(ap, op)
    return o


def polar_to_world_mueller(M, frame_stn, wi, wo):
    (m, mp), (f, fp_), (a, ap), (b, bp) = _d(M, 16), _d(frame_stn, 9), _d(wi, 3), _d(wo, 3)
    o, op = _out(16)
    lib().orc_polar_to_world_mueller(mp, fp_, ap, bp, op)
    return o.reshape(4, 4)


def angular_falloff(emitter, cos_theta):
    """angulararea.py:74-82 _fallof_curve in f64 for an `mtr_emitter`: the selects on the f32 cosines, the transition
    (cutoff - acos(c)) * inv_transition with f64 acos"""
    c = np.ascontiguousarray(cos_theta, np.float32).ravel()
    o = np.zeros(c.size, np.float64)
    lib().orc_angular_falloff(C.byref(emitter), c.size, _fp(c), o.ctypes.data_as(C.POINTER(C.c_double)))
    return o


def develop(film_desc, t4=None, s4=None):
    t3 = s3 = None
    if t4 is not None and film_desc.n_frequencies:
        t3 = np.empty(t4.shape[:-1] + (film_desc.n_frequencies, 2), np.float32)
    elif t4 is not None:
        t3 = np.empty(t4.shape[:-1] + (3,), np.float32)
    if s4 is not None:
        s3 = np.empty(s4.shape[:-1] + (3,), np.float32)
    lib().orc_develop(C.byref(film_desc), _fp(t4) if t4 is not None else None, _fp(t3) if t3 is not None else None,
                      _fp(s4) if s4 is not None else None, _fp(s3) if s3 is not None else None)
    # the reference's steady hdrfilm carries the crop window (transient_hdr_film.py:131-144): steady.develop() is
    # (crop_h, crop_w, 3); the accumulator is full-size with the window at its top-left corner
    if s3 is not None and (film_desc.crop_width, film_desc.crop_height) != (film_desc.width, film_desc.height) \
            and s3.shape[:2] == (film_desc.height, film_desc.width):
        s3 = np.ascontiguousarray(s3[:film_desc.crop_height, :film_desc.crop_width])
    return t3, s3


def splat_add(film_desc, pixel, opl, r, g, b, t4, laser_x=None, laser_y=None):
    pixel = np.ascontiguousarray(pixel, np.uint32)
    arrs = [np.ascontiguousarray(x, np.float32) for x in (opl, r, g, b)]
    up = C.POINTER(C.c_uint32)
    lx = np.ascontiguousarray(laser_x, np.uint32) if laser_x is not None else None
    ly = np.ascontiguousarray(laser_y, np.uint32) if laser_y is not None else None
    lib().orc_splat_add(C.byref(film_desc), len(pixel), pixel.ctypes.data_as(up), *[_fp(a) for a in arrs], _fp(t4),
                        lx.ctypes.data_as(up) if lx is not None else None, ly.ctypes.data_as(up) if ly is not None else None)


def phasor_term(freq, opl):
    c, s = C.c_float(0), C.c_float(0)
    lib().orc_phasor_term(np.float32(freq), np.float32(opl), C.byref(c), C.byref(s))
    return c.value, s.value


def bin_index(distance, start, width, T):
    return lib().orc_bin_index(np.float32(distance), np.float32(start), np.float32(width), T)


def intersect(scene_data, o, d, maxt=None, use_bvh=False):
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    t = np.empty(n, np.float32)
    prim = np.empty(n, np.int32)
    occ = np.empty(n, np.uint8)
    mt = np.ascontiguousarray(maxt, np.float32) if maxt is not None else None
    desc = scene_data.desc()
    lib().orc_intersect(C.byref(desc), n, _fp(o), _fp(d), _fp(mt) if mt is not None else None, int(use_bvh),
                        _fp(t), prim.ctypes.data_as(C.POINTER(C.c_int32)), occ.ctypes.data_as(C.POINTER(C.c_uint8)))
    return t, prim, occ


def camera_ray(scene_data, px, py, j1, j2):
    o = np.empty(3, np.float32)
    d = np.empty(3, np.float32)
    mt = C.c_float()
    desc = scene_data.desc()
    lib().orc_camera_ray(C.byref(desc), px, py, j1, j2, _fp(o), _fp(d), C.byref(mt))
    return o, d, mt.value


def pcg32_stream(initstate, initseq, n):
    u = np.empty(n, np.uint32)
    f = np.empty(n, np.float32)
    lib().orc_pcg32_stream(initstate, initseq, n, u.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(f))
    return u, f


def sampler_stream(seed_value, lane, n):
    f = np.empty(n, np.float32)
    lib().orc_sampler_stream(seed_value, lane, n, _fp(f))
    return f


def tea32(v0, v1, rounds=4):
    out = np.empty(2, np.uint32)
    lib().orc_tea32(v0, v1, rounds, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return int(out[0]), int(out[1])


def num_threads():
    return lib().orc_num_threads()
