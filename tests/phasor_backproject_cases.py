"""Shared by tests/test_phasor_backproject.py (CPU) and tests/test_gpu_phasor_backproject.py: the host build of
mtr_phasor_backproject.h (tests/host_phasor_backproject.cpp), an independent numpy f64 restatement of the sum, a numpy f32
restatement in the header's operation order (table form and the 16-anchor recurrence), the frequency tables, the tiny geometry of
the parity cases (backproject_cases.py's) and the scenes of the end-to-end check (render a quad at z = 1 with a phasor film,
reconstruct, the depth profile of |V| peaks at z = 1)."""
import ctypes as C
import os
import subprocess

import numpy as np

import backproject_cases as bc
from backproject_cases import CONFOCAL, EXHAUSTIVE, SINGLE, wall_points  # noqa: F401  (re-exported)

ROOT = bc.ROOT
# rel-L2 over the complex volume, the bar of every parity test here.  The numpy f32 restatement against f64 on the tiny geometry
# (8 x 8 scan, 6^3 voxels, start_opl 1.85; every capture type, offsets off and on, point-source and random phasors, weights ones
# and gaussian) is at worst 7.6e-6 (F = 15), 1.04e-5 (F = 28), 2.4e-5 (F = 151): the f32 rounding of a phase of several hundred
# radians, with and without the 16-anchor recurrence.  4 x the worst figure, for the quarter-range polynomials and host / device
# differences in contraction.
PB_TOL = 1e-4
FLT_MAX = np.float32(3.4028234663852886e38)
ANCHOR = 16                                 # kPbAnchor
POINT = (0.2, -0.1, 1.0)                    # the point source of the "point" phasors

# the films of tests/test_nlos_phasor.py (F = 15 from f = 0; F = 151: 9 full anchor blocks and a ragged one of 7) and the film of the
# end-to-end test (F = 28)
FILMS = {15: dict(temporal_bins=256, bin_width_opl=0.01, wl_mean=2.56, wl_sigma=0.1),
         151: dict(temporal_bins=4096, bin_width_opl=0.003, wl_mean=0.1, wl_sigma=0.0824),
         28: dict(temporal_bins=256, bin_width_opl=0.02, wl_mean=0.2, wl_sigma=0.2)}
SLICES = (1, 16, 17)                        # the first F entries of the 151 table: the anchor block's edges


def film_table(temporal_bins, bin_width_opl, wl_mean, wl_sigma):
    """the frequencies a phasor_hdr_film of these properties selects, f32 (numpy's fftfreq inside the band of the wavelet)"""
    span = temporal_bins * bin_width_opl
    mean, sigma = span / wl_mean, span / (wl_sigma * 6)
    lo, hi = max(0, int(np.floor(mean - 3 * sigma))), min(temporal_bins // 2, int(np.ceil(mean + 3 * sigma)))
    return np.ascontiguousarray(np.fft.fftfreq(temporal_bins, d=bin_width_opl)[lo:hi + 1].astype(np.float32))


def table(F):
    """(frequencies f32, the film's properties) of one of the test tables"""
    film = FILMS[F if F in FILMS else 151]
    f = film_table(**film)
    if F not in FILMS:
        f = np.ascontiguousarray(f[:F])
    assert len(f) == F, (len(f), F)
    return f, film


def gaussian_weights(freq, film):
    """exp(-1/2 ((f - 1 / wl_mean) / sigma_f)^2), sigma_f = 1 / (6 wl_sigma): the band the film selected its frequencies from"""
    f = np.asarray(freq, np.float64)
    return np.exp(-0.5 * ((f - 1.0 / film["wl_mean"]) * (6.0 * film["wl_sigma"])) ** 2).astype(np.float32)


def build_host_phasor_backproject():
    """tests/host_phasor_backproject.cpp with the flags of build_host_backproject() (backproject_cases.py)"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_phasor_backproject.so")
    src = os.path.join(ROOT, "tests", "host_phasor_backproject.cpp")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "mitransient_amd.h")] + [os.path.join(csrc, h) for h in (
        "mtr_phasor_backproject.h", "mtr_backproject.h", "mtr_core.h", "mtr_flat_prims.h", "mtr_shadow_hull.h")]
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
        _host = C.CDLL(build_host_phasor_backproject())
        _host.hb_check.restype = C.c_char_p
        _host.hpb_phasor_term.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
    return _host


def host_phasor_term(freq, tau):
    """(cos, sin) of phasor_term(freq, tau), the film's own f32 arithmetic"""
    cs = (C.c_float * 2)()
    host_lib().hpb_phasor_term(float(np.float32(freq)), float(np.float32(tau)), cs)
    return np.float32(cs[0]), np.float32(cs[1])


# ---------------------------------------------------------------- cases
def uniform_step(freq):
    """the product's classification of a table (nlos.uniform_frequency_step): the step, or 0.0 for the table form"""
    from mitransient_amd.nlos import uniform_frequency_step
    return uniform_frequency_step(freq)


def path_lengths(case, point):
    """d of every pair for a scatterer at `point`, f64 (the geometry's f32 values, offsets included)"""
    si, li = bc.pairs(case)
    x = np.asarray(point, np.float64)
    sp, lp = case["sp"].astype(np.float64)[si], case["lp"].astype(np.float64)[li]
    return (np.linalg.norm(sp - x, axis=-1) + np.linalg.norm(x - lp, axis=-1) + case["so"].astype(np.float64)[si]
            + case["lo"].astype(np.float64)[li])


def make_case(capture_type, sensor_points, laser_points, F=28, start=1.85, vmin=(-1, -1, 0.5), vmax=(1, 1, 1.5), res=(6, 6, 6),
              offsets=False, phasors="random", weights=None, form="uniform", window=None, freq=None, seed=0):
    """one call's inputs, f32 as the C-ABI takes them.  `phasors`: "random", "point" (a unit scatterer at POINT) or the
    (rows, F, 2) array itself; `weights`: None, "gaussian" or an (F,) array; `form`: "uniform" (the product's rule decides: a
    table it does not find uniform stays in the table form) or "table"; `window`: None or (tau_min, tau_max)"""
    case = bc.make_case(capture_type, sensor_points, laser_points, T=1, start=start, bin_width=1.0, vmin=vmin, vmax=vmax, res=res,
                        offsets=offsets)               # (the geometry; its one-bin transient capture is dropped)
    del case["capture"], case["T"], case["linear"]
    if freq is None:
        freq, film = table(F)
    else:
        freq, film = np.ascontiguousarray(freq, np.float32), None
    F = len(freq)
    rows = case["S"] * case["L"] if capture_type == EXHAUSTIVE else case["S"]
    if isinstance(phasors, str):
        if phasors == "point":
            rel = path_lengths(case, POINT) - float(case["start"])
            ph = np.exp(-2j * np.pi * freq.astype(np.float64)[None, :] * rel[:, None])
        else:
            rng = np.random.default_rng(seed)
            ph = rng.standard_normal((rows, F)) + 1j * rng.standard_normal((rows, F))
        ph = np.stack([ph.real, ph.imag], axis=-1)
    else:
        ph = np.asarray(phasors).reshape(rows, F, 2)
    if isinstance(weights, str):
        assert weights == "gaussian" and film is not None
        weights = gaussian_weights(freq, film)
    lo, hi = (-FLT_MAX, FLT_MAX) if window is None else window
    case.update(F=F, freq=freq, film=film, phasors=np.ascontiguousarray(ph, np.float32),
                weights=None if weights is None else np.ascontiguousarray(weights, np.float32),
                freq_step=np.float32(uniform_step(freq) if form == "uniform" else 0.0),
                tau_min=np.float32(lo), tau_max=np.float32(hi))
    return case


def tiny_case(kind, **kw):
    """the tiny geometry of backproject_cases.tiny_case: 8 x 8 scan points, 6^3 voxels in [-1, 1]^2 x [0.5, 1.5], start_opl 1.85"""
    g = bc.tiny_case(kind)
    return make_case(kind, g["sp"], g["lp"], **kw)


def with_form(case, form):
    c = dict(case)
    c["freq_step"] = np.float32(uniform_step(case["freq"]) if form == "uniform" else 0.0)
    return c


# every capture type x offsets x table x weights; the phasors alternate between the two kinds
PARITY = [(k, o, F, w) for k in (CONFOCAL, SINGLE, EXHAUSTIVE) for o in (False, True) for F in (15, 28, 151) for w in (None, "gaussian")]


def parity_case(kind, offsets, F, weights, form="uniform"):
    phasors = "point" if (offsets ^ (weights is None)) else "random"
    return tiny_case(kind, offsets=offsets, F=F, weights=weights, phasors=phasors, form=form, seed=F)


def taus(case, dtype):
    """tau = d - start_opl of every (voxel, pair), in `dtype` with the operation order of mtr_backproject.h"""
    c = dict(case)
    c["bin_width"] = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        return bc.positions(c, dtype)


def in_window(case, dtype):
    t = taus(case, dtype)
    with np.errstate(invalid="ignore"):
        return (t >= dtype(case["tau_min"])) & (t <= dtype(case["tau_max"]))


def weighted_rows(case, dtype):
    """(a, b) = w_k P[p, k], (rows, F) each"""
    a, b = case["phasors"][..., 0].astype(dtype), case["phasors"][..., 1].astype(dtype)
    if case["weights"] is not None:
        w = case["weights"].astype(dtype)[None, :]
        a, b = w * a, w * b
    return a, b


def as_complex(volume):
    v = np.asarray(volume)
    return v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)


def reference(case):
    """the sum restated in numpy f64, independent of the header: complex (nz, ny, nx)"""
    t = taus(case, np.float64)
    gate = in_window(case, np.float64)
    t = np.where(gate, t, 0.0)
    a, b = weighted_rows(case, np.float64)
    wp = a + 1j * b
    acc = np.zeros(t.shape[0], np.complex128)
    for k, f in enumerate(case["freq"].astype(np.float64)):
        acc += np.where(gate, wp[None, :, k] * np.exp(2j * np.pi * f * t), 0.0).sum(axis=1)
    nx, ny, nz = case["res"]
    return acc.reshape(nz, ny, nx)


def _fma(a, b, c):
    """fmaf on f32 arrays: the product is exact in f64; the sum is rounded to f64 and then to f32 (a double rounding that differs
    from one fma in rare last bits — the restatement is held to PB_TOL, not to equal bits)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def phasor_term_f32(freq, tau):
    """phasor_term (mtr_core.h) on f32 arrays: (cos, sin) of fmod(-2 pi f tau, 2 pi)"""
    f32 = np.float32
    freq, tau = np.asarray(freq, f32), np.asarray(tau, f32)
    y = f32(6.283185307179586)
    x = (f32(-6.283185307179586) * freq) * tau
    phase = x - y * np.floor(x / y)
    k = np.floor(_fma(phase, f32(0.6366197723675814), f32(0.5)))
    r = _fma(-k, f32(1.5707962512969971), phase)
    r = _fma(-k, f32(7.549789415861596e-08), r)
    z = r * r
    ps = _fma(_fma(f32(-1.9515295891e-4), z, f32(8.3321608736e-3)), z, f32(-1.6666654611e-1))
    s = _fma(r * z, ps, r)
    pc = _fma(_fma(f32(2.443315711809948e-5), z, f32(-1.388731625493765e-3)), z, f32(4.166664568298827e-2))
    c = _fma(z * z, pc, _fma(f32(-0.5), z, f32(1.0)))
    q = k.astype(np.int64) & 3
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def reference_f32(case, chunk=24):
    """the sum restated in numpy f32 in the header's operation order — table form (freq_step 0) or anchors every ANCHOR
    frequencies with z <- z r in between; the accumulator is a sequential f32 sum of the f32 products a zr, -(b zi) / a zi, b zr
    in the header's order (np.cumsum), where the header's fmaf skips the product's rounding.  (nz, ny, nx) complex"""
    f32 = np.float32
    tau_all, gate_all = taus(case, f32), in_window(case, f32)
    F, freq, step = case["F"], case["freq"], f32(case["freq_step"])
    a, b = weighted_rows(case, f32)
    out = np.zeros(tau_all.shape[0], np.complex128)
    for v0 in range(0, tau_all.shape[0], chunk):
        gate = gate_all[v0:v0 + chunk]
        t = np.where(gate, tau_all[v0:v0 + chunk], f32(0))
        if step == 0:
            c, s = phasor_term_f32(freq[None, None, :], t[..., None])
            zr, zi = c, -s
        else:
            anchors = np.arange(0, F, ANCHOR)
            c, s = phasor_term_f32(freq[anchors][None, None, :], t[..., None])
            cr, sr = phasor_term_f32(step, t)
            rr, ri = cr[..., None], -sr[..., None]
            zr, zi = np.empty(t.shape + (F,), f32), np.empty(t.shape + (F,), f32)
            cur_r, cur_i = c, -s
            for j in range(ANCHOR):
                ok = anchors + j < F
                zr[..., (anchors + j)[ok]], zi[..., (anchors + j)[ok]] = cur_r[..., ok], cur_i[..., ok]
                cur_r, cur_i = _fma(cur_r, rr, -(cur_i * ri)), _fma(cur_r, ri, cur_i * rr)
        g = gate[..., None, None]
        re = np.where(g, np.stack([a[None] * zr, -(b[None] * zi)], axis=-1), f32(0)).reshape(t.shape[0], -1)
        im = np.where(g, np.stack([a[None] * zi, b[None] * zr], axis=-1), f32(0)).reshape(t.shape[0], -1)
        out[v0:v0 + chunk] = np.cumsum(re, axis=1, dtype=f32)[:, -1].astype(np.float64) \
            + 1j * np.cumsum(im, axis=1, dtype=f32)[:, -1].astype(np.float64)
    nx, ny, nz = case["res"]
    return out.reshape(nz, ny, nx)


def rel_l2(a, b):
    """rel-L2 over complex volumes"""
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def desc_of(case, sp, lp, so, lo, freq, weights):
    """mtr_phasor_backproject_desc of a case; sp .. weights: the addresses of the six arrays (host or device; weights may be None)"""
    from mitransient_amd import _cabi
    d = _cabi.mtr_phasor_backproject_desc()
    d.capture_type, d.n_sensor, d.n_laser, d.n_freq = case["capture_type"], case["S"], case["L"], case["F"]
    d.start_opl, d.freq_step, d.tau_min, d.tau_max = case["start"], case["freq_step"], case["tau_min"], case["tau_max"]
    for k in range(3):
        d.volume_min[k], d.volume_max[k] = case["vmin"][k], case["vmax"][k]
    d.nx, d.ny, d.nz = case["res"]
    d.sensor_points, d.laser_points, d.sensor_offset, d.laser_offset, d.frequencies, d.weights = sp, lp, so, lo, freq, weights
    return d


def host_phasor_backproject(case, expect=0, fill=None):
    """the host build's volume, complex (nz, ny, nx) — or, refused, the untouched (nz, ny, nx, 2) f32 array"""
    nx, ny, nz = case["res"]
    vol = np.full((nz, ny, nx, 2), np.nan if fill is None else fill, np.float32)
    w = case["weights"]
    d = desc_of(case, *(case[k].ctypes.data for k in ("sp", "lp", "so", "lo", "freq")), None if w is None else w.ctypes.data)
    rc = host_lib().hpb_backproject(C.byref(d), C.c_void_p(case["phasors"].ctypes.data), C.c_void_p(vol.ctypes.data))
    assert rc == expect, rc
    return as_complex(vol) if expect == 0 else vol


def brightest(volume):
    """(ix, iy, iz) of the largest |V|"""
    v = np.abs(volume)
    iz, iy, ix = np.unravel_index(int(np.argmax(v)), v.shape)
    return int(ix), int(iy), int(iz)


# ---------------------------------------------------------------- end to end
E2E = bc.E2E
E2E_BOX = bc.E2E_BOX
E2E_SPP = bc.E2E_SPP
E2E_FILM = dict(FILMS[28], type="phasor_hdr_film")


def e2e_scene(name):
    """backproject_cases.e2e_scene with the F = 28 phasor film; the caller renders in a ``*_ad_mono`` variant"""
    from conftest import make_nlos
    kw = dict(sx=16, sy=16, start=1.2, max_depth=3, spp=E2E_SPP, film=dict(E2E_FILM))
    kw.update(E2E[name])
    scene = make_nlos(**kw)
    assert len(scene.sensors()[0].film().frequencies) == 28
    return scene


def depth_peak(volume):
    """backproject_cases.depth_peak of |V|"""
    return bc.depth_peak(np.abs(np.asarray(volume)))
