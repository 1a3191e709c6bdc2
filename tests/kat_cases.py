"""The known-answer cases of mtr_core.h (tests/test_kat_cases.py on the CPU, tests/test_gpu_kat.py on the device): per family of
MTR_HD functions, seeded inputs that reach the edges of each function, the one calling convention that drives the host twin
(tests/host_harness.cpp hh_<entry>), the oracle (orc_<entry>, where it exports the function) and the device harness
(mtr_test_dev_<entry><suffix>, mitransient_amd/csrc/mtr_kat.hip), and the bit-for-bit comparison.  Pure numpy; no GPU needed.

A case's edge inputs come FIRST, so that the runs at n = 1 and n = 63 evaluate edges too; N is no multiple of 64 or 256."""
import ctypes as C
import functools

import numpy as np

N = 200_003            # elements of a case (the bsdf family: N_BSDF per material and entry)
N_BSDF = 20_011
SMALL_N = (1, 63)
SUFFIXES = ("", "_k")  # the library's two flag sets (Makefile: OTHERS, KFLAGS)
F32 = np.float32
ONE_M = F32(1.0 - 2.0 ** -24)
FLT_MIN, FLT_MAX = F32(1.17549435e-38), F32(3.40282347e38)
DEN_MIN, DEN_MAX = np.uint32(1).view(F32), np.uint32(0x007fffff).view(F32)
INF, NAN = F32(np.inf), F32(np.nan)
FAMILIES = ("special", "trig", "warps", "fresnel", "bsdf", "rng", "film", "pairs")


def around(x, k=1):
    """x and its k f32 neighbours on either side"""
    x = F32(x)
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return out


def _fill(edges, rand, n=N):
    """edges first, then the random values, cut or cycled to n elements"""
    e = np.asarray(edges, np.float32).reshape(-1)
    r = np.asarray(rand, np.float32).reshape(-1)
    reps = -(-(n - len(e)) // len(r))
    return np.ascontiguousarray(np.concatenate([e, np.tile(r, reps)])[:n], np.float32)


def _planes(*cols):
    """SoA input: plane k = column k (f32 or u32), as words"""
    assert all(np.asarray(c).dtype in (np.float32, np.uint32) for c in cols)
    return np.ascontiguousarray(np.stack([np.ascontiguousarray(c).view(np.uint32) for c in cols]))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _handle(path):
    return C.CDLL(path)


def private_handle(lib):
    """the same shared library through a ctypes handle of this module's own: the argtypes other tests set on the session's handle
    (or this module's restype) stay apart"""
    return _handle(lib._name)


class Case:
    """entry: the function's name without prefix; pre: ctypes values handed over before n; ins: [(words, layout)], layout "soa"
    (planes, elements last) or "aos" (elements first); outs: [(components, layout)]; branches: {name: (mask over the elements,
    least count)}, derived from the inputs alone; oracle: the oracle exports the function; info: the inputs by name, for references"""

    def __init__(self, family, name, entry, pre, ins, outs, n_type=C.c_uint64, branches=None, oracle=False, info=None):
        self.family, self.name, self.entry, self.pre, self.ins, self.outs = family, name, entry, tuple(pre), ins, outs
        self.n_type, self.branches, self.oracle, self.info = n_type, branches or {}, oracle, info or {}
        self.n = ins[0][0].shape[-1] if ins[0][1] == "soa" else ins[0][0].shape[0]

    def inputs(self, n):
        return [np.ascontiguousarray(a[..., :n] if lay == "soa" else a[:n]).view(np.uint32) for a, lay in self.ins]

    def out_shapes(self, n):
        return [((k, n) if lay == "soa" else ((n, k) if k > 1 else (n,))) for k, lay in self.outs]

    def element_axis(self, j):
        return -1 if self.outs[j][1] == "soa" else 0

    def invoke(self, fn, n, in_ptrs, out_ptrs):
        args = [C.byref(p) if isinstance(p, C.Structure) else p for p in self.pre] + [self.n_type(n)]
        return fn(*args, *[C.c_void_p(p) for p in in_ptrs], *[C.c_void_p(p) for p in out_ptrs])

    def run_cpu(self, lib, prefix, n=None):
        """the host twin (prefix "hh_") or the oracle ("orc_"): the outputs as uint32 arrays"""
        n = self.n if n is None else n
        ins = self.inputs(n)
        outs = [np.zeros(s, np.uint32) for s in self.out_shapes(n)]
        fn = getattr(private_handle(lib), prefix + self.entry)
        fn.restype = None
        self.invoke(fn, n, [a.ctypes.data for a in ins], [o.ctypes.data for o in outs])
        return outs


def mismatches(case, a, b, n):
    """element mask: some output word of element i differs between the output lists a and b (NaNs of any payload are equal)"""
    bad = np.zeros(n, bool)
    for j, (x, y) in enumerate(zip(a, b)):
        ne = x != y
        ne &= ~(np.isnan(x.view(np.float32)) & np.isnan(y.view(np.float32)))
        if ne.ndim > 1:
            ne = ne.any(axis=0 if case.element_axis(j) == -1 else 1)
        bad |= ne
    return bad


def report(case, what, a, b, n, names=("host", "device")):
    """None when the two output lists agree on every word, else the message of the failing assertion: family, case, flag set, the
    first ten differing inputs and both bit patterns"""
    bad = mismatches(case, a, b, n)
    if not bad.any():
        return None
    ins = case.inputs(n)
    lines = [f"{case.family} / {case.name} [{what}] n = {n}: {int(bad.sum())} of {n} elements differ; the first ten:"]
    for i in np.flatnonzero(bad)[:10]:
        pick = lambda arr, lay: arr[..., i].reshape(-1) if lay == "soa" else np.atleast_1d(arr[i]).reshape(-1)     # noqa: E731
        x = np.concatenate([pick(arr, lay) for arr, (_, lay) in zip(ins, case.ins)])
        u = np.concatenate([pick(arr, lay) for arr, (_, lay) in zip(a, case.outs)])
        v = np.concatenate([pick(arr, lay) for arr, (_, lay) in zip(b, case.outs)])
        fmt = lambda w: " ".join(f"{int(t):08x}" for t in w)                                                       # noqa: E731
        lines.append(f"  [{i}] in {fmt(x)} ({' '.join(repr(float(t)) for t in x.view(np.float32))})\n"
                     f"        {names[0]} {fmt(u)}\n        {names[1]} {fmt(v)}")
    return "\n".join(lines)


def safe_rcp_distance(host, dev):
    """safe_rcp is the one function whose device form is NOT the host's by design (mtr_core.h: v_rcp_f32, 1 ulp, for culling alone).
    The distance of the device's words from the host's: {"max_ulp": over the results the host has as normal floats, "flushed": host
    results below FLT_MIN that the device returns as a zero of the same sign, "other": every remaining difference}"""
    h, d = host.reshape(-1), dev.reshape(-1)
    hf, df = h.view(np.float32), d.view(np.float32)
    same = (h == d) | (np.isnan(hf) & np.isnan(df))
    small = np.abs(hf) < FLT_MIN
    flushed = ~same & small & (df == 0) & (np.signbit(df) == np.signbit(hf))
    normal = ~same & ~small & np.isfinite(hf) & np.isfinite(df) & (np.signbit(df) == np.signbit(hf))
    ulp = np.abs(h[normal].astype(np.int64) - d[normal].astype(np.int64))
    return {"max_ulp": int(ulp.max()) if ulp.size else 0, "differ": int((~same).sum()), "flushed": int(flushed.sum()),
            "other": int((~same & ~flushed & ~normal).sum())}


# ---------------------------------------------------------------------------------------------------------------- special
def special_cases():
    rng = np.random.default_rng(0)
    w5 = F32(np.sqrt(1.0 - np.exp(-5.0)))                        # erfinv: w = -log(1 - x^2) = 5, the branch
    x_exp = _fill([0.0, -0.0, *around(-87.0, 4), 88.0, 88.5, *around(88.0, 2), INF, -INF, NAN, -86.999, -87.3365, -100.0, 89.0, 1e30, -1e30],
                  rng.uniform(-87, 88, N))
    x_log = _fill([FLT_MIN, *around(1.0, 4), *around(1.41421356237, 4), *around(2.0 * 1.41421356237, 2), *around(0.5 * 1.41421356237, 2),
                   FLT_MAX, np.nextafter(FLT_MIN, F32(1)), 2.0, 0.5], np.exp(rng.uniform(-80, 80, N)))
    x_erf = _fill([0.0, -0.0, INF, -INF, 1e-30, -1e-30, 10.0, 13.0, 13.5, 14.0, 20.0, -20.0, 100.0, 1e10, 1e38, -1e38, NAN],
                  rng.uniform(-6, 6, N))
    x_inv = _fill([0.0, -0.0, *around(w5, 8), *around(-w5, 8), ONE_M, -ONE_M, *around(0.9999999, 1), 0.5, -0.5],
                  np.concatenate([rng.uniform(-1, 1, N // 2), 1 - np.exp(rng.uniform(-16, -2, N // 2))]))
    w = -np.log((1.0 - x_inv.astype(np.float64)) * (1.0 + x_inv.astype(np.float64)))
    out = []
    for which, (name, x, br) in enumerate([("exp", x_exp, {}), ("log", x_log, {"folded mantissa": ((np.frexp(x_log)[0] * 2 > 1.4143), 100),
                                                                                  "plain mantissa": ((np.frexp(x_log)[0] * 2 < 1.4141), 100)}),
                                           ("erf", x_erf, {}),
                                           ("erfinv", x_inv, {"w < 5": (w < 4.999, 100), "w >= 5": (w > 5.001, 100),
                                                              "at the branch": (np.abs(w - 5.0) < 1e-4, 5)})]):
        out.append(Case("special", name, "special", [C.c_int(which)], [(x, "aos")], [(1, "aos")], branches=br, oracle=True, info={"x": x}))
    return out


# ---------------------------------------------------------------------------------------------------------------- trig
def phasor_quadrant(freq, opl):
    """(q, safe): the quadrant of fmod(-2 pi f opl, 2 pi) to the nearest multiple of pi / 2, in f64, and whether the phase is far
    enough from a quadrant's border for f32 to agree"""
    ph = np.mod(-2 * np.pi * freq.astype(np.float64) * opl.astype(np.float64), 2 * np.pi)
    t = ph / (np.pi / 2) + 0.5
    big = np.abs(freq.astype(np.float64) * opl.astype(np.float64)) > 1e4
    return np.floor(t).astype(np.int64) & 3, (np.abs(t - np.round(t)) > 1e-2) & ~big


def trig_cases():
    rng = np.random.default_rng(1)
    q = F32(np.pi / 4)
    x_q = _fill([0.0, -0.0, DEN_MIN, -DEN_MIN, DEN_MAX, 1e-40, -1e-40, FLT_MIN, q, -q, *around(q, 1)[1:2], 1e-20], rng.uniform(-q, q, N))
    eighths = [v for k in range(9) for v in around(k / 8.0, 1) if 0.0 <= v <= 1.0]
    x_2pi = _fill([0.0, 1.0, *eighths, DEN_MIN, FLT_MIN], rng.uniform(0, 1, N))
    k8 = np.floor(x_2pi.astype(np.float64) * 4 + 0.5).astype(np.int64) & 3
    safe8 = np.abs((x_2pi.astype(np.float64) * 4 + 0.5) % 1.0 - 0.5) < 0.49
    x_as = _fill([0.0, -0.0, 0.5, -0.5, *around(0.5, 2), DEN_MIN, 1e-20], rng.uniform(-0.5, 0.5, N))
    x_ac = _fill([0.0, -0.0, *around(0.5, 4), *around(-0.5, 4), 1.0, -1.0, np.nextafter(F32(1), F32(0)), np.nextafter(F32(-1), F32(0)),
                  DEN_MIN, 1e-20], rng.uniform(-1, 1, N))
    # phasor_term: quarter periods (freq * opl = k / 4, exact), opl = 0, huge products, negative opl, then the films' ranges
    fq = [0.25] * 17 + [0.5] * 9 + [0.05, 50.0, 1.0, 1e3, 1e4, 1e5, 3e4, 0.125]
    oq = [float(k) for k in range(17)] + [k / 2.0 for k in range(9)] + [0.0, 0.0, 0.0, 1e3, 1e5, 1e4, 3e4, -2.0]
    n_neg = 20000
    freq = _fill(fq, np.exp(rng.uniform(np.log(0.05), np.log(50.0), N)))
    opl = _fill(oq, np.concatenate([rng.uniform(-50.0, 0.0, n_neg), rng.uniform(0.0, 100.0, N - n_neg)]))
    pq, psafe = phasor_quadrant(freq, opl)
    ax = np.abs(x_ac)
    cases = [
        Case("trig", "sincos_quarter", "trig", [C.c_int(0)], [(_planes(x_q), "soa")], [(2, "soa")], info={"x": x_q}),
        Case("trig", "sincos_2pi", "trig", [C.c_int(1)], [(_planes(x_2pi), "soa")], [(2, "soa")], info={"x": x_2pi},
             branches={f"quadrant {k}": (safe8 & (k8 == k), 100) for k in range(4)}),
        Case("trig", "asin_half", "trig", [C.c_int(2)], [(_planes(x_as), "soa")], [(1, "soa")], info={"x": x_as}),
        Case("trig", "acos_f32", "trig", [C.c_int(3)], [(_planes(x_ac), "soa")], [(1, "soa")], info={"x": x_ac},
             branches={"|x| <= 1/2": (ax <= 0.5, 100), "x > 1/2": (x_ac > 0.5, 100), "x < -1/2": (x_ac < -0.5, 100)}),
        Case("trig", "phasor_term", "trig", [C.c_int(4)], [(_planes(freq, opl), "soa")], [(2, "soa")], info={"freq": freq, "opl": opl},
             oracle=True, branches={**{f"quadrant {k}": (psafe & (pq == k), 100) for k in range(4)},
                                    "negative opl": (opl < 0, 100), "opl = 0": (opl == 0, 3),
                                    "huge product": (np.abs(freq.astype(np.float64) * opl) >= 1e6, 3)}),
    ]
    return cases


# ---------------------------------------------------------------------------------------------------------------- warps
def _dirs(n, rng):
    v = rng.normal(size=(n, 3))
    return _unit(v)


AXES = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 0, -0.0), (0, 1, -0.0), (-0.0, -0.0, 1), (-0.0, 0.0, -1)]


def warps_cases():
    rng = np.random.default_rng(2)
    g = np.arange(0, 1024, 16) / 1024.0                               # u on a grid: 2 u - 1 is exact, so |x| == |y| on the diagonals
    e1 = [0.5, 0.0, 0.0, ONE_M, ONE_M, 0.5, 0.5, 0.0, ONE_M, *g, *g[1:], *g[1:], 0.0, ONE_M]
    e2 = [0.5, 0.0, ONE_M, 0.0, ONE_M, 0.0, ONE_M, 0.5, 0.5, *g, *(1.0 - g[1:]), *(0.5 + 0 * g[1:]), 0.25, 0.75]
    n_e = len(e1)
    u1, u2 = _fill(e1, rng.random(N)), _fill(e2, rng.random(N))
    u1[n_e:n_e + 500], u2[n_e + 500:n_e + 1000] = 0.0, 0.0
    u1[n_e + 1000:n_e + 1500], u2[n_e + 1500:n_e + 2000] = ONE_M, ONE_M
    x, y = 2.0 * u1.astype(np.float64) - 1.0, 2.0 * u2.astype(np.float64) - 1.0
    disk_br = {"swap": (np.abs(x) < np.abs(y), 100), "no swap": (np.abs(x) > np.abs(y), 100), "diagonal |x| == |y|": ((np.abs(x) == np.abs(y)) & (x != 0), 100),
               "centre": ((x == 0) & (y == 0), 1), "u = 0": ((u1 == 0) | (u2 == 0), 100), "u = 1 - 2^-24": ((u1 == ONE_M) | (u2 == ONE_M), 100)}
    nn = np.concatenate([np.array(AXES, np.float32), _dirs(N - len(AXES), rng)])
    vv = np.concatenate([np.array(AXES[::-1], np.float32), _dirs(N - len(AXES), rng)])
    nn[100:600] = _unit(nn[100:600] * np.array([1, 1, 1e-4]))         # the frame's 1 / (sign + n.z) next to the equator
    nn[600:1100] = _unit(np.concatenate([1e-4 * rng.normal(size=(500, 2)), -np.ones((500, 1))], 1))       # ... and next to -z
    n3 = [np.ascontiguousarray(nn[:, k]) for k in range(3)]
    v3 = [np.ascontiguousarray(vv[:, k]) for k in range(3)]
    frame_br = {"n.z < 0": (nn[:, 2] < 0, 100), "n.z > 0": (nn[:, 2] > 0, 100), "+z": ((nn[:, 2] == 1) & (nn[:, 0] == 0), 1),
                "-z": ((nn[:, 2] == -1) & (nn[:, 0] == 0), 1), "n.z = -0": ((nn[:, 2] == 0) & np.signbit(nn[:, 2]), 1)}
    ou = _fill([0.0, 1.0, -1.0, 0.0, 0.0, 0.5, -0.5, 0.5, 1.0, -1.0, 0.25, -0.0], rng.uniform(-1, 1, N))
    ov = _fill([0.0, 0.0, 0.0, 1.0, -1.0, 0.5, 0.5, -0.5, 1.0, -1.0, -0.75, -0.0], rng.uniform(-1, 1, N))
    zz = 1.0 - np.abs(ou.astype(np.float64)) - np.abs(ov.astype(np.float64))
    ll = (nn.astype(np.float64) * 10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
    ll[len(AXES)] = 0.0
    l3 = [np.ascontiguousarray(ll[:, k]) for k in range(3)]
    bits = rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x_rcp = _fill([0.0, -0.0, DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX, FLT_MIN, -FLT_MIN, INF, -INF, NAN, 1.0, -1.0, FLT_MAX, 1e-28, 1e-29, -1e-29, 3.0],
                  np.concatenate([bits[:N // 2], ((10.0 ** rng.uniform(-6, 6, N // 2)) * rng.choice([-1.0, 1.0], N // 2)).astype(np.float32)]))
    pa = _fill([0.0, INF, 1.0, 1e20, 0.0, 3.0, INF, 1e-30, FLT_MAX, DEN_MIN], 10.0 ** rng.uniform(-6, 6, N))
    pb = _fill([0.0, 2.0, 1.0, 1e20, 1.0, 0.0, INF, 1e-30, 1.0, DEN_MIN], 10.0 ** rng.uniform(-6, 6, N))
    pb[100:400] = pa[100:400]
    W = lambda name, which, cols, k, br=None, **info: Case("warps", name, "warps", [C.c_int(which)], [(_planes(*cols), "soa")], [(k, "soa")],    # noqa: E731
                                                           branches=br, info=info)
    return [
        W("concentric_disk", 0, (u1, u2), 2, disk_br, u1=u1, u2=u2), W("cosine_hemisphere", 1, (u1, u2), 3, disk_br, u1=u1, u2=u2),
        W("coordinate_system", 2, n3, 6, frame_br, n=nn), W("to_local_about", 3, n3 + v3, 3, frame_br, n=nn, v=vv),
        W("sphere_dir_encode", 4, n3, 2, {"lower half": (nn[:, 2] < 0, 100), "upper half": (nn[:, 2] >= 0, 100)}, n=nn),
        W("sphere_dir_decode", 5, (ou, ov), 3, {"lower half": (zz < -1e-6, 100), "upper half": (zz > 1e-6, 100)}, u=ou, v=ov),
        W("unit_z", 6, l3, 1, {"null vector": ((ll == 0).all(1), 1)}, l=ll),
        W("safe_rcp", 7, (x_rcp,), 1, {"clamped": (np.abs(x_rcp) < F32(1e-29), 100), "zero": (x_rcp == 0, 2),
                                       "denormal": ((np.abs(x_rcp) > 0) & (np.abs(x_rcp) < FLT_MIN), 100), "infinite": (np.isinf(x_rcp), 2)}, x=x_rcp),
        W("mis_weight", 8, (pa, pb), 1, {"0, 0": ((pa == 0) & (pb == 0), 1), "Inf, finite": (np.isinf(pa) & np.isfinite(pb), 1),
                                         "equal": ((pa == pb) & (pa > 0) & np.isfinite(pa), 100)}, a=pa, b=pb),
    ]


# ---------------------------------------------------------------------------------------------------------------- fresnel
CONDUCTORS = [(0.0, 1.0), (1.657, 9.224), (0.880, 6.270), (0.521, 4.837), (0.2, 3.9), (1.5, 0.0), (1.0, 0.0)]      # "none", the suites' eta / k, k = 0
ETAS = [1.0, 1.5, 1.0 / 1.5, 1.000001, 2.4]


def fresnel_dielectric_f64(ci, eta):
    """mtr_core.h fresnel_dielectric in f64: (r, cos_t, eta_it, eta_ti, total internal reflection)"""
    ci, eta = np.asarray(ci, np.float64), np.asarray(eta, np.float64)
    outside = ci >= 0
    eit = np.where(outside, eta, 1 / eta)
    eti = 1 / eit
    ct2 = 1 - (1 - ci * ci) * eti * eti
    cta, cia = np.sqrt(np.maximum(ct2, 0)), np.abs(ci)
    with np.errstate(all="ignore"):
        a_s, a_p = (cia - eit * cta) / (cia + eit * cta), (cta - eit * cia) / (cta + eit * cia)
    r = 0.5 * (a_s * a_s + a_p * a_p)
    r = np.where(eta == 1, 0.0, np.where(cia == 0, 1.0, r))
    return r, np.where(np.signbit(ci), cta, -cta), eit, eti, ct2 <= 0


def fresnel_conductor_f64(ci, er, ei):
    ci, er, ei = (np.asarray(v, np.float64) for v in (ci, er, ei))
    c2 = ci * ci
    s2 = 1 - c2
    t1 = er * er - ei * ei - s2
    a2pb2 = np.sqrt(np.maximum(t1 * t1 + 4 * ei * ei * er * er, 0))
    a = np.sqrt(np.maximum(0.5 * (a2pb2 + t1), 0))
    term1, term2 = a2pb2 + c2, 2 * ci * a
    with np.errstate(all="ignore"):
        rs = (term1 - term2) / (term1 + term2)
        term3, term4 = a2pb2 * c2 + s2 * s2, term2 * s2
        rp = rs * (term3 - term4) / (term3 + term4)
    return 0.5 * (rs + rp)


def falloff_emitter(cutoff_deg, beam_deg):
    """the constants mitransient_amd/scene.py stores for an `angulararea` emitter"""
    import math
    from mitransient_amd import _cabi
    e = _cabi.mtr_emitter()
    cutoff, beam = math.radians(cutoff_deg), math.radians(beam_deg)
    e.angular, e.cutoff, e.cos_cutoff, e.cos_beam = 1, F32(cutoff), F32(math.cos(cutoff)), F32(math.cos(beam))
    e.inv_transition = F32(math.inf if cutoff == beam else 1.0 / (cutoff - beam))
    return e


def fresnel_cases():
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(CONDUCTORS), N)
    ek = np.array(CONDUCTORS, np.float32)[pick]
    ci_c = _fill([0.0, 1.0, -0.0, DEN_MIN, 1e-20, ONE_M, 0.5], rng.uniform(0, 1, N))
    ci_c[100:800] = np.repeat(np.array([0.0, 1.0, ONE_M, 1e-3, 1e-6], np.float32), 140)       # ... with every constant pair
    ek[100:800] = np.tile(np.array(CONDUCTORS, np.float32), (100, 1))
    edge_ci, edge_eta = [], []
    for eta in ETAS:
        edge_ci += [0.0, -0.0, 1.0, -1.0, DEN_MIN, -DEN_MIN]
        edge_eta += [eta] * 6
        if eta != 1.0:                                                # the critical angle, met from the denser side
            e_ti = max(eta, 1.0 / eta)
            c = np.sqrt(1.0 - 1.0 / (e_ti * e_ti)) * (-1.0 if eta > 1.0 else 1.0)
            nbr = around(c, 16)
            edge_ci += nbr
            edge_eta += [eta] * len(nbr)
    eta_d = _fill(edge_eta, np.array(ETAS, np.float32)[rng.integers(0, len(ETAS), N)])
    ci_d = _fill(edge_ci, rng.uniform(-1, 1, N))
    r, ct, eit, eti, tir = fresnel_dielectric_f64(ci_d, eta_d)
    margin = np.abs(1 - (1 - ci_d.astype(np.float64) ** 2) * eti * eti) > 1e-5
    cases = [
        Case("fresnel", "fresnel_conductor", "fresnel", [C.c_int(0)], [(_planes(ci_c, ek[:, 0], ek[:, 1]), "soa")], [(1, "soa")],
             info={"ci": ci_c, "eta": ek[:, 0], "k": ek[:, 1]},
             branches={"k = 0": (ek[:, 1] == 0, 100), "ci = 0": (ci_c == 0, 10), "ci = 1": (ci_c == 1, 10)}),
        Case("fresnel", "fresnel_dielectric", "fresnel", [C.c_int(1)], [(_planes(ci_d, eta_d), "soa")], [(4, "soa")],
             info={"ci": ci_d, "eta": eta_d},
             branches={"total internal reflection": (tir & margin, 100), "refraction": (~tir & margin, 100), "from inside": (ci_d < 0, 100),
                       "index matched": (eta_d == 1, 100), "ci = +0": ((ci_d == 0) & ~np.signbit(ci_d), 5), "ci = -0": ((ci_d == 0) & np.signbit(ci_d), 5),
                       "at the critical angle": (~margin & (np.abs(ci_d) > 0.1) & (eta_d != 1), 90)}),
    ]
    for cutoff, beam in ((20.0, 10.0), (30.0, 30.0), (1.0, 0.5)):
        e = falloff_emitter(cutoff, beam)
        cc, cb = F32(e.cos_cutoff), F32(e.cos_beam)
        x = _fill([1.0, -1.0, *around(cc, 8), *around(cb, 8), 0.0, -0.0], np.concatenate([rng.uniform(-1, 1, N // 2), rng.uniform(cc - 0.01, 1.0, N // 2)]))
        cases.append(Case("fresnel", f"angular_falloff {cutoff:g}/{beam:g}", "angular_falloff", [e], [(x, "aos")], [(1, "aos")], info={"x": x, "emitter": e},
                          branches={"inside the beam": (x >= cb, 100), "outside the cone": (x <= cc, 100), "at the cutoff": (np.abs(x - cc) < 1e-6, 5),
                                    **({"transition": ((x < cb) & (x > cc), 100)} if cutoff != beam else {})}))
    return cases


# ---------------------------------------------------------------------------------------------------------------- bsdf
def bsdf_materials():
    """(name, mtr_material, transmissive): every material kind tests/test_rough_bsdf.py builds, and the smooth ones"""
    import test_rough_bsdf as R
    from mitransient_amd.scene import _SceneBuilder
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    mk = lambda bd, two: _SceneBuilder({}, ".")._make_material({"type": "twosided", "bsdf": bd} if two else bd)      # noqa: E731
    out = []
    for alpha in (0.05, 0.4):
        for kind in R.KINDS:
            for two in (False, True):
                out.append((f"{kind} alpha {alpha}{' twosided' if two else ''}", R._mat(kind, alpha, two), False))
        for kind in R.DKINDS:
            out.append((f"{kind} alpha {alpha}", R._mat(kind, alpha), True))
    for two in (False, True):
        out.append((f"plastic{' twosided' if two else ''}", R._mat("plastic", twosided=two), False))
        out.append((f"conductor{' twosided' if two else ''}", mk({"type": "conductor", "eta": [1.657, 0.880, 0.521], "k": [9.224, 6.270, 4.837]}, two), False))
        out.append((f"diffuse{' twosided' if two else ''}", mk({"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.3, 0.2]}}, two), False))
    out.append(("thindielectric", R._mat("thindielectric"), True))
    out.append(("dielectric", mk({"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0}, False), True))
    return out


def lobe_threshold(m, wi_z):
    """the value of u1 at which bsdf_sample changes lobe for incidence cosine wi_z, in f64 (NaN where u1 selects nothing)"""
    from mitransient_amd import _cabi as A
    z = np.asarray(wi_z, np.float64)
    if m.flags & A.MTR_MAT_TWOSIDED:
        z = np.abs(z)
    eta = float(m.int_ior) / float(m.ext_ior) if m.ext_ior else 1.0
    if m.type == A.MTR_BSDF_DIELECTRIC:
        return fresnel_dielectric_f64(z, eta)[0]
    if m.type == A.MTR_BSDF_THINDIELECTRIC:
        r = fresnel_dielectric_f64(np.abs(z), eta)[0]
        return np.where(r < 1, r * 2 / (1 + r), r)
    w = float(m.specular_sampling_weight)
    if m.type == A.MTR_BSDF_PLASTIC:
        f_i = fresnel_dielectric_f64(z, eta)[0]
        ps, pd = f_i * w, (1 - f_i) * (1 - w)
        return np.where(z > 0, ps / (ps + pd), np.nan)
    if m.type == A.MTR_BSDF_ROUGHPLASTIC:
        tab = np.array(list(m.external_transmittance), np.float64)
        x = np.clip(z, 0, 1) * (len(tab) - 1)
        i = np.minimum(x.astype(np.int64), len(tab) - 2)
        t_i = (1 - (x - i)) * tab[i] + (x - i) * tab[i + 1]
        ps, pd = (1 - t_i) * w, t_i * (1 - w)
        return np.where(z > 0, ps / (ps + pd), np.nan)
    return np.full(z.shape, np.nan)


SWEEP_Z = (1.0, 0.9, 0.6, 0.3, 0.05)


def bsdf_cases():
    from mitransient_amd import _cabi as A
    cases = []
    for k, (name, m, transmissive) in enumerate(bsdf_materials()):
        rng = np.random.default_rng(100 + k)
        n = N_BSDF
        upper = not (transmissive or (m.flags & A.MTR_MAT_TWOSIDED))

        def dirs(up):
            v = _dirs(n, rng)
            if up:
                v[:, 2] = np.abs(v[:, 2])
            return v
        wi, wo = dirs(upper), dirs(False)
        wi[:1000, 2] *= 1e-3; wo[1000:2000, 2] *= 1e-3                      # grazing
        wi[2000:2100] = [0, 0, 1]                                           # perpendicular incidence
        if not upper:
            wi[2050:2100] = [0, 0, -1]
        wi[0], wo[0] = [0, 0, 1], [0, 0, 1]
        cases.append(Case("bsdf", f"eval_pdf {name}", "bsdf_eval_pdf", [m], [(wi, "aos"), (wo, "aos")], [(3, "aos"), (1, "aos")], n_type=C.c_uint32,
                          oracle=True, info={"material": m, "wi": wi, "wo": wo},
                          branches={"grazing": (np.abs(wi[:, 2]) < 1e-3, 100), "perpendicular": (np.abs(wi[:, 2]) == 1, 50)}))
        ws = dirs(upper)
        u = rng.random((3, n)).astype(np.float32)
        ws[0] = [0, 0, 1]; u[:, 0] = 0.5
        pos = 1
        for z in SWEEP_Z:                                                   # the lobe-selection threshold of this incidence, +- 16 ulp
            d = np.array([np.sqrt(1 - z * z), 0.0, z], np.float32)
            for sgn in ((1.0, -1.0) if not upper else (1.0,)):
                dd = d * np.array([1, 1, sgn], np.float32)
                t = lobe_threshold(m, np.array([dd[2]], np.float32))[0]
                vals = around(t if np.isfinite(t) else 0.5, 16)
                ws[pos:pos + len(vals)] = dd; u[0, pos:pos + len(vals)] = vals
                pos += len(vals)
        for a in (0.0, ONE_M):                                              # the ends of every random number
            for b in (0.0, ONE_M, 0.5):
                for c in (0.0, ONE_M, 0.5):
                    u[:, pos] = (a, b, c); pos += 1
        u = np.clip(u, 0.0, ONE_M)
        ws[1000:2000, 2] *= 1e-3
        ws[2000:2100] = [0, 0, 1]
        if not upper:
            ws[2050:2100] = [0, 0, -1]
        thr = lobe_threshold(m, ws[:, 2])
        br = {"u = 0": ((u == 0).any(0), 6), "u = 1 - 2^-24": ((u == ONE_M).any(0), 6), "grazing": (np.abs(ws[:, 2]) < 1e-3, 100),
              "perpendicular": (np.abs(ws[:, 2]) == 1, 50)}
        if np.isfinite(thr).any():
            first, second = (("reflection", "transmission") if transmissive else ("specular lobe", "diffuse lobe"))
            br.update({first: (u[0] < thr - 1e-4, 100), second: (u[0] > thr + 1e-4, 100), "at the threshold": (np.abs(u[0] - thr) < 4e-6, 30)})
        cases.append(Case("bsdf", f"sample {name}", "bsdf_sample", [m], [(ws, "aos"), (u[0].copy(), "aos"), (u[1].copy(), "aos"), (u[2].copy(), "aos")],
                          [(3, "aos"), (1, "aos"), (3, "aos")], n_type=C.c_uint32, oracle=True, branches=br,
                          info={"material": m, "wi": ws, "u": u, "transmissive": transmissive, "rough_dielectric": m.type == A.MTR_BSDF_ROUGHDIELECTRIC}))
    return cases


# ---------------------------------------------------------------------------------------------------------------- rng
def rng_cases():
    from mitransient_amd import _cabi as A
    rng = np.random.default_rng(5)
    seeds, lanes = [0, 1, 0xffffffff], [0, 1, 63, 64, 0xffffffff]
    flags = [0, A.MTR_FLAG_PCG_INITSEQ_PLUS_LANE, A.MTR_FLAG_PCG_TEA64, A.MTR_FLAG_PCG_INITSEQ_PLUS_LANE | A.MTR_FLAG_PCG_TEA64, 0xffffffff,
             A.MTR_FLAG_DETERMINISTIC | A.MTR_FLAG_KEEP_COUNTERS]
    grid = np.array([(s, l, f) for f in flags for s in seeds for l in lanes], np.uint32)
    n_r = N - len(grid)
    rand = np.stack([np.array(seeds, np.uint32)[rng.integers(0, 3, n_r)], rng.integers(0, 2 ** 32, n_r, dtype=np.uint64).astype(np.uint32),
                     np.array(flags, np.uint32)[rng.integers(0, len(flags), n_r)]], 1)
    rand[: n_r // 4, 0] = rng.integers(0, 2 ** 32, n_r // 4, dtype=np.uint64).astype(np.uint32)
    rand[n_r // 4: n_r // 2, 1] = np.arange(n_r // 2 - n_r // 4, dtype=np.uint32)                # the lanes of a small render, in order
    x = np.ascontiguousarray(np.concatenate([grid, rand]).T)
    br = {f"flags {f:#x}": (x[2] == f, 100) for f in flags}
    br.update({f"lane {l:#x}": (x[1] == l, len(seeds)) for l in lanes})
    return [Case("rng", "rng_seed / rng_u32 / rng_f32 / tea4 / rng_inc_of", "rng", [], [(x, "soa")], [(24, "soa")], branches=br, info={"x": x})]


# ---------------------------------------------------------------------------------------------------------------- film
FILMS = {"transient T=1": (3.5, 6.0, 1, 1, 0), "transient T=64": (3.5, 6.0 / 64, 64, 1, 0), "transient T=4096": (3.5, 6.0 / 4096, 4096, 1, 0),
         "nlos T=4096": (1.85, 2.0 ** -11, 4096, 1, 0), "phasor": (0.0, 1.0, 1, 1, 3), "exhaustive 6 lasers": (1.85, 0.03, 64, 6, 0)}


def film_cases():
    rng = np.random.default_rng(6)
    cases = []
    for name, (start, bw, tbins, lasers, n_freq) in FILMS.items():
        start, bw = F32(start), F32(bw)
        end = F32(start + bw * F32(tbins))
        edges = (start + bw * np.arange(tbins + 1, dtype=np.float32)).astype(np.float32)
        e = np.concatenate([[start, end, INF, -INF, NAN, 3e38, -3e38, np.nextafter(start, -INF), np.nextafter(end, -INF), np.nextafter(end, INF),
                             start - 1, end + 1, 0.0, -0.0],
                            edges, np.nextafter(edges, -INF), np.nextafter(edges, INF)]).astype(np.float32)
        opl = _fill(e, rng.uniform(start - 0.2 * (end - start) - 0.1, end + 0.2 * (end - start) + 0.1, N))
        laser = rng.integers(0, lasers + 1, N).astype(np.uint32)
        laser[:14] = 0
        laser[14:40] = np.tile(np.array([lasers - 1, lasers], np.uint32), 13)
        pos = (opl.astype(np.float64) - float(start)) / float(bw)
        with np.errstate(invalid="ignore"):
            far = np.abs(pos - np.round(pos)) > 1e-3                       # not at an edge: f32 and f64 agree on the bin
        br = {"NaN": (np.isnan(opl), 1), "Inf": (np.isinf(opl), 2), "+-3e38": (np.abs(opl) == F32(3e38), 2),
              "laser = lasers - 1": (laser == lasers - 1, 10), "laser = lasers": (laser == lasers, 10)}
        if not n_freq:
            br.update({"below the start": (far & (pos < 0), 100), "beyond the end": (far & (pos >= tbins), 100), "bin 0": (far & (pos > 0) & (pos < 1), 1),
                       "bin T - 1": (far & (pos > tbins - 1) & (pos < tbins), 1), "inside": (far & (pos >= 0) & (pos < tbins), 100),
                       "at an edge": (~far & np.isfinite(pos), min(300, 3 * tbins))})
        cases.append(Case("film", name, "film", [C.c_float(start), C.c_float(bw), C.c_uint32(tbins), C.c_uint32(lasers), C.c_uint32(n_freq)],
                          [(_planes(opl, laser), "soa")], [(2, "soa")], branches=br,
                          info={"opl": opl, "laser": laser, "start": start, "bw": bw, "tbins": tbins, "lasers": lasers, "n_freq": n_freq}))
    return cases


# ---------------------------------------------------------------------------------------------------------------- pairs
SPECIALS = np.array([0.0, -0.0, DEN_MIN, DEN_MAX, FLT_MIN, 1.0, FLT_MAX, INF, -INF, NAN], np.float32)


def pairs_cases():
    rng = np.random.default_rng(7)
    x = rng.integers(0, 2 ** 32, (6, N), dtype=np.uint64).astype(np.uint32).view(np.float32)          # the whole exponent range, every class of value
    S, k = SPECIALS, len(SPECIALS)
    g3 = np.array(np.meshgrid(S, S, S, indexing="ij")).reshape(3, -1)                                 # (a, b, c) of one half, the other half random
    g4 = np.array(np.meshgrid(S, S, S, S, indexing="ij")).reshape(4, -1)                              # a and b, both halves
    p = 0
    x[0, p:p + k ** 3], x[2, p:p + k ** 3], x[4, p:p + k ** 3] = g3; p += k ** 3
    x[1, p:p + k ** 3], x[3, p:p + k ** 3], x[5, p:p + k ** 3] = g3; p += k ** 3
    x[0:4, p:p + k ** 4] = g4
    x[4, p:p + k ** 4], x[5, p:p + k ** 4] = np.resize(S, k ** 4), np.resize(S[::-1], k ** 4); p += k ** 4
    tame = slice(p, p + 50000)                                                                        # ordinary magnitudes: results that round
    x[:, tame] = (rng.normal(size=(6, 50000)) * 10.0 ** rng.uniform(-3, 3, (6, 50000))).astype(np.float32)
    xw = np.ascontiguousarray(x).view(np.uint32)
    cls = lambda v: np.isnan(v) | np.isinf(v) | (np.abs(v) < FLT_MIN)                                 # noqa: E731
    br = {"special beside ordinary (x)": (cls(x[0]) & ~cls(x[1]), 100), "special beside ordinary (y)": (cls(x[1]) & ~cls(x[0]), 100),
          "denormal operand": (((np.abs(x) < FLT_MIN) & (x != 0)).any(0), 100), "NaN operand": (np.isnan(x).any(0), 100),
          "ordinary": ((~cls(x)).all(0), 100)}
    return [Case("pairs", "mul2 / sub2 / add2 / fma2", "pairs", [], [(xw, "soa")], [(16, "soa")], branches=br, info={"x": x})]


_MAKERS = {"special": special_cases, "trig": trig_cases, "warps": warps_cases, "fresnel": fresnel_cases, "bsdf": bsdf_cases, "rng": rng_cases,
           "film": film_cases, "pairs": pairs_cases}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(_MAKERS[family]())
