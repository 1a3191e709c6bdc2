"""The CPU side of the known-answer harness (tests/kat_cases.py), which keeps tests/test_gpu_kat.py from passing vacuously: the
inputs reach every branch of every family (derived from the inputs in numpy, not from the code under test); the host twin
(tests/host_harness.cpp, what the device is compared with) equals the oracle bit for bit wherever the oracle exports the function;
and the host twin is within a stated distance of a numpy / scipy f64 evaluation of the same formula — the project's existing
tolerances where it has one, else the error measured on the host (an approximation error, so the host is the thing to measure) with
a factor 2 of margin, the measured figure beside the assertion."""
import numpy as np
import pytest

import kat_cases as K

F64 = np.float64


def _host(host_harness, case, n=None):
    return case.run_cpu(host_harness, "hh_", n)


# ---------------------------------------------------------------------------------------------------------- branch coverage
@pytest.mark.parametrize("family", K.FAMILIES)
def test_inputs_reach_every_branch(family, oracle):
    cases = K.cases(family)
    assert cases and all(c.n % 64 and c.n % 256 for c in cases)
    assert all(c.n == (K.N_BSDF if family == "bsdf" else K.N) for c in cases)
    for c in cases:
        for name, (mask, least) in c.branches.items():
            assert mask.shape == (c.n,) and int(mask.sum()) >= least, (family, c.name, name, int(mask.sum()), least)
        if c.info.get("rough_dielectric"):
            # which lobe a rough dielectric takes depends on the sampled normal: read it off the ORACLE's sample (not the host twin's)
            wo, pdf, w = (o.view(np.float32) for o in c.run_cpu(oracle.lib(), "orc_"))
            side = wo[:, 2] * c.info["wi"][:, 2]
            for inside in (False, True):
                sel = (pdf > 0) & ((c.info["wi"][:, 2] < 0) == inside)
                assert (sel & (side > 0)).sum() >= 100 and (sel & (side < 0)).sum() >= 100, (c.name, inside)
    if family == "bsdf":
        names = " ".join(c.name for c in cases)
        import test_rough_bsdf as R
        for kind in R.KINDS + R.DKINDS + ["plastic", "thindielectric", "conductor", "dielectric", "diffuse"]:
            assert f"eval_pdf {kind}" in names and f"sample {kind}" in names, kind
        assert "alpha 0.05" in names and "alpha 0.4" in names and "twosided" in names
        from mitransient_amd import _cabi as A
        for c in cases:                          # dielectrics from outside and from inside
            if c.info.get("transmissive") and c.info["material"].type != A.MTR_BSDF_THINDIELECTRIC:
                z = c.info["wi"][:, 2]
                assert (z > 0).sum() >= 1000 and (z < 0).sum() >= 1000, c.name
    if family == "trig":
        ph = {c.name: c for c in cases}["phasor_term"]
        f, o = ph.info["freq"], ph.info["opl"]
        assert f.min() >= np.float32(0.05) and f[34:].max() <= 50.0 and o[34:].max() <= 100.0
        quarter = (np.mod(4.0 * f.astype(F64) * o.astype(F64), 1.0) == 0) & (o > 0)
        assert quarter.sum() >= 20                                      # products that are exact multiples of a quarter period


@pytest.mark.parametrize("family", K.FAMILIES)
def test_small_runs_equal_the_head_of_the_full_run(family, host_harness):
    """n = 1 and n = 63 (what the device test also runs) see the first elements, edges included, in their own plane layout"""
    for c in K.cases(family):
        full = _host(host_harness, c)
        for n in K.SMALL_N:
            head = [(x[..., :n] if lay == "soa" else x[:n]) for x, (_, lay) in zip(full, c.outs)]
            assert K.report(c, "n small", head, _host(host_harness, c, n), n, ("head", "small")) is None


# ------------------------------------------------------------------------------------------------- host twin == oracle
@pytest.mark.parametrize("family", ["special", "bsdf"])
def test_host_twin_equals_oracle(family, oracle, host_harness):
    for c in K.cases(family):
        assert c.oracle
        msg = K.report(c, "host twin against oracle", c.run_cpu(oracle.lib(), "orc_"), _host(host_harness, c), c.n, ("oracle", "host  "))
        assert msg is None, msg


def test_host_phasor_term_equals_oracle(oracle, host_harness):
    c = {c.name: c for c in K.cases("trig")}["phasor_term"]
    cs = _host(host_harness, c)[0].view(np.float32)
    idx = np.concatenate([np.arange(2000), np.arange(2000, c.n, 5)])
    f, o = c.info["freq"], c.info["opl"]
    ref = np.array([oracle.phasor_term(f[i], o[i]) for i in idx], np.float32)
    assert np.array_equal(ref[:, 0].view(np.uint32), cs[0, idx].view(np.uint32)) and np.array_equal(ref[:, 1].view(np.uint32), cs[1, idx].view(np.uint32))


def test_host_film_bin_equals_oracle(oracle, host_harness):
    for c in K.cases("film"):
        i = c.info
        if i["n_freq"]:
            continue
        got = _host(host_harness, c)[0].view(np.int32)[0]
        idx = np.concatenate([np.arange(min(c.n, 14 + 3 * (i["tbins"] + 1))), np.arange(13000, c.n, 97)])
        idx = idx[np.isfinite(i["opl"][idx])]               # (the oracle's callers filter non-finite distances before the bin)
        ref = np.array([oracle.bin_index(i["opl"][k], i["start"], i["bw"], i["tbins"]) for k in idx])
        assert np.array_equal(ref, got[idx]), (c.name, idx[np.flatnonzero(ref != got[idx])[:10]])


# ------------------------------------------------------------------------------------------------- f64 references
def _err(got, ref, kind="abs", floor=1e-30):
    e = np.abs(got.astype(F64) - ref)
    if kind == "rel":
        e = e / np.maximum(np.abs(ref), floor)
    return float(np.nanmax(e))


def _check(label, measured, bound):
    print(f"[kat f64] {label}: measured {measured:.3e}, bound {bound:.1e}")
    assert measured <= bound, (label, measured, bound)


def test_special_against_f64(host_harness):
    """test_rough_bsdf.py::test_special_functions' tolerances (2e-7 / 2e-7 / 3e-6 / 6e-7) on its ranges, and the exact ends"""
    from scipy import special
    cs = {c.name: c for c in K.cases("special")}
    y = {k: _host(host_harness, c)[0].view(np.float32) for k, c in cs.items()}
    x = {k: c.info["x"] for k, c in cs.items()}
    X = {k: v.astype(F64) for k, v in x.items()}
    m = (x["exp"] > -87) & (x["exp"] <= 88)
    _check("exp rel", _err(y["exp"][m], np.exp(X["exp"][m]), "rel"), 2e-7)
    assert np.all(y["exp"][~(x["exp"] > -87)] == 0) and np.all(y["exp"][x["exp"] > 88] == y["exp"][x["exp"] == 88][0])      # 0 below, clamped above; NaN -> 0
    assert y["exp"][0] == 1.0 and y["exp"][1] == 1.0 and np.all(y["exp"][m] >= np.float32(1.17549435e-38))                   # +-0; never a denormal
    _check("log rel1", _err(y["log"], np.log(X["log"]), "rel", 1e-3), 2e-7)
    m = np.isfinite(x["erf"])
    _check("erf abs", _err(y["erf"][m], special.erf(X["erf"][m])), 3e-6)
    assert y["erf"][x["erf"] == np.inf][0] == 1.0 and y["erf"][x["erf"] == -np.inf][0] == -1.0 and np.all(np.abs(y["erf"][m]) <= 1.0)
    assert np.all(y["erf"][np.abs(x["erf"]) >= 10] == np.sign(x["erf"][np.abs(x["erf"]) >= 10]))                             # t^16 overflows: 1 - 1 / Inf
    m = np.abs(x["erfinv"]) < 0.9999999
    _check("erfinv rel", _err(y["erfinv"][m], special.erfinv(X["erfinv"][m]), "rel"), 6e-7)
    assert np.isfinite(y["erfinv"]).all() and np.array_equal(np.signbit(y["erfinv"]), np.signbit(x["erfinv"]))               # up to 1 - 2^-24; +-0 keep their sign


def test_trig_against_f64(host_harness):
    cs = {c.name: c for c in K.cases("trig")}
    out = {k: _host(host_harness, c)[0].view(np.float32) for k, c in cs.items()}
    x = cs["sincos_quarter"].info["x"].astype(F64)
    _check("sincos_quarter", max(_err(out["sincos_quarter"][0], np.sin(x)), _err(out["sincos_quarter"][1], np.cos(x))), 2 * 7.4e-8)       # measured 7.4e-8
    u = cs["sincos_2pi"].info["x"]
    ph = (np.float32(6.283185307179586) * u).astype(F64)                  # the function's own f32 phase, then f64 sin / cos of it
    _check("sincos_2pi", max(_err(out["sincos_2pi"][0], np.sin(ph)), _err(out["sincos_2pi"][1], np.cos(ph))), 2 * 9.2e-8)                  # measured 9.2e-8
    x = cs["asin_half"].info["x"].astype(F64)
    _check("asin_half", _err(out["asin_half"][0], np.arcsin(x)), 2 * 3.4e-8)                                                                # measured 3.4e-8
    # acos_f32: test_angular_emitter.py's bound, 2 ulp of the f32 result
    x = cs["acos_f32"].info["x"].astype(F64)
    ref = np.arccos(x)
    ulp = np.spacing(ref.astype(np.float32)).astype(F64)
    _check("acos_f32 (ulp)", float((np.abs(out["acos_f32"][0].astype(F64) - ref) / ulp).max()), 2.0)
    # phasor_term: test_phasor.py's bound, 3e-7 against f64 cos / sin of the reference's f32 phase
    f, o = cs["phasor_term"].info["freq"], cs["phasor_term"].info["opl"]
    xx = (np.float32(-2 * np.pi) * f) * o
    yy = np.float32(2 * np.pi)
    phase = (xx - yy * np.floor(xx / yy)).astype(F64)
    _check("phasor_term", max(_err(out["phasor_term"][0], np.cos(phase)), _err(out["phasor_term"][1], np.sin(phase))), 3e-7)
    assert tuple(out["phasor_term"][:, np.flatnonzero(o == 0)[0]]) == (1.0, 0.0)


def _frame64(n):
    sign = np.copysign(1.0, n[:, 2])
    a = -1.0 / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    s = np.stack([sign * n[:, 0] * n[:, 0] * a + 1.0, sign * b, -sign * n[:, 0]], 1)
    t = np.stack([b, n[:, 1] * n[:, 1] * a + sign, -n[:, 1]], 1)
    return s, t


def _disk64(u1, u2):
    x, y = 2.0 * u1.astype(F64) - 1.0, 2.0 * u2.astype(F64) - 1.0
    swap = np.abs(x) < np.abs(y)
    r, rp = np.where(swap, y, x), np.where(swap, x, y)
    with np.errstate(all="ignore"):
        phi = np.where((x == 0) & (y == 0), 0.0, (np.pi / 4) * rp / r)
    s, c = np.sin(phi), np.cos(phi)
    return r * np.where(swap, s, c), r * np.where(swap, c, s)


def test_warps_against_f64(host_harness):
    """no bound existed for these: the host twin's largest error against the same formula in f64, measured, times 2"""
    cs = {c.name: c for c in K.cases("warps")}
    out = {k: _host(host_harness, c)[0].view(np.float32) for k, c in cs.items()}
    i = cs["concentric_disk"].info
    px, py = _disk64(i["u1"], i["u2"])
    _check("concentric_disk", max(_err(out["concentric_disk"][0], px), _err(out["concentric_disk"][1], py)), 2 * 1.7e-7)                  # measured 1.7e-7
    _check("cosine_hemisphere xy", max(_err(out["cosine_hemisphere"][0], px), _err(out["cosine_hemisphere"][1], py)), 2 * 1.7e-7)         # measured 1.7e-7
    z = np.sqrt(np.maximum(1.0 - (px * px + py * py), 0.0))
    # (z = sqrt(1 - r^2): at the rim an error of 1e-7 in r^2 is one of 3e-4 in z; in z^2 it stays small)
    _check("cosine_hemisphere z^2", _err(out["cosine_hemisphere"][2].astype(F64) ** 2, z * z), 2 * 2.4e-7)                                # measured 2.4e-7
    n = cs["coordinate_system"].info["n"].astype(F64)
    s, t = _frame64(n)
    got = out["coordinate_system"].astype(F64).T
    _check("coordinate_system", max(_err(got[:, :3], s), _err(got[:, 3:], t)), 2 * 1.4e-7)                                                 # measured 1.4e-7
    v = cs["to_local_about"].info["v"].astype(F64)
    ref = np.stack([(v * s).sum(1), (v * t).sum(1), (v * n).sum(1)], 1)
    _check("to_local_about", _err(out["to_local_about"].astype(F64).T, ref), 2 * 1.3e-7)                                                   # measured 1.3e-7
    inv = 1.0 / np.abs(n).sum(1)
    qx, qy = n[:, 0] * inv, n[:, 1] * inv
    low = n[:, 2] < 0
    eu = np.where(low, np.copysign(1 - np.abs(qy), qx), qx)
    ev = np.where(low, np.copysign(1 - np.abs(qx), qy), qy)
    _check("sphere_dir_encode", max(_err(out["sphere_dir_encode"][0], eu), _err(out["sphere_dir_encode"][1], ev)), 2 * 1.4e-7)             # measured 1.4e-7
    u, w = cs["sphere_dir_decode"].info["u"].astype(F64), cs["sphere_dir_decode"].info["v"].astype(F64)
    zz = 1 - np.abs(u) - np.abs(w)
    low = zz < 0
    d = np.stack([np.where(low, np.copysign(1 - np.abs(w), u), u), np.where(low, np.copysign(1 - np.abs(u), w), w), zz], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    _check("sphere_dir_decode", _err(out["sphere_dir_decode"].astype(F64).T, d), 2 * 1.5e-7)                                               # measured 1.5e-7
    l = cs["unit_z"].info["l"].astype(F64)                                                                                                # noqa: E741
    ok = (l != 0).any(1)
    _check("unit_z", _err(out["unit_z"][0][ok], l[ok, 2] / np.linalg.norm(l[ok], axis=1)), 2 * 1.6e-7)                                     # measured 1.6e-7
    assert np.isnan(out["unit_z"][0][~ok]).all()
    x = cs["safe_rcp"].info["x"]
    with np.errstate(all="ignore"):
        r = (np.float32(1.0) / x).astype(np.float32)                      # correctly rounded, as the host has it
    r = np.where(np.abs(r) <= np.float32(1e28), r, np.copysign(np.float32(1e28), x)).astype(np.float32)
    assert np.array_equal(r.view(np.uint32)[~np.isnan(x)], out["safe_rcp"][0].view(np.uint32)[~np.isnan(x)])
    a, b = cs["mis_weight"].info["a"].astype(F64), cs["mis_weight"].info["b"].astype(F64)
    with np.errstate(all="ignore"):
        a2, b2 = (a.astype(np.float32) ** 2).astype(F64), (b.astype(np.float32) ** 2).astype(F64)      # (the squares in f32: they overflow there)
        wgt = a2 / (a2 + b2)
    wgt = np.where(np.isfinite(wgt), wgt, 0.0)
    _check("mis_weight", _err(out["mis_weight"][0], wgt), 2 * 8.7e-8)                                                                       # measured 8.7e-8


def test_fresnel_against_f64(host_harness):
    """no bound existed for these either: measured on the host against the same formula in f64, times 2"""
    cs = {c.name: c for c in K.cases("fresnel")}
    c = cs["fresnel_conductor"]
    got = _host(host_harness, c)[0].view(np.float32)[0]
    # (eta = 1, k = 0 is no conductor at all: r = 0 by cancellation of everything, garbage in any precision — compared on the device, not here)
    real = ~((c.info["eta"] == 1) & (c.info["k"] == 0))
    _check("fresnel_conductor", _err(got[real], K.fresnel_conductor_f64(c.info["ci"], c.info["eta"], c.info["k"])[real]), 2 * 7.3e-7)     # measured 7.3e-7
    c = cs["fresnel_dielectric"]
    got = _host(host_harness, c)[0].view(np.float32)
    ci, eta = c.info["ci"], c.info["eta"]
    r, ct, eit, eti, tir = K.fresnel_dielectric_f64(ci, eta)
    # away from the critical angle (|1 - sin^2 / eta^2| > 1e-5: next to it sqrt turns an ulp of cos^2 theta_t into 3e-4 of cos theta_t)
    # ... and from a denormal |ci|: eta_it * |ci| rounds to zero there and r is 0 / 0 = NaN when eta_it < 1/2 (ci = -1e-45, eta 2.4),
    # in the oracle, on the host and on the device alike; no cosine of a real direction is that small
    far = (c.branches["total internal reflection"][0] | c.branches["refraction"][0]) & ((ci == 0) | (np.abs(ci) >= K.FLT_MIN))
    assert np.isfinite(got[:, far]).all()
    _check("fresnel_dielectric r", _err(got[0][far], r[far]), 2 * 5.2e-5)                                                                  # measured 5.2e-5
    _check("fresnel_dielectric cos_t", _err(got[1][far], ct[far]), 2 * 4.7e-6)                                                             # measured 4.7e-6
    _check("fresnel_dielectric eta", max(_err(got[2], eit, "rel"), _err(got[3], eti, "rel")), 2.0 ** -24)                                  # one rounding of 1 / eta
    assert np.all(got[0][tir & far] == 1.0) and np.all(got[1][tir & far] == 0.0)                    # total internal reflection is exact
    zero = ci == 0
    assert np.all(got[0][zero & (eta != 1)] == 1.0) and np.all(got[0][eta == 1] == 0.0)
    assert np.array_equal(np.signbit(got[1][~tir & far]), ~np.signbit(ci[~tir & far]))             # cos_t opposes ci, the sign of ci = -0 included
    for name, c in cs.items():
        if not name.startswith("angular_falloff"):
            continue
        e, x = c.info["emitter"], c.info["x"]
        got = _host(host_harness, c)[0].view(np.float32)
        with np.errstate(all="ignore"):
            beam = np.where(x >= np.float32(e.cos_beam), 1.0, (F64(e.cutoff) - np.arccos(x.astype(F64))) * F64(e.inv_transition))
        ref = np.where(x > np.float32(e.cos_cutoff), beam, 0.0)
        # acos_f32 is good to 2 ulp of an angle below pi (4.8e-7), the subtraction rounds once more, times 1 / transition
        bound = (2 * 2.4e-7 + 2.0 ** -24) * float(e.inv_transition) if np.isfinite(e.inv_transition) else 0.0
        _check(name, _err(got, ref), bound)


def _tea4_np(v0, v1):
    v0, v1 = v0.astype(np.uint32).copy(), v1.astype(np.uint32).copy()
    s = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(4):
            s = np.uint32((int(s) + 0x9e3779b9) & 0xffffffff)
            v0 += ((v1 << np.uint32(4)) + np.uint32(0xa341316c)) ^ (v1 + s) ^ ((v1 >> np.uint32(5)) + np.uint32(0xc8013ea4))
            v1 += ((v0 << np.uint32(4)) + np.uint32(0xad90777d)) ^ (v0 + s) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7e95761e))
    return v0, v1


def _pcg_next(state, inc):
    with np.errstate(over="ignore"):
        new = state * np.uint64(0x5851f42d4c957f2d) + inc
    xs = (((state >> np.uint64(18)) ^ state) >> np.uint64(27)).astype(np.uint32)
    rot = (state >> np.uint64(59)).astype(np.uint32)
    return new, (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))


def test_rng_against_integer_reference(host_harness):
    """PCG32 (O'Neill) seeded through TEA (4 rounds), in numpy's wrapping integers: every word, exactly"""
    from mitransient_amd import _cabi as A
    c = K.cases("rng")[0]
    got = _host(host_harness, c)[0]
    seed, lane, flags = c.info["x"]
    v0, v1 = _tea4_np(seed, lane)
    w0, w1 = _tea4_np(lane, seed)
    tea64 = (flags & A.MTR_FLAG_PCG_TEA64) != 0
    plus = (flags & A.MTR_FLAG_PCG_INITSEQ_PLUS_LANE) != 0
    u64 = lambda lo, hi: lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))       # noqa: E731
    zero = np.zeros_like(v0)
    with np.errstate(over="ignore"):
        st = np.where(tea64, u64(v0, v1), u64(v0, zero))
        sq = np.where(tea64, u64(w0, w1), v1.astype(np.uint64) + np.where(plus, lane.astype(np.uint64), np.uint64(0)))
        inc = (sq << np.uint64(1)) | np.uint64(1)
        state, _ = _pcg_next(np.zeros_like(st), inc)
        state = state + st
    state, _ = _pcg_next(state, inc)
    assert np.array_equal(got[16], v0) and np.array_equal(got[17], v1)
    assert np.array_equal(u64(got[18], got[19]), inc) and np.array_equal(u64(got[22], got[23]), inc) and np.array_equal(u64(got[20], got[21]), state)
    for k in range(16):
        state, r = _pcg_next(state, inc)
        if k < 8:
            assert np.array_equal(got[k], r), k
        else:
            assert np.array_equal(got[k], (((r >> np.uint32(9)) | np.uint32(0x3f800000)).view(np.float32) - np.float32(1.0)).view(np.uint32)), k
    assert len(np.unique(got[0])) > 0.99 * c.n


def test_film_against_f64(host_harness):
    """away from a bin's edge (1e-3 of a bin) the f64 position decides the bin; -1 for each of its reasons; rows of the exhaustive film"""
    for c in K.cases("film"):
        i = c.info
        b, row = _host(host_harness, c)[0].view(np.int32)
        opl, laser = i["opl"], i["laser"]
        if i["n_freq"]:
            assert np.array_equal(b, np.where(np.isfinite(opl), 0, -1))
        else:
            pos = (opl.astype(F64) - F64(i["start"])) / F64(i["bw"])
            far = c.branches["inside"][0] | c.branches["below the start"][0] | c.branches["beyond the end"][0]
            bin64 = lambda p: np.where((p >= 0) & (p < i["tbins"]), np.floor(np.where(np.isfinite(p), p, 0)), -1).astype(np.int64)      # noqa: E731
            assert np.array_equal(b[far], bin64(pos)[far]), c.name
            assert np.all(b[~np.isfinite(opl)] == -1) and np.all((b >= -1) & (b < i["tbins"]))
            assert (b == 0).any() and (b == i["tbins"] - 1).any()
            at = ~far & np.isfinite(pos)                                          # at an edge: the bin on one of its two sides
            assert np.all((b[at] == bin64(pos - 1e-3)[at]) | (b[at] == bin64(pos + 1e-3)[at])), c.name
        assert np.array_equal(row, np.where((b < 0) | (laser >= i["lasers"]), -1, laser.astype(np.int64) * i["tbins"] + b))
        assert (row[laser == i["lasers"]] == -1).all()


def test_pairs_against_numpy(host_harness):
    """mul2 / sub2 / add2 against numpy's IEEE f32 operations, word for word (the plain form is all the host has; fma2 is C's fmaf,
    which numpy cannot restate without a second rounding: it is held to the f64 value within half an ulp plus that rounding)"""
    c = K.cases("pairs")[0]
    got = _host(host_harness, c)[0]
    assert np.array_equal(got[:8], got[8:])
    x = c.info["x"]
    a, b, cc = x[0:2], x[2:4], x[4:6]
    with np.errstate(all="ignore"):
        for k, ref in enumerate((a * b, a - b, a + b)):
            g = got[2 * k:2 * k + 2]
            same = (g == ref.view(np.uint32)) | (np.isnan(g.view(np.float32)) & np.isnan(ref))
            assert same.all(), (k, np.flatnonzero(~same.all(0))[:10])
        ref = a.astype(F64) * b.astype(F64) + cc.astype(F64)
        g = got[6:8].view(np.float32)
        fin = np.isfinite(ref) & (np.abs(ref) < 3e38) & (np.abs(ref) > 1e-30)
        assert np.all(np.abs(g[fin].astype(F64) - ref[fin]) <= np.abs(ref[fin]) * 2.0 ** -24 * (1 + 2.0 ** -20))
        assert np.array_equal(np.isnan(g), np.isnan(ref.astype(np.float32)) | np.isnan(ref))
