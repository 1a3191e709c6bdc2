"""The `angulararea` emitter against the oracle's restatement of mitransient/emitters/angulararea.py (oracle/mtr_oracle.c: the
falloff's transition in f64, the local direction normalized as the plugin's dr.normalize does): the f64 falloff against numpy, the
product's f32 falloff (mtr_core.h angular_falloff through tests/host_harness.cpp) against it at the cone's edges, and the host build
of the product's path arithmetic against the oracle's render, scene by scene (tests/angular_cases.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import angular_cases as AC
from conftest import rel_l2

# (cutoff_angle, beam_width) in degrees: the notebook's, the default (a step: infinite transition), and the edges
PAIRS = [(35, 20), (10, 10), (60, 30), (90, 0), (180, 120), (2, 1), (30, 29.999)]


def _emitter(cutoff, beam):
    from mitransient_amd import _cabi
    from mitransient_amd.scene import _angular_constants
    e = _cabi.mtr_emitter()
    _angular_constants(e, {"cutoff_angle": cutoff, "beam_width": beam})
    return e


def _numpy_falloff(e, c):
    """angulararea.py:74-82 _fallof_curve restated in numpy: the selects on the f32 cosine against the f32 constants, the
    transition (cutoff - acos(cos_theta)) * inv_transition in f64 (math.acos: np.arccos may round 1 ulp apart, which the
    57,000 of inv_transition at (30, 29.999) degrees would scale to 6e-12)"""
    c = np.asarray(c, np.float32)
    acos = np.frompyfunc(math.acos, 1, 1)(c.astype(np.float64)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        trans = (np.float64(e.cutoff) - acos) * np.float64(e.inv_transition)
    beam = np.where(c >= np.float32(e.cos_beam), 1.0, trans)
    return np.where(c > np.float32(e.cos_cutoff), beam, 0.0)


def _around(x, k=64):
    i = np.array(x, np.float32).view(np.int32)
    if i < 0:                                   # negative floats: step the magnitude
        return -_around(-np.float32(x), k)
    return np.arange(i - k, i + k + 1, dtype=np.int32).view(np.float32)


def _inputs(e):
    ends = np.array([1.0, -1.0, 0.0, -0.0], np.float32)
    sweep = np.linspace(-1, 1, 400_001, dtype=np.float32)
    x = np.concatenate([_around(e.cos_cutoff), _around(e.cos_beam), ends, sweep])
    return x[(x >= -1) & (x <= 1)].astype(np.float32)


def _ordered(x):
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _near(e, c):
    """oracle/mtr_oracle.c ang_is_near: the cosine within 4 ulps of cos_cutoff or cos_beam, or the f64 cutoff - acos(c) within 4
    ulps of cutoff of 0"""
    oc = _ordered(c)
    gap = np.float64(e.cutoff) - np.arccos(np.asarray(c, np.float64))
    ulp = float(np.spacing(np.float32(e.cutoff)))
    return (np.abs(oc - _ordered(e.cos_cutoff)) <= 4) | (np.abs(oc - _ordered(e.cos_beam)) <= 4) | (np.abs(gap) <= 4 * ulp)


def _hh_falloff(host_harness, e, c):
    c = np.ascontiguousarray(c, np.float32)
    y = np.empty_like(c)
    fp = C.POINTER(C.c_float)
    host_harness.hh_angular_falloff.argtypes = [C.c_void_p, C.c_uint64, fp, fp]
    host_harness.hh_angular_falloff(C.addressof(e), c.size, c.ctypes.data_as(fp), y.ctypes.data_as(fp))
    return y


@pytest.mark.parametrize("cutoff,beam", PAIRS)
def test_oracle_falloff_matches_numpy(oracle, cutoff, beam):
    e = _emitter(cutoff, beam)
    c = _inputs(e)
    got, ref = oracle.angular_falloff(e, c), _numpy_falloff(e, c)
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref).max() <= 1e-12
    assert np.all((got == 0) == (ref == 0)) and np.all((got == 1) == (ref == 1))


# the measured maximum of |f32 - f64| over the inputs of _inputs, per pair (the bound below is what is asserted)
# (in units of the bound: 0.23, 0, 0.18, 0.18, 0.28, 0.18, 0.24)
MEASURED = {(35, 20): 2.48e-7, (10, 10): 0.0, (60, 30): 1.85e-7, (90, 0): 1.02e-7, (180, 120): 3.01e-7, (2, 1): 1.90e-7,
            (30, 29.999): 2.48e-3}


@pytest.mark.parametrize("cutoff,beam", PAIRS)
def test_product_falloff_against_f64(oracle, host_harness, cutoff, beam):
    """mtr_core.h angular_falloff (f32, acos_f32) against the oracle's f64 falloff: every f32 within 64 ulps of cos_cutoff and of
    cos_beam, +-1, +-0 and a dense sweep of [-1, 1].  |f32 - f64| <= 4e-7 + inv_transition * (2 ulp of the acos, bounded by
    test_acos_polynomial_against_f64, + 1 ulp of cutoff for the difference); no NaN / Inf, the infinite transition included; the
    sign of `falloff > 0` agrees except at near points (oracle/mtr_oracle.c ang_is_near).  Measured maxima: MEASURED."""
    e = _emitter(cutoff, beam)
    c = _inputs(e)
    f32 = _hh_falloff(host_harness, e, c).astype(np.float64)
    f64 = oracle.angular_falloff(e, c)
    assert np.all(np.isfinite(f32)) and np.all(np.isfinite(f64))
    acos = np.arccos(c.astype(np.float64))
    inv_t = float(e.inv_transition) if math.isfinite(e.inv_transition) else 0.0
    bound = 4e-7 + inv_t * (2.0 * np.spacing(acos.astype(np.float32)).astype(np.float64) + float(np.spacing(np.float32(e.cutoff))))
    err = np.abs(f32 - f64)
    print(f"({cutoff}, {beam}): max |f32 - f64| = {err.max():.3e}, max err / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), (float(err.max()), float((err / bound).max()))
    assert err.max() <= 1.5 * MEASURED[(cutoff, beam)] + 1e-9
    near = _near(e, c)
    assert np.all(((f32 > 0) == (f64 > 0)) | near)
    assert near.sum() <= 300                      # the band is a few ulps wide: <= 2 x 129 points around the thresholds + a few
    # the selects are exact comparisons of the f32 cosine with the stored constants
    assert np.all(f32[c >= e.cos_beam] == (c[c >= e.cos_beam] > e.cos_cutoff))
    assert np.all(f32[c <= e.cos_cutoff] == 0.0)


@pytest.mark.parametrize("case", ["notebook_view1", "cornell_60_30", "cube_40_20"])
def test_oracle_does_not_treat_angular_as_area(tmp_path, case):
    """the oracle's render of an angular scene differs from its render of the same scene with `angular` forced to 0 — the
    silent fallback to an area light — and the host build of the product matches the angular one (the next test)"""
    build, seed, spp, _ = AC.SCENE_CASES[case]
    scene = build(str(tmp_path))
    s_ang, t_ang, _, _, _ = AC.oracle_render(scene, seed, spp)
    s_area, t_area, _, _, n_area = AC.oracle_render(scene, seed, spp, sd=AC.as_area(scene.data()))
    assert n_area == 0
    assert rel_l2(t_ang, t_area) > 0.05 and rel_l2(s_ang, s_area) > 0.05


# near totals the oracle reported for these scenes at these seeds and sample counts (ang_is_near evaluations)
NEAR_MAX = 64


@pytest.mark.parametrize("case", list(AC.SCENE_CASES))
def test_host_build_matches_oracle(host_harness, tmp_path, case):
    """the host build of mtr_core.h against the oracle scene by scene: rel-L2 <= 1e-5 transient and steady outside the near pixels,
    counters equal up to the near total; the cone clips each image (wide cones: the render differs from the area light's)"""
    build, seed, spp, wide = AC.SCENE_CASES[case]
    scene = build(str(tmp_path))
    assert any(scene.data().emitters[i].angular for i in range(scene.data().n_emitters))
    s, t, c = AC.hh_render_developed(host_harness, scene, seed, spp)
    n_near = AC.assert_matches_oracle(s, t, c, AC.oracle_render(scene, seed, spp), case)
    print(f"{case}: near total {n_near}")
    assert n_near <= NEAR_MAX, n_near
    AC.assert_cone_clips(scene, seed, wide=wide)


def test_oracle_refuses_angular_in_polarized_and_nlos(oracle):
    """the restatement covers the transient path loop only: a polarized render of an angular scene is an error, not an area light"""
    scene = AC.cornell(60, 30, res=4)
    p = scene.integrator().render_params(scene.sensors()[0].film(), 0, 1)
    with pytest.raises(RuntimeError):
        oracle.render_polarized(scene.data(), p)
