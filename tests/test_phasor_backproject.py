"""nlos.phasor_backproject on the CPU: the host build of mtr_phasor_backproject.h (tests/host_phasor_backproject.cpp) against an
independent numpy f64 restatement in both forms (table, and the 16-anchor recurrence of a uniform table), the numpy f32
restatement against the bar on its own, exact one-term checks, the focus on a point source, the window, the end-to-end check of
the NLOS tier in the frequency domain (render a quad at z = 1 with the oracle into a phasor film, reconstruct, the depth profile of
|V| peaks at z = 1), the additive C-ABI, capture_geometry on a phasor-film scene and the refusals that need no GPU."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import phasor_backproject_cases as pc
from phasor_backproject_cases import (CONFOCAL, E2E, E2E_BOX, E2E_SPP, EXHAUSTIVE, FLT_MAX, PARITY, PB_TOL, SINGLE, SLICES, depth_peak,
                                      host_phasor_backproject, make_case, parity_case, reference, reference_f32, rel_l2, tiny_case,
                                      wall_points, with_form)

ROOT = pc.ROOT


@functools.lru_cache(maxsize=None)
def parity_reference(kind, offsets, F, weights):
    """the f64 volume of a parity case (the form does not enter it), computed once"""
    ref = reference(parity_case(kind, offsets, F, weights))
    ref.setflags(write=False)
    return ref


@pytest.fixture
def mono_after():
    """conftest.make_nlos selects llvm_ad_rgb; a phasor film renders in a mono variant — switch, and back here"""
    import mitransient_amd.mi as mi

    def switch():
        mi.set_variant("llvm_ad_mono")
    try:
        yield switch
    finally:
        mi.set_variant("llvm_ad_rgb")


# ---------------------------------------------------------------- the host build against numpy f64
@pytest.mark.parametrize("kind,offsets,F,weights", PARITY)
def test_host_build_matches_f64(kind, offsets, F, weights):
    ref = parity_reference(kind, offsets, F, weights)
    assert np.abs(ref).max() > 0
    got = {}
    for form in ("uniform", "table"):
        case = parity_case(kind, offsets, F, weights, form)
        assert (case["freq_step"] > 0) == (form == "uniform")          # the film's tables are uniformly spaced
        got[form] = host_phasor_backproject(case)
        e = rel_l2(got[form], ref)
        print(f"{kind} offsets={offsets} F={F} weights={weights} {form}: rel-L2 {e:.3e}")
        assert e <= PB_TOL, e
    e = rel_l2(got["uniform"], got["table"])
    print(f"uniform form against table form: rel-L2 {e:.3e}")
    assert e <= PB_TOL, e


def test_f32_restatement_is_within_the_bar():
    """the tolerance holds for the reference alone: numpy in f32 (the header's operation order, both forms) against f64"""
    worst = 0.0
    for kind, offsets, F, weights in PARITY:
        for form in ("uniform", "table"):
            e = rel_l2(reference_f32(parity_case(kind, offsets, F, weights, form)), parity_reference(kind, offsets, F, weights))
            worst = max(worst, e)
            assert e <= PB_TOL, (kind, offsets, F, weights, form, e)
    print(f"worst rel-L2 of the f32 restatement: {worst:.3e}")
    assert worst <= 5e-5                        # (what the bar was derived from: 2.4e-5 at F = 151)


@pytest.mark.parametrize("F", SLICES)
@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_anchor_block_edges(kind, F):
    """F = 1 (the per-term form whatever is asked), one whole block, one block and one frequency"""
    for weights in (None, np.linspace(0.5, 1.5, F)):
        case = tiny_case(kind, F=F, offsets=True, weights=weights)
        assert (case["freq_step"] > 0) == (F > 1)
        ref = reference(case)
        assert np.abs(ref).max() > 0
        table = host_phasor_backproject(with_form(case, "table"))
        got = host_phasor_backproject(case)
        assert rel_l2(got, ref) <= PB_TOL and rel_l2(table, ref) <= PB_TOL and rel_l2(got, table) <= PB_TOL
        assert rel_l2(reference_f32(case), ref) <= PB_TOL
        if F == 1:
            assert np.array_equal(got, table)


def test_host_build_is_deterministic():
    case = parity_case(EXHAUSTIVE, True, 151, "gaussian")
    assert np.array_equal(host_phasor_backproject(case), host_phasor_backproject(case))


# ---------------------------------------------------------------- uniform or table: the Python rule
def test_frequency_table_classification():
    from mitransient_amd.nlos import uniform_frequency_step
    for F in (15, 28, 151, 16, 17):
        f, film = pc.table(F)
        step = uniform_frequency_step(f)
        assert step > 0 and abs(step - 1.0 / (film["temporal_bins"] * film["bin_width_opl"])) <= 1e-6 * step
        assert uniform_frequency_step(np.delete(f, len(f) // 2)) == 0.0          # one frequency removed: a gap
        assert uniform_frequency_step(f[::-1]) == 0.0                              # descending: step <= 0
    assert uniform_frequency_step(pc.table(1)[0]) == 0.0
    assert uniform_frequency_step([2.0, 2.0, 2.0]) == 0.0
    assert uniform_frequency_step([1.0, 2.0, 3.0 + 1e-5]) == 0.0                  # 40 ulps of 3.0 off the line
    assert uniform_frequency_step([1.0, 2.0, float(np.nextafter(np.float32(3.0), np.float32(4.0)))]) > 0      # 1 ulp: within the rule
    # a table the rule does not find uniform runs in the table form whatever is asked
    f = np.delete(pc.table(28)[0], 5)
    case = tiny_case(CONFOCAL, freq=f)
    assert case["freq_step"] == 0 and rel_l2(host_phasor_backproject(case), reference(case)) <= PB_TOL


# ---------------------------------------------------------------- exact checks
def one_term(freq, phasor):
    """one scan point at the origin, one voxel on its normal at z = 0.5, start_opl 0: tau = 1"""
    p = np.zeros((1, 3), np.float32)
    return make_case(CONFOCAL, p, p, start=0.0, vmin=(-0.5, -0.5, 0.0), vmax=(0.5, 0.5, 1.0), res=(1, 1, 1), freq=[freq],
                     phasors=np.asarray(phasor, np.float32).reshape(1, 1, 2))


@pytest.mark.parametrize("freq", [1.0, 1.37])
def test_one_term(freq):
    assert np.array_equal(pc.taus(one_term(freq, (1, 0)), np.float32), [[1.0]])
    v = host_phasor_backproject(one_term(freq, (1.0, 0.0)))[0, 0, 0]
    assert abs(v - np.exp(2j * np.pi * float(np.float32(freq)))) <= PB_TOL, v         # f = 1: V = 1 + 0i
    # P = the film's own term at tau: V = |P|^2 = 1, zero phase
    c, s = pc.host_phasor_term(freq, 1.0)
    v = host_phasor_backproject(one_term(freq, (c, s)))[0, 0, 0]
    assert abs(abs(v) - 1.0) <= PB_TOL and abs(np.angle(v)) <= PB_TOL, v


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_point_source_focus(kind):
    """the phasors of a unit scatterer at POINT: at a voxel whose centre is the point every term has phase 0 and |V| = pairs x F, the
    bound of every voxel (|term| = 1).  Voxels of 0.1 with POINT at the centre of voxel (3, 3, 3)"""
    g = pc.bc.tiny_case(kind)
    x, y, z = pc.POINT
    for offsets in (False, True):
        for form in ("uniform", "table"):
            case = make_case(kind, g["sp"], g["lp"], F=28, offsets=offsets, phasors="point", form=form,
                             vmin=(x - 0.35, y - 0.35, z - 0.35), vmax=(x + 0.35, y + 0.35, z + 0.35), res=(7, 7, 7))
            vol = host_phasor_backproject(case)
            assert pc.brightest(vol) == (3, 3, 3)
            rows = case["phasors"].shape[0]
            assert abs(abs(vol[3, 3, 3]) / (rows * 28) - 1.0) <= PB_TOL
            assert np.sort(np.abs(vol).ravel())[-2] < 0.9 * abs(vol[3, 3, 3])


# ---------------------------------------------------------------- the window
def test_boxes_beyond_the_window_give_exact_zeros():
    film = pc.FILMS[28]
    capture = (np.float32(0.0), np.float32(film["temporal_bins"] * film["bin_width_opl"]))      # window="capture"
    for kind in (CONFOCAL, SINGLE, EXHAUSTIVE):
        for form in ("uniform", "table"):
            case = tiny_case(kind, form=form, window=capture, vmin=(100, 100, 100), vmax=(102, 102, 101))
            assert np.array_equal(host_phasor_backproject(case), np.zeros((6, 6, 6)))
            # ... and so far that the path length overflows, with the default window
            case = tiny_case(kind, form=form, vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
            assert case["tau_min"] == -FLT_MAX and case["tau_max"] == FLT_MAX
            assert np.array_equal(host_phasor_backproject(case), np.zeros((6, 6, 6)))


WINDOW_CUT = dict(window=(np.float32(0.5), np.float32(1.5)), start=1.85)


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_window_that_cuts_through_the_box(kind):
    for form in ("uniform", "table"):
        case = tiny_case(kind, offsets=False, weights="gaussian", form=form, **WINDOW_CUT)
        # the precondition of a comparison across precisions: f32 and f64 agree on the membership of every (voxel, pair)
        m32, m64 = pc.in_window(case, np.float32), pc.in_window(case, np.float64)
        assert np.array_equal(m32, m64)
        assert 0.2 < m64.mean() < 0.8
        ref = reference(case)
        assert np.abs(ref).max() > 0
        assert rel_l2(host_phasor_backproject(case), ref) <= PB_TOL
        assert rel_l2(host_phasor_backproject(case), host_phasor_backproject(tiny_case(kind, weights="gaussian", form=form))) > 0.1


# ---------------------------------------------------------------- refusals
def bad_descriptions():
    good = tiny_case(CONFOCAL)
    bad = []
    for key, value in (("F", 0), ("S", 0), ("L", 0), ("res", (6, 0, 6)), ("vmax", np.array([1, -1, 1.5], np.float32)),
                       ("vmax", np.array([1, 1, 0.25], np.float32)), ("capture_type", 7), ("start", np.float32(np.inf)),
                       ("start", np.float32(np.nan)), ("tau_min", np.float32(np.nan)), ("tau_max", np.float32(np.nan)),
                       ("tau_min", np.float32(2.0)), ("freq_step", np.float32(-0.1)), ("freq_step", np.float32(np.nan))):
        c = dict(good)
        c[key] = value
        if key == "tau_min" and value == 2.0:
            c["tau_max"] = np.float32(1.0)
        bad.append(c)
    c = dict(good); c["L"] = 63; bad.append(c)                            # Confocal: L != S
    c = dict(tiny_case(SINGLE)); c["L"] = 2; bad.append(c)                # Single: L != 1
    return good, bad


def test_invalid_descriptions_leave_the_volume_untouched():
    good, bad = bad_descriptions()
    lib = pc.host_lib()
    for c in bad:
        vol = host_phasor_backproject(c, expect=-1, fill=7.0)
        assert np.all(vol == 7.0)
    # hb_check names the reason; NULL pointers (weights alone may be NULL)
    vol = np.full((6, 6, 6, 2), 7.0, np.float32)
    ptrs = [good[k].ctypes.data for k in ("sp", "lp", "so", "lo", "freq")]
    ph, out = C.c_void_p(good["phasors"].ctypes.data), C.c_void_p(vol.ctypes.data)
    d = pc.desc_of(good, *ptrs, None)
    assert lib.hb_check(C.byref(d), ph, out) == b""
    for k in range(5):
        broken = list(ptrs)
        broken[k] = None
        d = pc.desc_of(good, *broken, None)
        assert b"NULL" in lib.hb_check(C.byref(d), ph, out)
        assert lib.hpb_backproject(C.byref(d), ph, out) == -1
    d = pc.desc_of(good, *ptrs, None)
    assert lib.hpb_backproject(C.byref(d), None, out) == -1 and lib.hpb_backproject(C.byref(d), ph, None) == -1
    assert lib.hpb_backproject(None, ph, out) == -1
    d.tau_min, d.tau_max = 2.0, 1.0
    assert b"tau_min" in lib.hb_check(C.byref(d), ph, out)
    d = pc.desc_of(good, *ptrs, None)
    d.freq_step = -1.0
    assert b"freq_step" in lib.hb_check(C.byref(d), ph, out)
    assert np.all(vol == 7.0)


def test_phasor_backproject_validates_before_touching_the_gpu(mono_after):
    import mitransient_amd as mitr
    from mitransient_amd.nlos import CaptureGeometry, phasor_backproject
    sp = wall_points(4, 2).astype(np.float64)
    g = CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16)
    gx = CaptureGeometry(EXHAUSTIVE, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16)
    box = ((-1, -1, 0.5), (1, 1, 1.5), 4)
    f = [1.0, 1.5, 2.0]
    ok = np.zeros((2, 4, 3, 2), np.float32)
    for phasors, geom, freq, args, kw in (
            (np.zeros((2, 4, 4, 2), np.float32), g, f, box, {}),                          # frequency count
            (np.zeros((2, 4, 4), np.complex64), g, f, box, {}),
            (np.zeros((4, 2, 3, 2), np.float32), g, f, box, {}),                          # scan size
            (np.zeros((2, 4, 3), np.float32), g, f, box, {}),                             # real without a (Re, Im) axis
            (np.zeros((2, 4, 3, 3), np.float32), g, f, box, {}),
            (np.zeros((2, 4, 2, 2, 3, 2), np.float32), g, f, box, {}),                    # an exhaustive tensor for a confocal geometry
            (ok, gx, f, box, {}),                                                         # ... and the reverse
            (np.zeros((2, 4, 3, 2, 3, 2), np.float32), gx, f, box, {}),                   # 6 != 8 lasers
            (ok, g, [], box, {}),
            (ok, g, [1.0, np.nan, 2.0], box, {}),
            (ok, g, f, ((-1, -1, 0.5), (1, 1, 0.5), 4), {}),                              # empty box
            (ok, g, f, ((-1, -1, 0.5), (1, 1, 1.5), 0), {}),                              # resolution
            (ok, g, f, ((-1, -1, 0.5), (1, 1, 1.5), (4, 4)), {}),
            (ok, g, f, box, {"weights": [1.0, 1.0]}),
            (ok, g, f, box, {"weights": "gaussian"}),                                     # needs a film
            (ok, g, f, box, {"weights": "hann"}),
            (ok, g, f, box, {"window": (2.0, 1.0)}),
            (ok, g, f, box, {"window": (np.nan, 1.0)}),
            (ok, g, f, box, {"window": "film"}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.0, 0), f, box, {"window": "capture"}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), np.inf, 0.04, 16), f, box, {}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3)[:7], np.zeros((2, 4)), np.zeros(7), 1.2, 0.04, 16), f, box, {}),
            (ok, CaptureGeometry(SINGLE, sp, sp.reshape(-1, 3)[:2], np.zeros((2, 4)), np.zeros(2), 1.2, 0.04, 16), f, box, {}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 3)), np.zeros(8), 1.2, 0.04, 16), f, box, {}),
            (ok, "geometry", f, box, {})):
        with pytest.raises(ValueError, match="phasor_backproject"):
            phasor_backproject(phasors, geom, freq, *args, **kw)
    assert mitr.nlos.phasor_backproject is phasor_backproject
    import torch
    if not torch.cuda.is_available():           # a valid call without a GPU: the product has no CPU path
        from mitransient_amd._cabi import MitransientAMDError
        with pytest.raises(MitransientAMDError):
            phasor_backproject(ok, g, f, *box)


# ---------------------------------------------------------------- capture_geometry on a phasor-film scene
@pytest.mark.parametrize("capture", ["single", "confocal"])
def test_capture_geometry_of_a_phasor_film_scene(mono_after, capture):
    import mitransient_amd as mitr
    from conftest import make_nlos
    film = dict(pc.E2E_FILM)
    scene = make_nlos(sx=4, sy=2, capture=capture, start=1.7, account_first_and_last_bounces=True, film=film)
    ref = make_nlos(sx=4, sy=2, capture=capture, start=1.7, account_first_and_last_bounces=True, bins=256, bin_width=0.02)
    mono_after()
    assert isinstance(scene.sensors()[0].film(), mitr.PhasorHDRFilm)
    g, want = mitr.nlos.capture_geometry(scene), mitr.nlos.capture_geometry(ref)
    assert g.capture_type == (SINGLE if capture == "single" else CONFOCAL) and g.sensor_points.shape == (2, 4, 3)
    for k in ("sensor_points", "laser_points", "sensor_offset", "laser_offset"):
        assert np.array_equal(getattr(g, k), getattr(want, k))
    assert g.sensor_offset.any() and g.laser_offset.any()
    assert (g.start_opl, g.bin_width_opl, g.temporal_bins) == (1.7, 0.02, 256)


# ---------------------------------------------------------------- end to end: oracle render -> host reconstruction
@pytest.mark.parametrize("name", sorted(E2E))
def test_rendered_quad_reconstructs_at_its_depth(oracle, mono_after, name):
    import mitransient_amd as mitr
    scene = pc.e2e_scene(name)
    mono_after()
    film = scene.sensors()[0].film()
    sd = scene.data()
    p = scene.integrator().render_params(film, 0, E2E_SPP)
    raw, s4, _ = oracle.render(sd, p)
    ph, _ = oracle.develop(sd.film, raw, s4)
    assert ph.shape == (16, 16, 28, 2) and np.count_nonzero(ph) > 0
    g = mitr.nlos.capture_geometry(scene)
    for weights in (None, "gaussian"):
        case = make_case(g.capture_type, g.sensor_points, g.laser_points, F=28, start=g.start_opl, vmin=E2E_BOX[0], vmax=E2E_BOX[1],
                         res=(E2E_BOX[2],) * 3, phasors=ph.reshape(256, 28, 2), weights=weights)
        assert np.array_equal(case["freq"], film.frequencies_f32) and case["freq_step"] > 0
        case["so"] = g.sensor_offset.reshape(-1).astype(np.float32)
        case["lo"] = g.laser_offset.astype(np.float32)
        z, prof = depth_peak(host_phasor_backproject(case))
        print(name, weights, "depth profile of |V| peaks at z =", z, "neighbours / peak", prof[7:10] / prof.max())
        assert prof.max() > 0 and abs(z - 1.0) <= 1.0 / 16.0, (z, prof)


# ---------------------------------------------------------------- the additive C-ABI
def test_abi_is_additive():
    from mitransient_amd import _cabi
    assert _cabi.MTR_ABI_VERSION == 24
    assert "mtr_phasor_backproject" in _cabi.EXPORTS
    lib = C.CDLL(_cabi.LIB_PATH)
    assert hasattr(lib, "mtr_phasor_backproject")
    lib.mtr_abi_version.restype = C.c_int
    assert lib.mtr_abi_version() == 24
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mitransient_amd.h"\nint main(){printf("%zu %zu %zu %d\\n", '
            "sizeof(mtr_phasor_backproject_desc), offsetof(mtr_phasor_backproject_desc, sensor_points), "
            "offsetof(mtr_phasor_backproject_desc, weights), MTR_ABI_VERSION);return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, first, last, version = (int(x) for x in subprocess.check_output([exe]).split())
    d = _cabi.mtr_phasor_backproject_desc
    assert (C.sizeof(d), d.sensor_points.offset, d.weights.offset, version) == (size, first, last, 24)
