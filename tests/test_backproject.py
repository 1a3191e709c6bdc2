"""nlos.backproject on the CPU: the host build of mtr_backproject.h (tests/host_backproject.cpp) against an independent numpy
f64 restatement, its edges, capture_geometry, the end-to-end check of the NLOS tier (render a quad at z = 1 with the oracle,
backproject, the depth profile peaks at z = 1), the additive C-ABI, laplacian_filter and the refusals that need no GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from backproject_cases import (CONFOCAL, E2E, E2E_BOX, E2E_SPP, EXHAUSTIVE, SINGLE, TINY, TOL, bin_disagreements, depth_peak,
                               e2e_scene, host_backproject, host_lib, make_case, positions, reference, tiny_case, wall_points)
from conftest import make_nlos, make_nlos_camera, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the host build against numpy f64
@pytest.mark.parametrize("kind,interpolation,offsets", TINY)
def test_host_build_matches_f64(kind, interpolation, offsets):
    for capture in ("smooth", "spiky"):
        case = tiny_case(kind, interpolation, offsets, capture)
        if interpolation == "nearest":
            # the precondition of a `nearest` comparison across precisions: f32 and f64 pick the same bin everywhere
            assert bin_disagreements(case) == 0
        ref = reference(case)
        assert np.abs(ref).max() > 0
        e = rel_l2(host_backproject(case), ref)
        print(f"{kind} {interpolation} offsets={offsets} {capture}: rel-L2 {e:.3e}")
        assert e <= TOL, e


def test_f32_restatement_is_within_the_bar():
    """the tolerance holds for the reference alone: numpy in f32 (mtr_backproject.h's operation order) against f64"""
    for kind, interpolation, offsets in TINY:
        for capture in ("smooth", "spiky"):
            case = tiny_case(kind, interpolation, offsets, capture)
            assert rel_l2(reference(case, np.float32), reference(case)) <= TOL


def test_host_build_is_deterministic():
    case = tiny_case(EXHAUSTIVE, "linear", True, "spiky")
    assert np.array_equal(host_backproject(case), host_backproject(case))


# ---------------------------------------------------------------- edges
def test_far_box_gives_exact_zeros():
    for interpolation in ("nearest", "linear"):
        case = tiny_case(CONFOCAL, interpolation, vmin=(100, 100, 100), vmax=(102, 102, 101))
        assert np.array_equal(host_backproject(case), np.zeros((6, 6, 6), np.float32))
    # ... and so far that the path length overflows to inf
    case = tiny_case(SINGLE, "linear", vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
    assert np.array_equal(host_backproject(case), np.zeros((6, 6, 6), np.float32))


@pytest.mark.parametrize("interpolation", ["nearest", "linear"])
def test_one_bin(interpolation):
    case = tiny_case(CONFOCAL, interpolation, T=1, start=1.0, bin_width=6.0, capture="spiky")      # paths span 1.17 .. 6.5
    ref = reference(case)
    assert np.abs(ref).max() > 0
    assert rel_l2(host_backproject(case), ref) <= TOL
    if interpolation == "nearest":          # every path of this geometry lies in the one bin: each voxel is the sum of the rows
        assert np.allclose(host_backproject(case), case["capture"].sum(), rtol=1e-5)


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_one_scan_point(kind):
    sp = np.array([[0.25, -0.25, 0.0]], np.float32)
    lp = sp if kind == CONFOCAL else np.array([[0.0, 0.5, 0.0]], np.float32)
    for interpolation in ("nearest", "linear"):
        case = make_case(kind, sp, lp, interpolation=interpolation, capture="spiky")
        assert bin_disagreements(case) == 0
        ref = reference(case)
        assert np.abs(ref).max() > 0
        assert rel_l2(host_backproject(case), ref) <= TOL


def test_voxel_on_a_scan_point():
    """8 x 8 x 1 voxels whose centres ARE the scan points (path length 0 for the voxel's own point, read from bin 0)"""
    sp = wall_points(8, 8)
    cap = np.random.default_rng(3).random((64, 64)).astype(np.float32)
    for interpolation in ("nearest", "linear"):
        case = make_case(CONFOCAL, sp, sp, start=0.0, bin_width=0.125, vmin=(-1, -1, -0.125), vmax=(1, 1, 0.125), res=(8, 8, 1),
                         interpolation=interpolation, capture=cap)
        assert interpolation == "linear" or bin_disagreements(case) == 0
        vol = host_backproject(case)
        assert np.all(np.isfinite(vol))
        assert rel_l2(vol, reference(case)) <= TOL
    # nearest, one scan point and its own voxel: exactly the first bin
    one = make_case(CONFOCAL, sp[3:4, 5:6], sp[3:4, 5:6], start=0.0, bin_width=0.125, vmin=(-1, -1, -0.125), vmax=(1, 1, 0.125),
                    res=(8, 8, 1), capture=cap[:1])
    assert host_backproject(one)[0, 3, 5] == cap[0, 0]


def test_linear_taps_at_minus_one_and_T():
    """one scan point at the origin, one voxel on its normal at height z: d = 2 z, bins of 1 from 0, T = 4 — exact arithmetic"""
    H = np.array([[8.0, 2.0, 4.0, 16.0]], np.float32)
    p = np.zeros((1, 3), np.float32)

    def at(z):
        case = make_case(CONFOCAL, p, p, T=4, start=0.0, bin_width=1.0, vmin=(-0.5, -0.5, z - 0.5), vmax=(0.5, 0.5, z + 0.5),
                         res=(1, 1, 1), interpolation="linear", capture=H)
        return float(host_backproject(case)[0, 0, 0])
    assert at(0.125) == 0.75 * 8.0              # u' = -0.25: taps -1 (outside: 0) and 0
    assert at(0.5) == 0.5 * 8.0 + 0.5 * 2.0     # u' = 0.5: taps 0 and 1
    assert at(2.125) == 0.25 * 16.0             # u' = 3.75: taps 3 and T (outside: 0)
    assert at(2.25) == 0.0                      # u' = 4: both outside
    assert at(2.0 ** -10) == 0.5 * 8.0 + 2.0 ** -9 * 8.0     # u' just above -0.5


def test_window_after_the_first_arrivals():
    for interpolation in ("nearest", "linear"):
        case = tiny_case(CONFOCAL, interpolation, capture="spiky", start=2.6)
        if interpolation == "nearest":
            assert bin_disagreements(case) == 0
        u = positions(case, np.float64)
        assert 0.2 < np.mean(u < 0) < 0.8                                      # a good share of the paths arrive before the window
        ref = reference(case)
        assert np.abs(ref).max() > 0
        assert rel_l2(host_backproject(case), ref) <= TOL


def test_invalid_descriptions_leave_the_volume_untouched():
    good = tiny_case(CONFOCAL)
    assert host_lib().hb_check is not None
    bad = []
    for key, value in (("T", 0), ("S", 0), ("L", 0), ("bin_width", np.float32(0.0)), ("bin_width", np.float32(-0.04)),
                       ("bin_width", np.float32(np.nan)), ("res", (6, 0, 6)), ("vmax", np.array([1, -1, 1.5], np.float32)),
                       ("vmax", np.array([1, 1, 0.25], np.float32)), ("capture_type", 7)):
        c = dict(good)
        c[key] = value
        bad.append(c)
    c = dict(good); c["L"] = 63; bad.append(c)                            # Confocal: L != S
    c = dict(tiny_case(SINGLE)); c["L"] = 2; bad.append(c)                # Single: L != 1
    for c in bad:
        vol = host_backproject(c, expect=-1, fill=7.0)
        assert np.all(vol == 7.0)


def test_plan_splits_pairs_only_when_voxels_are_few():
    lib = host_lib()
    out = (C.c_uint64 * 3)()
    lib.hb_plan.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    assert lib.hb_plan(6, 6, 6, 64, 256, out) == 1 and list(out) == [2, 1, 64]              # 64 pairs: one slab
    assert lib.hb_plan(2, 2, 2, 1024, 256, out) == 1 and list(out) == [1, 16, 64]           # few voxels, many pairs: slabs of >= 64
    assert lib.hb_plan(128, 128, 128, 65536, 256, out) == 1 and list(out) == [8192, 1, 65536]
    assert lib.hb_plan(5, 3, 7, 1000, 256, out) == 1 and out[0] == 2 and out[1] * out[2] >= 1000 > (out[1] - 1) * out[2]
    assert lib.hb_plan(0, 1, 1, 1, 256, out) == 0


# ---------------------------------------------------------------- capture_geometry
@pytest.mark.parametrize("capture", ["single", "confocal"])
@pytest.mark.parametrize("first_last", [False, True])
def test_capture_geometry(capture, first_last):
    import mitransient_amd as mitr
    scene = make_nlos(sx=4, sy=2, capture=capture, account_first_and_last_bounces=first_last)
    relay = [s for s in scene.shapes() if s.sensor() is not None][0]
    mitr.nlos.focus_emitter_at_relay_wall_uv((0.75, 0.25), relay, scene.emitters()[0])
    g = mitr.nlos.capture_geometry(scene)
    assert g.capture_type == (SINGLE if capture == "single" else CONFOCAL)
    assert g.sensor_points.shape == (2, 4, 3)
    want = np.array([[[-0.75 + 0.5 * x, -0.5 + y, 0.0] for x in range(4)] for y in range(2)])
    assert np.allclose(g.sensor_points, want, atol=1e-12)
    if capture == "single":
        assert g.laser_points.shape == (1, 3) and np.allclose(g.laser_points[0], [0.5, -0.5, 0.0], atol=1e-12)
    else:
        assert np.array_equal(g.laser_points, g.sensor_points.reshape(-1, 3))
    o = np.array([-0.5, 0.0, 0.25])
    if first_last:
        assert np.allclose(g.sensor_offset, np.linalg.norm(o - want, axis=-1), atol=1e-12)
        assert np.allclose(g.laser_offset, np.linalg.norm(o - g.laser_points, axis=-1), atol=1e-12)
    else:
        assert not g.sensor_offset.any() and not g.laser_offset.any()
    assert g.sensor_offset.shape == (2, 4) and g.laser_offset.shape == (len(g.laser_points),)
    assert (g.start_opl, g.bin_width_opl, g.temporal_bins) == (1.85, 0.03, 64)


def test_capture_geometry_exhaustive_equal_grids():
    import mitransient_amd as mitr
    from test_nlos import exhaustive_scene
    scene = exhaustive_scene(sx=3, sy=2, lw=3, lh=2)
    g = mitr.nlos.capture_geometry(scene)
    assert g.capture_type == EXHAUSTIVE and g.laser_grid == (3, 2) and g.laser_points.shape == (6, 3)
    for i in range(6):                          # point i = sensor point (i // W, i % W)
        assert np.array_equal(g.laser_points[i], g.sensor_points[i // 3, i % 3])


def test_capture_geometry_refusals():
    import mitransient_amd as mitr
    from test_nlos import exhaustive_scene
    with pytest.raises(ValueError, match="perspective camera"):
        mitr.nlos.capture_geometry(make_nlos_camera())
    with pytest.raises(ValueError, match="force_equal_illumination_scanning"):
        mitr.nlos.capture_geometry(exhaustive_scene(sx=4, sy=3, lw=3, lh=2, equal=False))
    scene = make_nlos(sx=1, sy=1, capture="single", sensor_extra={"original_film_width": 8, "original_film_height": 8})
    with pytest.raises(ValueError, match="is_confocal"):
        mitr.nlos.capture_geometry(scene)


# ---------------------------------------------------------------- end to end: oracle render -> host backprojection
@pytest.mark.parametrize("name", sorted(E2E))
def test_rendered_quad_backprojects_to_its_depth(oracle, name):
    import mitransient_amd as mitr
    scene = e2e_scene(name)
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), 0, E2E_SPP)
    t4, s4, _ = oracle.render(sd, p)
    t3, _ = oracle.develop(sd.film, t4, s4)
    assert t3.shape == (16, 16, 128, 3)
    g = mitr.nlos.capture_geometry(scene)
    case = make_case(g.capture_type, g.sensor_points, g.laser_points, T=g.temporal_bins, start=g.start_opl, bin_width=g.bin_width_opl,
                     vmin=E2E_BOX[0], vmax=E2E_BOX[1], res=(E2E_BOX[2],) * 3, capture=t3.mean(axis=-1).reshape(256, 128))
    case["so"] = g.sensor_offset.reshape(-1).astype(np.float32)
    case["lo"] = g.laser_offset.astype(np.float32)
    z, prof = depth_peak(host_backproject(case))
    print(name, "depth profile peaks at z =", z)
    assert prof.max() > 0 and abs(z - 1.0) <= 1.0 / 16.0, (z, prof)


# ---------------------------------------------------------------- the additive C-ABI
def test_abi_is_additive():
    from mitransient_amd import _cabi
    assert _cabi.MTR_ABI_VERSION == 24
    assert "mtr_backproject" in _cabi.EXPORTS
    lib = C.CDLL(_cabi.LIB_PATH)
    assert hasattr(lib, "mtr_backproject")
    lib.mtr_abi_version.restype = C.c_int
    assert lib.mtr_abi_version() == 24
    prog = ('#include <stdio.h>\n#include "mitransient_amd.h"\nint main(){printf("%zu %d\\n", sizeof(mtr_backproject_desc), '
            "MTR_ABI_VERSION);return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, version = (int(x) for x in subprocess.check_output([exe]).split())
    assert C.sizeof(_cabi.mtr_backproject_desc) == size and version == 24


# ---------------------------------------------------------------- laplacian_filter
def test_laplacian_filter_matches_a_numpy_stencil():
    import torch
    import mitransient_amd as mitr
    v = np.random.default_rng(5).random((5, 4, 7))
    p = np.pad(v, 1)
    want = (6 * v - p[2:, 1:-1, 1:-1] - p[:-2, 1:-1, 1:-1] - p[1:-1, 2:, 1:-1] - p[1:-1, :-2, 1:-1] - p[1:-1, 1:-1, 2:]
            - p[1:-1, 1:-1, :-2])
    slow = np.zeros_like(v)
    for z in range(5):
        for y in range(4):
            for x in range(7):
                nb = [(z + 1, y, x), (z - 1, y, x), (z, y + 1, x), (z, y - 1, x), (z, y, x + 1), (z, y, x - 1)]
                slow[z, y, x] = 6 * v[z, y, x] - sum(v[q] for q in nb if all(0 <= q[k] < v.shape[k] for k in range(3)))
    assert np.allclose(want, slow, atol=1e-12)
    got = mitr.nlos.laplacian_filter(torch.from_numpy(v))
    assert got.device.type == "cpu" and got.shape == (5, 4, 7)
    assert np.allclose(got.numpy(), slow, atol=1e-12)
    with pytest.raises(ValueError):
        mitr.nlos.laplacian_filter(torch.zeros(3, 3))


# ---------------------------------------------------------------- refusals that need no GPU
def test_backproject_validates_before_touching_the_gpu():
    import mitransient_amd as mitr
    from mitransient_amd.nlos import CaptureGeometry, backproject
    sp = wall_points(4, 2).astype(np.float64)
    g = CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16)
    box = ((-1, -1, 0.5), (1, 1, 1.5), 4)
    ok = np.zeros((2, 4, 16), np.float32)
    for transient, geom, args, kw in (
            (np.zeros((2, 4, 15), np.float32), g, box, {}),                              # bins
            (np.zeros((4, 2, 16), np.float32), g, box, {}),                              # scan size
            (np.zeros((2, 4), np.float32), g, box, {}),                                  # rank
            (np.zeros((2, 4, 2, 2, 16), np.float32), g, box, {}),                        # an exhaustive tensor for a confocal geometry
            (ok, g, ((-1, -1, 0.5), (1, 1, 0.5), 4), {}),                                # empty box
            (ok, g, ((-1, -1, 0.5), (1, 1, 1.5), 0), {}),                                # resolution
            (ok, g, ((-1, -1, 0.5), (1, 1, 1.5), (4, 4)), {}),
            (ok, g, box, {"interpolation": "cubic"}),
            (ok, g, box, {"filter": "gaussian"}),
            (ok, g, box, {"channel": 0}),                                                # no channel axis
            (np.zeros((2, 4, 16, 3), np.float32), g, box, {"channel": 3}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3)[:7], np.zeros((2, 4)), np.zeros(7), 1.2, 0.04, 16), box, {}),
            (ok, CaptureGeometry(SINGLE, sp, sp.reshape(-1, 3)[:2], np.zeros((2, 4)), np.zeros(2), 1.2, 0.04, 16), box, {}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.0, 16), box, {}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 3)), np.zeros(8), 1.2, 0.04, 16), box, {}),
            (np.zeros((2, 4, 3, 2, 16), np.float32),
             CaptureGeometry(EXHAUSTIVE, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16), box, {}),     # 6 != 8 lasers
            (ok, "geometry", box, {})):
        with pytest.raises(ValueError):
            backproject(transient, geom, *args, **kw)
    assert mitr.nlos.backproject is backproject
    import torch
    if not torch.cuda.is_available():           # a valid call without a GPU: the product has no CPU path
        from mitransient_amd._cabi import MitransientAMDError
        with pytest.raises(MitransientAMDError):
            backproject(ok, g, *box)
