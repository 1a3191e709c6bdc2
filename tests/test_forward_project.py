"""nlos.forward_project on the CPU: the host build of mtr_forward_project.h (tests/host_forward_project.cpp) against an
independent numpy f64 scatter, the transposes of backproject's edge tests, the adjoint identity between the two host builds,
fp_plan, the additive C-ABI, the refusals that need no GPU, and CGLS on a synthetic volume."""
import ctypes as C

import numpy as np
import pytest

from backproject_cases import (CONFOCAL, EXHAUSTIVE, SINGLE, TINY, TOL, bin_disagreements, host_backproject, make_case, positions,
                               reference, tiny_case, wall_points)
from conftest import rel_l2
from forward_project_cases import (adjoint_gap, cgls, cgls_case, host_forward_project, host_plan, make_volume, reference_T,
                                   rows_of)

VOLUMES = ("smooth", "spiky")


def check(case, kinds=VOLUMES):
    if not case["linear"]:
        # the precondition of a `nearest` comparison across precisions: f32 and f64 pick the same bin everywhere
        assert bin_disagreements(case) == 0
    for kind in kinds:
        x = make_volume(case, kind)
        ref = reference_T(case, x)
        assert np.abs(ref).max() > 0
        got = host_forward_project(case, x)
        assert np.all(np.isfinite(got))                 # every cell written over the NaN fill
        e = rel_l2(got, ref)
        print(f"{case['capture_type']} linear={case['linear']} {kind}: rel-L2 {e:.3e}")
        assert e <= TOL, e


# ---------------------------------------------------------------- the host build against numpy f64
@pytest.mark.parametrize("kind,interpolation,offsets", TINY)
def test_host_build_matches_f64(kind, interpolation, offsets):
    check(tiny_case(kind, interpolation, offsets))


def test_f32_restatement_is_within_the_bar():
    """the tolerance holds for the reference alone: the numpy scatter in f32 (mtr_backproject.h's operation order) against f64"""
    for kind, interpolation, offsets in TINY:
        case = tiny_case(kind, interpolation, offsets)
        for vol in VOLUMES:
            x = make_volume(case, vol)
            assert rel_l2(reference_T(case, x, np.float32), reference_T(case, x)) <= TOL


def test_reference_is_the_transpose_of_backprojects_reference():
    """<A y, x> = <y, A^T x> between the two f64 restatements, to rounding of f64"""
    for kind, interpolation, offsets in TINY:
        case = tiny_case(kind, interpolation, offsets, "spiky")
        x = make_volume(case, "spiky").astype(np.float64)
        y = case["capture"].astype(np.float64)
        lhs, rhs = float((reference(case) * x).sum()), float((y * reference_T(case, x)).sum())
        assert abs(lhs - rhs) <= 1e-13 * abs(lhs)


# ---------------------------------------------------------------- edges: the transposes of test_backproject.py's
def test_far_box_gives_exact_zeros():
    for interpolation in ("nearest", "linear"):
        case = tiny_case(CONFOCAL, interpolation, vmin=(100, 100, 100), vmax=(102, 102, 101))
        assert np.array_equal(host_forward_project(case, make_volume(case)), np.zeros((64, 64), np.float32))
    # ... and so far that the path length overflows to inf
    case = tiny_case(SINGLE, "linear", vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
    assert np.array_equal(host_forward_project(case, make_volume(case)), np.zeros((64, 64), np.float32))


@pytest.mark.parametrize("interpolation", ["nearest", "linear"])
def test_one_bin(interpolation):
    case = tiny_case(CONFOCAL, interpolation, T=1, start=1.0, bin_width=6.0)      # paths span 1.17 .. 6.5
    check(case)
    if interpolation == "nearest":          # every path of this geometry lies in the one bin: each row is the sum of the volume
        x = make_volume(case, "spiky")
        assert np.allclose(host_forward_project(case, x), x.sum(), rtol=1e-5)


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_one_scan_point(kind):
    sp = np.array([[0.25, -0.25, 0.0]], np.float32)
    lp = sp if kind == CONFOCAL else np.array([[0.0, 0.5, 0.0]], np.float32)
    for interpolation in ("nearest", "linear"):
        case = make_case(kind, sp, lp, interpolation=interpolation)
        assert bin_disagreements(case) == 0
        check(case)


def test_voxel_on_a_scan_point():
    """8 x 8 x 1 voxels whose centres ARE the scan points (path length 0 for the voxel's own point lands in bin 0)"""
    sp = wall_points(8, 8)
    for interpolation in ("nearest", "linear"):
        case = make_case(CONFOCAL, sp, sp, start=0.0, bin_width=0.125, vmin=(-1, -1, -0.125), vmax=(1, 1, 0.125), res=(8, 8, 1),
                         interpolation=interpolation)
        check(case)
    # nearest, one scan point and only its own voxel lit: exactly the first bin
    one = make_case(CONFOCAL, sp[3:4, 5:6], sp[3:4, 5:6], start=0.0, bin_width=0.125, vmin=(-1, -1, -0.125), vmax=(1, 1, 0.125),
                    res=(8, 8, 1))
    x = np.zeros((1, 8, 8), np.float32)
    x[0, 3, 5] = 0.625
    got = host_forward_project(one, x)
    assert got[0, 0] == np.float32(0.625) and np.count_nonzero(got) == 1


def test_linear_taps_at_minus_one_and_T():
    """one scan point at the origin, one voxel on its normal at height z: d = 2 z, bins of 1 from 0, T = 4 — exact arithmetic"""
    p = np.zeros((1, 3), np.float32)
    x = np.full((1, 1, 1), 8.0, np.float32)

    def at(z):
        case = make_case(CONFOCAL, p, p, T=4, start=0.0, bin_width=1.0, vmin=(-0.5, -0.5, z - 0.5), vmax=(0.5, 0.5, z + 0.5),
                         res=(1, 1, 1), interpolation="linear")
        return host_forward_project(case, x)[0].tolist()
    assert at(0.125) == [0.75 * 8.0, 0.0, 0.0, 0.0]            # u' = -0.25: taps -1 (outside: nothing) and 0
    assert at(0.5) == [0.5 * 8.0, 0.5 * 8.0, 0.0, 0.0]         # u' = 0.5: taps 0 and 1
    assert at(2.125) == [0.0, 0.0, 0.0, 0.25 * 8.0]            # u' = 3.75: taps 3 and T (outside: nothing)
    assert at(2.25) == [0.0, 0.0, 0.0, 0.0]                    # u' = 4: both outside
    assert at(2.0 ** -10) == [0.5 * 8.0 + 2.0 ** -9 * 8.0, 0.0, 0.0, 0.0]      # u' just above -0.5


def test_window_after_the_first_arrivals():
    for interpolation in ("nearest", "linear"):
        case = tiny_case(CONFOCAL, interpolation, start=2.6)
        u = positions(case, np.float64)
        assert 0.2 < np.mean(u < 0) < 0.8                                      # a good share of the paths arrive before the window
        check(case)


def test_invalid_descriptions_leave_the_capture_untouched():
    good = tiny_case(CONFOCAL)
    bad = []
    for key, value in (("T", 0), ("S", 0), ("L", 0), ("bin_width", np.float32(0.0)), ("bin_width", np.float32(-0.04)),
                       ("bin_width", np.float32(np.nan)), ("res", (6, 0, 6)), ("vmax", np.array([1, -1, 1.5], np.float32)),
                       ("capture_type", 7)):
        c = dict(good)
        c[key] = value
        bad.append(c)
    c = dict(good); c["L"] = 63; bad.append(c)                            # Confocal: L != S
    c = dict(tiny_case(SINGLE)); c["L"] = 2; bad.append(c)                # Single: L != 1
    x = make_volume(good)
    for c in bad:
        out = np.full((64, 64), 7.0, np.float32)
        from forward_project_cases import desc_of, host_lib
        d = desc_of(c, c["sp"].ctypes.data, c["lp"].ctypes.data, c["so"].ctypes.data, c["lo"].ctypes.data)
        assert host_lib().hf_forward_project(C.byref(d), C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data)) == -1
        assert np.all(out == 7.0)


# ---------------------------------------------------------------- the adjoint identity between the two host builds
@pytest.mark.parametrize("kind,interpolation,offsets", TINY)
def test_host_builds_are_transposes(kind, interpolation, offsets):
    case = tiny_case(kind, interpolation, offsets, "spiky")
    x, y = make_volume(case, "spiky"), case["capture"]
    gap, bound = adjoint_gap(host_backproject(case), x, y, host_forward_project(case, x))
    print(f"|<Ay, x> - <y, A^T x>| = {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound


# ---------------------------------------------------------------- fp_plan
def test_plan():
    for kind, interpolation, offsets in TINY:
        case = tiny_case(kind, interpolation, offsets)
        pl = host_plan(*case["res"], rows_of(case), case["T"])
        assert (pl["windows"], pl["slabs"], pl["slab_len"]) == (1, 1, 216)
    W = host_plan(6, 6, 6, 64, 64)["window"]
    assert 0 < W <= 16384                                                       # 64 KiB of LDS at most
    assert host_plan(6, 6, 6, 64, W)["windows"] == 1 and host_plan(6, 6, 6, 64, W + 37)["windows"] == 2
    for rows in (2, 12):                                                        # 1 x 2 scan points (Exhaustive: x 6 lasers)
        pl = host_plan(32, 32, 16, rows, 64)
        assert pl["slabs"] > 1 and pl["slabs"] * pl["slab_len"] >= 32 * 32 * 16 > (pl["slabs"] - 1) * pl["slab_len"]
    pl = host_plan(128, 128, 128, 65536, 4096)                                  # config 4: the rows fill the device
    assert (pl["windows"], pl["slabs"], pl["slab_len"]) == (1, 1, 128 ** 3)
    # the byte cap: 4 rows x 2^20 bins are 16 MiB a plane and 256 (row, window) workgroups; a device of 4096 compute units would
    # want 64 slabs, the cap has room for 16 planes
    pl = host_plan(128, 128, 128, 4, 1 << 20, n_cu=4096)
    assert pl["cap"] == 256 << 20 and pl["slabs"] == 16 and pl["slabs"] * 4 * (1 << 20) * 4 <= pl["cap"]
    assert host_plan(128, 128, 128, 4, 1 << 20)["slabs"] == 4                   # 256 compute units: 4 slabs, below the cap
    pl = host_plan(128, 128, 128, 40, 1 << 21, n_cu=4096)                       # a plane above the cap: one slab, no planes at all
    assert pl["slabs"] == 1
    assert host_plan(0, 1, 1, 1, 1) is None and host_plan(1, 1, 1, 1, 0) is None
    assert host_plan(2048, 2048, 512, 1, 1) is None                             # 2^31 voxels


def test_plan_hook_of_the_library():
    from mitransient_amd import _cabi
    lib = C.CDLL(_cabi.LIB_PATH)
    lib.mtr_test_forward_project_plan.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 5)()
    assert lib.mtr_test_forward_project_plan(32, 32, 16, 2, 64, 256, out) == 1
    pl = host_plan(32, 32, 16, 2, 64)
    assert list(out) == [pl["windows"], pl["slabs"], pl["slab_len"], 0, pl["window"]]
    assert lib.mtr_test_forward_project_plan(0, 32, 16, 2, 64, 256, out) == 0


# ---------------------------------------------------------------- the additive C-ABI
def test_abi_is_additive():
    from mitransient_amd import _cabi
    assert _cabi.MTR_ABI_VERSION == 24
    assert "mtr_forward_project" in _cabi.EXPORTS
    lib = C.CDLL(_cabi.LIB_PATH)
    assert hasattr(lib, "mtr_forward_project")
    lib.mtr_abi_version.restype = C.c_int
    assert lib.mtr_abi_version() == 24


# ---------------------------------------------------------------- refusals that need no GPU
def test_python_validates_before_touching_the_gpu():
    import mitransient_amd as mitr
    from mitransient_amd.nlos import CaptureGeometry, forward_project, reconstruct_cgls
    sp = wall_points(4, 2).astype(np.float64)
    g = CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16)
    ex = CaptureGeometry(EXHAUSTIVE, sp, sp.reshape(-1, 3)[:6], np.zeros((2, 4)), np.zeros(6), 1.2, 0.04, 16)
    box = ((-1, -1, 0.5), (1, 1, 1.5))
    ok = np.zeros((4, 4, 4), np.float32)
    for volume, geom, args, kw in (
            (np.zeros((4, 4), np.float32), g, box, {}),                                  # not 3-D
            (np.zeros((4, 4, 4, 1), np.float32), g, box, {}),
            (np.zeros((4, 0, 4), np.float32), g, box, {}),
            (ok, ex, box, {}),                                                           # Exhaustive without laser_grid
            (ok, CaptureGeometry(EXHAUSTIVE, sp, sp.reshape(-1, 3)[:6], np.zeros((2, 4)), np.zeros(6), 1.2, 0.04, 16, (2, 2)), box, {}),
            (ok, g, box, {"interpolation": "cubic"}),
            (ok, g, ((-1, -1, 0.5), (1, 1, 0.5)), {}),                                   # empty box
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3)[:7], np.zeros((2, 4)), np.zeros(7), 1.2, 0.04, 16), box, {}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.0, 16), box, {}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 0), box, {}),
            (ok, "geometry", box, {})):
        with pytest.raises(ValueError, match="forward_project"):
            forward_project(volume, geom, *args, **kw)
    y = np.zeros((2, 4, 16), np.float32)
    for transient, kw in ((y, {"iterations": 0}), (y, {"iterations": 2.5}), (y, {"iterations": True}), (y, {"channel": 0}),
                          (np.zeros((2, 4, 16, 3), np.float32), {"channel": 3}), (y, {"interpolation": "cubic"}),
                          (np.zeros((2, 4, 15), np.float32), {})):
        with pytest.raises(ValueError, match="reconstruct_cgls"):
            reconstruct_cgls(transient, g, *box, 4, **kw)
    assert mitr.nlos.forward_project is forward_project and mitr.nlos.reconstruct_cgls is reconstruct_cgls
    import torch
    if not torch.cuda.is_available():           # valid calls without a GPU: the product has no CPU path
        from mitransient_amd._cabi import MitransientAMDError
        with pytest.raises(MitransientAMDError):
            forward_project(ok, g, *box)
        with pytest.raises(MitransientAMDError):
            reconstruct_cgls(y, g, *box, 4)
        with pytest.raises(MitransientAMDError):     # ... a tensor that asks for a graph included: no eager fall-back
            mitr.nlos.backproject(torch.zeros((2, 4, 16), requires_grad=True), g, *box, 4)


# ---------------------------------------------------------------- CGLS, dense, on the host builds
def check_cgls(x, residuals):
    print("residuals", " ".join(f"{r:.3e}" for r in residuals))
    assert len(residuals) == 11 and residuals[0] == 1.0
    assert residuals[-1] <= 1e-2                     # (the f64 reference reaches 4.7e-4: 20 x for f32)
    assert all(b <= a * (1.0 + 1e-4) for a, b in zip(residuals, residuals[1:]))
    prof = np.asarray(x, np.float64).sum(axis=(1, 2))
    assert int(np.argmax(prof)) == 3, prof


def test_cgls_recovers_a_synthetic_patch():
    case, x0 = cgls_case()
    y64 = reference_T(case, x0)

    def back64(r):
        c = dict(case)
        c["capture"] = r
        return reference(c)
    x, res = cgls(lambda p: reference_T(case, p), back64, y64, 10)
    check_cgls(x, res)
    assert res[-1] <= 1e-3                           # the reference itself: 4.7e-4 measured
    # the same on the host builds, in f32
    y = host_forward_project(case, x0)

    def back32(r):
        c = dict(case)
        c["capture"] = np.ascontiguousarray(r, np.float32)
        return host_backproject(c)
    x, res = cgls(lambda p: host_forward_project(case, p), back32, y, 10)
    assert x.dtype == np.float32
    check_cgls(x, res)
    # what the fit is worth: the best-scaled plain backprojection leaves more than half of the capture unexplained
    bp = back32(y)
    fb = host_forward_project(case, bp).astype(np.float64)
    scale = float((fb * y).sum() / (fb * fb).sum())
    assert 0.4 < np.linalg.norm(scale * fb - y) / np.linalg.norm(y.astype(np.float64)) < 0.7
