"""nlos.backproject on the GPU: the kernels of mtr_backproject.hip against the host build of the same arithmetic
(tests/host_backproject.cpp) and against numpy f64, the kernels' own edges (ragged tiles, one and many scan points, one bin, a row
of 4500 bins, the slab path), render -> backproject -> depth peak end to end, the input forms and the C-ABI's refusals."""
import ctypes as C

import numpy as np
import pytest

from backproject_cases import (CONFOCAL, E2E, E2E_BOX, EXHAUSTIVE, SINGLE, TINY, TOL, bin_disagreements, depth_peak, desc_of,
                               e2e_scene, host_backproject, make_case, reference, tiny_case, wall_points)
from conftest import rel_l2

pytestmark = pytest.mark.gpu


def gpu_backproject(case, expect=0, fill=None):
    """mtr_backproject through the C-ABI on the arrays of a case: (nz, ny, nx) f32"""
    import torch
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    dev = [torch.from_numpy(case[k]).cuda() for k in ("sp", "lp", "so", "lo", "capture")]
    nx, ny, nz = case["res"]
    vol = torch.full((nz, ny, nx), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    d = desc_of(case, *(t.data_ptr() for t in dev[:4]))
    ctx.bind_current_stream()
    rc = ctx.lib.mtr_backproject(ctx.handle, C.byref(d), C.c_void_p(dev[4].data_ptr()), C.c_void_p(vol.data_ptr()))
    torch.cuda.synchronize()
    assert rc == expect, (rc, ctx.lib.mtr_last_error(ctx.handle))
    return vol.cpu().numpy()


def plan(case):
    """(tiles, slabs) mtr_backproject chooses for a case on this device"""
    import torch
    from mitransient_amd import _cabi
    out = (C.c_uint32 * 4)()
    lib = _cabi.load_library()
    lib.mtr_test_backproject_plan.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    rows = case["capture"].shape[0]
    assert lib.mtr_test_backproject_plan(*case["res"], rows, torch.cuda.get_device_properties(0).multi_processor_count, out) == 1
    return out[0], out[1]


def check(case, nearest_checked=True):
    if not case["linear"] and nearest_checked:
        assert bin_disagreements(case) == 0
    got, host, ref = gpu_backproject(case), host_backproject(case), reference(case)
    assert np.abs(ref).max() > 0
    eh, er = rel_l2(got, host), rel_l2(got, ref)
    print(f"rel-L2 against the host build {eh:.3e}, against f64 {er:.3e}")
    assert eh <= TOL and er <= TOL, (eh, er)
    return got


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("kind,interpolation,offsets", TINY)
def test_kernel_matches_host_build_and_f64(kind, interpolation, offsets):
    for capture in ("smooth", "spiky"):
        case = tiny_case(kind, interpolation, offsets, capture)
        got = check(case)
        assert np.array_equal(got, gpu_backproject(case))          # the same call twice: equal bits
        assert plan(case) == (2, 6 if kind == EXHAUSTIVE else 1)   # 64 pairs: one slab; Exhaustive's 384: six of 64


# ---------------------------------------------------------------- the kernels' edges
@pytest.mark.parametrize("res", [(6, 6, 6), (5, 3, 7), (9, 17, 5)])
def test_ragged_tiles(res):
    for kind, interpolation in ((CONFOCAL, "linear"), (EXHAUSTIVE, "nearest")):
        case = tiny_case(kind, interpolation, True, "spiky", res=res)
        check(case)


@pytest.mark.parametrize("n", [1, 65])
def test_scan_point_counts(n):
    sp = wall_points(n, 1) if n > 1 else np.array([[0.25, -0.25, 0.0]], np.float32)
    for kind, interpolation in ((CONFOCAL, "nearest"), (SINGLE, "linear"), (CONFOCAL, "linear")):
        lp = sp if kind == CONFOCAL else np.array([[0.0, 0.5, 0.0]], np.float32)
        check(make_case(kind, sp, lp, interpolation=interpolation, capture="spiky", offsets=True))


@pytest.mark.parametrize("T,start,bin_width", [(1, 1.0, 6.0), (4500, 1.0, 0.00125)])
def test_row_lengths(T, start, bin_width):
    """one bin, and a row longer than anything a workgroup could stage in LDS (64 x 4500 floats).  The long row is compared with
    the host build — the same f32 arithmetic — alone: in bins of 0.00125 a path length of 1 .. 6.5 carries 2e-4 .. 4e-4 of a bin of
    f32 rounding, which the `linear` weight passes on (the host build itself is 3.4e-5 from f64 there)"""
    for interpolation in ("nearest", "linear"):
        case = tiny_case(CONFOCAL, interpolation, T=T, start=start, bin_width=bin_width, capture="spiky")
        if T == 1:
            check(case)
        else:
            got, host = gpu_backproject(case), host_backproject(case)
            e = rel_l2(got, host)
            print(f"rel-L2 against the host build {e:.3e}")
            assert np.abs(host).max() > 0 and e <= TOL


def test_far_box_and_late_window():
    case = tiny_case(CONFOCAL, "linear", vmin=(100, 100, 100), vmax=(102, 102, 101))
    assert np.array_equal(gpu_backproject(case), np.zeros((6, 6, 6), np.float32))
    case = tiny_case(SINGLE, "nearest", vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
    assert np.array_equal(gpu_backproject(case), np.zeros((6, 6, 6), np.float32))
    for interpolation in ("nearest", "linear"):
        check(tiny_case(CONFOCAL, interpolation, capture="spiky", start=2.6))      # a window that starts after the first arrivals


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_slab_path(kind):
    """2 x 2 x 2 voxels against a 32 x 32 scan: the pairs are split over workgroups and the planes added in slab order"""
    sp = wall_points(32, 32)
    lp = sp if kind == CONFOCAL else (np.zeros((1, 3), np.float32) if kind == SINGLE else wall_points(2, 3).reshape(-1, 3))
    for interpolation in ("nearest", "linear"):
        case = make_case(kind, sp, lp, res=(2, 2, 2), interpolation=interpolation, capture="spiky", offsets=True)
        tiles, slabs = plan(case)
        assert tiles == 1 and slabs > 1
        got = check(case)
        assert np.array_equal(got, gpu_backproject(case))
    # a one-slab call on the same voxels: 9 (Exhaustive: 54) pairs are not worth splitting
    case = make_case(kind, wall_points(3, 3), wall_points(3, 3) if kind == CONFOCAL else lp, res=(2, 2, 2), interpolation="linear",
                     capture="spiky", offsets=True)
    assert plan(case) == (1, 1)
    check(case)


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def renders():
    """name -> (geometry, the tensor mi.render returned, wavefront) and the same for auto: rendered once"""
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    out = {}
    for name in sorted(E2E):
        for mode, number in (("wavefront", 2), ("auto", 0)):      # MTR_MODE_WAVEFRONT, MTR_MODE_AUTO
            scene = e2e_scene(name)
            scene.integrator().mode = number
            _, transient = mi.render(scene, spp=64, seed=0)
            out[name, mode] = (mitr.nlos.capture_geometry(scene), transient)
    return out


@pytest.mark.parametrize("mode", ["wavefront", "auto"])
@pytest.mark.parametrize("name", sorted(E2E))
def test_rendered_quad_backprojects_to_its_depth(renders, name, mode):
    import mitransient_amd as mitr
    g, transient = renders[name, mode]
    assert transient.shape[:3] == (16, 16, 128)
    for filt in (None, "laplacian"):
        vol = mitr.nlos.backproject(transient, g, *E2E_BOX, filter=filt)
        assert vol.is_cuda and tuple(vol.shape) == (16, 16, 16)
        z, prof = depth_peak(vol.cpu().numpy())
        print(name, mode, filt, "depth profile peaks at z =", z)
        assert prof.max() > 0 and abs(z - 1.0) <= 1.0 / 16.0, (z, prof)


# ---------------------------------------------------------------- input forms and the C-ABI
def test_input_forms(renders):
    import torch
    import mitransient_amd as mitr
    g, transient = renders["confocal", "auto"]
    t = transient.torch()
    want = mitr.nlos.backproject(t, g, *E2E_BOX, interpolation="linear")
    assert np.array_equal(want.cpu().numpy(), mitr.nlos.backproject(transient, g, *E2E_BOX, interpolation="linear").cpu().numpy())
    assert np.array_equal(want.cpu().numpy(), mitr.nlos.backproject(np.array(transient), g, *E2E_BOX, interpolation="linear").cpu().numpy())
    assert np.array_equal(want.cpu().numpy(), mitr.nlos.backproject(t.double(), g, *E2E_BOX, interpolation="linear").cpu().numpy())
    strided = torch.empty((t.shape[-1], 16, 128, 16), dtype=t.dtype, device=t.device).permute(1, 3, 2, 0)
    strided.copy_(t)
    assert not strided.is_contiguous()
    assert np.array_equal(want.cpu().numpy(), mitr.nlos.backproject(strided, g, *E2E_BOX, interpolation="linear").cpu().numpy())
    # one channel picked, (H, W, T) without a channel axis, and (nx, ny, nz) resolutions
    one = mitr.nlos.backproject(t, g, *E2E_BOX, channel=0)
    assert np.array_equal(one.cpu().numpy(), mitr.nlos.backproject(t[..., 0], g, *E2E_BOX).cpu().numpy())
    assert tuple(mitr.nlos.backproject(t, g, E2E_BOX[0], E2E_BOX[1], (5, 3, 7)).shape) == (7, 3, 5)
    # the python surface against the C-ABI called directly on the same numbers
    case = make_case(g.capture_type, g.sensor_points, g.laser_points, T=g.temporal_bins, start=g.start_opl, bin_width=g.bin_width_opl,
                     vmin=E2E_BOX[0], vmax=E2E_BOX[1], res=(16,) * 3, capture=t[..., 0].cpu().numpy().reshape(256, 128))
    assert np.array_equal(one.cpu().numpy(), gpu_backproject(case))


def test_exhaustive_tensor_layout():
    """an (H, W, Lx, Ly, T, C) tensor is read as rows (s, l = laser_x * Ly + laser_y)"""
    import torch
    from mitransient_amd.nlos import CaptureGeometry, backproject
    case = tiny_case(EXHAUSTIVE, "linear", True, "spiky")
    g = CaptureGeometry(EXHAUSTIVE, case["sp"].reshape(8, 8, 3), case["lp"], case["so"].reshape(8, 8), case["lo"], float(case["start"]),
                        float(case["bin_width"]), 64, (3, 2))
    t6 = torch.from_numpy(case["capture"].reshape(8, 8, 3, 2, 64, 1)).cuda()
    vol = backproject(t6, g, case["vmin"], case["vmax"], 6, interpolation="linear")
    assert np.array_equal(vol.cpu().numpy(), gpu_backproject(case))
    rgb = torch.cat([t6, 3.0 * t6, 2.0 * t6], dim=-1)                  # channels are averaged: 2 x
    assert rel_l2(backproject(rgb, g, case["vmin"], case["vmax"], 6, interpolation="linear").cpu().numpy(), 2.0 * reference(case)) <= TOL


def test_invalid_descriptions_leave_the_volume_untouched():
    from mitransient_amd.runtime import get_context
    good = tiny_case(CONFOCAL)
    bad = []
    for key, value in (("T", 0), ("S", 0), ("L", 0), ("bin_width", np.float32(0.0)), ("bin_width", np.float32(-0.04)),
                       ("res", (6, 0, 6)), ("vmax", np.array([1, -1, 1.5], np.float32)), ("capture_type", 7)):
        c = dict(good)
        c[key] = value
        bad.append(c)
    c = dict(good); c["L"] = 63; bad.append(c)
    c = dict(tiny_case(SINGLE)); c["L"] = 2; bad.append(c)
    for c in bad:
        assert np.all(gpu_backproject(c, expect=-1, fill=7.0) == 7.0)
        assert b"mtr_backproject" in get_context().lib.mtr_last_error(get_context().handle)
    # NULL pointers
    import torch
    ctx = get_context()
    vol = torch.full((6, 6, 6), 7.0, device="cuda")
    dev = [torch.from_numpy(good[k]).cuda() for k in ("sp", "lp", "so", "lo", "capture")]
    for k in range(4):
        ptrs = [t.data_ptr() for t in dev[:4]]
        ptrs[k] = None
        d = desc_of(good, *ptrs)
        assert ctx.lib.mtr_backproject(ctx.handle, C.byref(d), C.c_void_p(dev[4].data_ptr()), C.c_void_p(vol.data_ptr())) == -1
    d = desc_of(good, *(t.data_ptr() for t in dev[:4]))
    assert ctx.lib.mtr_backproject(ctx.handle, C.byref(d), None, C.c_void_p(vol.data_ptr())) == -1
    assert ctx.lib.mtr_backproject(ctx.handle, C.byref(d), C.c_void_p(dev[4].data_ptr()), None) == -1
    assert ctx.lib.mtr_backproject(ctx.handle, None, C.c_void_p(dev[4].data_ptr()), C.c_void_p(vol.data_ptr())) == -1
    torch.cuda.synchronize()
    assert bool((vol == 7.0).all())
