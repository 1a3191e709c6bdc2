"""nlos.forward_project on the GPU: the kernels of mtr_forward_project.hip against the host build of the same arithmetic
(tests/host_forward_project.cpp) and against an independent numpy f64 scatter, the kernels' own edges (ragged voxel counts, one
and many scan points, one bin, more than one LDS window, the slab path, a NaN voxel), the adjoint identity with mtr_backproject,
autograd through both calls, the input forms, the C-ABI's refusals and reconstruct_cgls."""
import ctypes as C

import numpy as np
import pytest

from backproject_cases import (CONFOCAL, E2E_BOX, EXHAUSTIVE, SINGLE, TINY, TOL, bin_disagreements, depth_peak, desc_of, e2e_scene,
                               make_case, reference, tiny_case, wall_points)
from conftest import rel_l2
from forward_project_cases import (adjoint_gap, cgls_case, host_forward_project, make_volume, reference_T, rows_of)

pytestmark = pytest.mark.gpu

VOLUMES = ("smooth", "spiky")


def gpu_call(entry, case, src, expect=0, fill=np.nan):
    """mtr_forward_project / mtr_backproject through the C-ABI on the arrays of a case; the output is pre-filled"""
    import torch
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    dev = [torch.from_numpy(case[k]).cuda() for k in ("sp", "lp", "so", "lo")]
    nx, ny, nz = case["res"]
    shape = (rows_of(case), case["T"]) if entry == "mtr_forward_project" else (nz, ny, nx)
    out = torch.full(shape, float(fill), dtype=torch.float32, device="cuda")
    s = torch.from_numpy(np.ascontiguousarray(src, np.float32)).cuda()
    d = desc_of(case, *(t.data_ptr() for t in dev))
    ctx.bind_current_stream()
    rc = getattr(ctx.lib, entry)(ctx.handle, C.byref(d), C.c_void_p(s.data_ptr()), C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    assert rc == expect, (rc, ctx.lib.mtr_last_error(ctx.handle))
    return out.cpu().numpy()


def gpu_forward_project(case, volume, **kw):
    return gpu_call("mtr_forward_project", case, volume, **kw)


def plan(case):
    """(windows, slabs, kFpWindow) mtr_forward_project chooses for a case on this device"""
    import torch
    from mitransient_amd import _cabi
    out = (C.c_uint32 * 5)()
    lib = _cabi.load_library()
    lib.mtr_test_forward_project_plan.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.mtr_test_forward_project_plan(*case["res"], rows_of(case), case["T"], n_cu, out) == 1
    return out[0], out[1], out[4]


def check(case, kinds=VOLUMES, f64=True, adjoint=False):
    if not case["linear"] and f64:
        assert bin_disagreements(case) == 0
    for kind in kinds:
        x = make_volume(case, kind)
        got, host = gpu_forward_project(case, x), host_forward_project(case, x)
        assert np.all(np.isfinite(got))                 # every cell written over the NaN fill
        assert np.abs(host).max() > 0
        eh = rel_l2(got, host)
        er = rel_l2(got, reference_T(case, x)) if f64 else 0.0
        print(f"rel-L2 against the host build {eh:.3e}, against f64 {er:.3e}")
        assert eh <= TOL and er <= TOL, (eh, er)
        if adjoint:
            gap, bound = adjoint_gap(gpu_call("mtr_backproject", case, case["capture"]), x, case["capture"], got)
            print(f"|<Ay, x> - <y, A^T x>| = {gap:.3e}, bound {bound:.3e}")
            assert gap <= bound


# ---------------------------------------------------------------- parity and the adjoint identity
@pytest.mark.parametrize("kind,interpolation,offsets", TINY)
def test_kernel_matches_host_build_and_f64(kind, interpolation, offsets):
    case = tiny_case(kind, interpolation, offsets, "spiky")
    assert plan(case)[:2] == (1, 1)
    check(case, adjoint=True)


# ---------------------------------------------------------------- the kernels' edges
@pytest.mark.parametrize("res", [(5, 3, 7), (9, 17, 5), (1, 1, 1)])
def test_ragged_voxel_counts(res):
    for kind, interpolation in ((CONFOCAL, "linear"), (EXHAUSTIVE, "nearest")):
        check(tiny_case(kind, interpolation, True, res=res))


@pytest.mark.parametrize("n", [1, 65])
def test_scan_point_counts(n):
    sp = wall_points(n, 1) if n > 1 else np.array([[0.25, -0.25, 0.0]], np.float32)
    for kind, interpolation in ((CONFOCAL, "nearest"), (SINGLE, "linear"), (CONFOCAL, "linear")):
        lp = sp if kind == CONFOCAL else np.array([[0.0, 0.5, 0.0]], np.float32)
        check(make_case(kind, sp, lp, interpolation=interpolation, offsets=True))


def test_one_bin():
    for interpolation in ("nearest", "linear"):
        check(tiny_case(CONFOCAL, interpolation, T=1, start=1.0, bin_width=6.0))


def test_more_than_one_window():
    """a row longer than a workgroup's LDS window.  Compared with the host build — the same f32 arithmetic — alone, as
    test_gpu_backproject.py's test_row_lengths does and for its reason: in bins this fine the f32 rounding of a path length is a
    visible fraction of a bin, which the `linear` weight passes on"""
    W = plan(tiny_case(CONFOCAL))[2]
    T = W + 37
    bw = 5.5 / T                                    # the second window holds the path lengths 3 .. 3.0124: 12^3 voxels reach it
    for interpolation in ("nearest", "linear"):
        case = tiny_case(CONFOCAL, interpolation, T=T, start=3.0 - W * bw, bin_width=bw, capture="spiky", res=(12, 12, 12))
        assert plan(case)[0] == 2 and plan(case)[1] == 1
        x = make_volume(case, "spiky")
        host = host_forward_project(case, x)
        assert np.abs(host[:, W:]).max() > 0 and np.abs(host[:, :W]).max() > 0          # both windows receive
        check(case, f64=False, adjoint=True)


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_slab_path(kind):
    """1 x 2 scan points against 32 x 32 x 16 voxels: the voxels are split over workgroups and the planes added in slab order"""
    sp = wall_points(2, 1)
    lp = sp if kind == CONFOCAL else (np.zeros((1, 3), np.float32) if kind == SINGLE else wall_points(2, 3).reshape(-1, 3))
    for interpolation in ("nearest", "linear"):
        case = make_case(kind, sp, lp, res=(32, 32, 16), interpolation=interpolation, capture="spiky", offsets=True)
        windows, slabs, _ = plan(case)
        assert windows == 1 and slabs > 1
        check(case, kinds=("spiky",), adjoint=True)


def test_far_box_and_late_window():
    case = tiny_case(CONFOCAL, "linear", vmin=(100, 100, 100), vmax=(102, 102, 101))
    assert np.array_equal(gpu_forward_project(case, make_volume(case)), np.zeros((64, 64), np.float32))
    case = tiny_case(SINGLE, "nearest", vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
    assert np.array_equal(gpu_forward_project(case, make_volume(case)), np.zeros((64, 64), np.float32))
    for interpolation in ("nearest", "linear"):
        check(tiny_case(CONFOCAL, interpolation, start=2.6))       # a window that starts after the first arrivals


def test_one_nan_voxel_reaches_its_cells_and_no_others():
    """... and zeros are the only voxels skipped: a volume of zeros around the NaN gives NaN exactly where f64 says that voxel lands"""
    for kind, interpolation in ((CONFOCAL, "nearest"), (EXHAUSTIVE, "linear"), (SINGLE, "linear")):
        case = tiny_case(kind, interpolation, True)
        one = np.zeros((6, 6, 6), np.float32)
        one[2, 4, 1] = 1.0
        reached = reference_T(case, one) != 0                     # (no linear weight of this voxel is exactly 0 in these cases)
        assert 0 < reached.sum() < reached.size
        for rest in (0.0, "smooth"):
            x = np.zeros((6, 6, 6), np.float32) if rest == 0.0 else make_volume(case, "smooth")
            x[2, 4, 1] = np.nan
            got = gpu_forward_project(case, x)
            nan = np.isnan(got)
            assert np.array_equal(nan, reached)
            clean = x.copy()
            clean[2, 4, 1] = 0.0
            want = reference_T(case, clean)
            assert rel_l2(np.where(nan, 0.0, got), np.where(nan, 0.0, want)) <= TOL


# ---------------------------------------------------------------- autograd
def tiny_geometry(case, grid=None):
    from mitransient_amd.nlos import CaptureGeometry
    return CaptureGeometry(case["capture_type"], case["sp"].reshape(8, 8, 3), case["lp"], case["so"].reshape(8, 8), case["lo"],
                           float(case["start"]), float(case["bin_width"]), case["T"], grid)


def np_laplacian(v):
    p = np.pad(v, 1)
    return (6 * v - p[2:, 1:-1, 1:-1] - p[:-2, 1:-1, 1:-1] - p[1:-1, 2:, 1:-1] - p[1:-1, :-2, 1:-1] - p[1:-1, 1:-1, 2:]
            - p[1:-1, 1:-1, :-2])


@pytest.mark.parametrize("interpolation", ["nearest", "linear"])
def test_autograd_through_backproject(interpolation):
    import torch
    from mitransient_amd.nlos import backproject
    case = tiny_case(CONFOCAL, interpolation, True, "spiky")
    g = tiny_geometry(case)
    rng = np.random.default_rng(2)
    t = torch.from_numpy(rng.random((8, 8, 64, 3)).astype(np.float32)).cuda().requires_grad_(True)
    w = rng.standard_normal((6, 6, 6))
    wt = torch.from_numpy(w.astype(np.float32)).cuda()
    vol = backproject(t, g, case["vmin"], case["vmax"], 6, interpolation=interpolation, filter="laplacian")
    assert vol.grad_fn is not None
    (vol * wt).sum().backward()
    # the zero-padded 7-point Laplacian is symmetric: d loss / d t[..., c] = A^T (laplacian(w)) / 3
    want = reference_T(case, np_laplacian(w.astype(np.float32).astype(np.float64))).reshape(8, 8, 64) / 3.0
    for c in range(3):
        assert rel_l2(t.grad[..., c].cpu().numpy(), want) <= TOL
    # channel=1: the other channels receive zero
    t2 = t.detach().clone().requires_grad_(True)
    (backproject(t2, g, case["vmin"], case["vmax"], 6, interpolation=interpolation, channel=1) * wt).sum().backward()
    assert rel_l2(t2.grad[..., 1].cpu().numpy(), reference_T(case, w.astype(np.float32)).reshape(8, 8, 64)) <= TOL
    assert not t2.grad[..., 0].any() and not t2.grad[..., 2].any()
    # no requires_grad, or grad disabled: no graph, and the bits of the C-ABI called directly on the same numbers
    plain = backproject(t.detach()[..., 1], g, case["vmin"], case["vmax"], 6, interpolation=interpolation)
    assert plain.grad_fn is None and not plain.requires_grad
    c1 = dict(case)
    c1["capture"] = np.ascontiguousarray(t.detach()[..., 1].cpu().numpy().reshape(64, 64))
    direct = gpu_call("mtr_backproject", c1, c1["capture"])
    assert np.array_equal(plain.cpu().numpy(), direct)
    with torch.no_grad():
        quiet = backproject(t, g, case["vmin"], case["vmax"], 6, interpolation=interpolation, channel=1)
    assert quiet.grad_fn is None and np.array_equal(quiet.cpu().numpy(), direct)
    # the graph's forward value is the same kernel's
    assert np.array_equal(backproject(t, g, case["vmin"], case["vmax"], 6, interpolation=interpolation, channel=1).detach().cpu().numpy(), direct)


@pytest.mark.parametrize("interpolation", ["nearest", "linear"])
def test_autograd_through_forward_project(interpolation):
    import torch
    from mitransient_amd.nlos import forward_project
    case = tiny_case(CONFOCAL, interpolation, True, "spiky")
    g = tiny_geometry(case)
    x = torch.from_numpy(make_volume(case, "smooth")).cuda().requires_grad_(True)
    wt = torch.from_numpy(case["capture"].reshape(8, 8, 64)).cuda()
    cap = forward_project(x, g, case["vmin"], case["vmax"], interpolation=interpolation)
    assert cap.grad_fn is not None and tuple(cap.shape) == (8, 8, 64)
    (cap * wt).sum().backward()
    assert rel_l2(x.grad.cpu().numpy(), reference(case)) <= TOL           # d <w, A^T x> / dx = A w
    plain = forward_project(x.detach(), g, case["vmin"], case["vmax"], interpolation=interpolation)
    assert plain.grad_fn is None and not plain.requires_grad
    assert rel_l2(plain.cpu().numpy(), cap.detach().cpu().numpy()) <= TOL


# ---------------------------------------------------------------- input forms and the C-ABI
def test_input_forms():
    import torch
    from mitransient_amd.nlos import forward_project
    from mitransient_amd.tensor import TensorXf
    case = tiny_case(SINGLE, "linear", True)
    g = tiny_geometry(case)
    x = make_volume(case, "spiky")
    want = reference_T(case, x).reshape(8, 8, 64)
    args = (g, case["vmin"], case["vmax"])
    strided = torch.empty((6, 6, 6), dtype=torch.float32).permute(2, 1, 0)
    strided.copy_(torch.from_numpy(x))
    assert not strided.is_contiguous()
    for form in (x, torch.from_numpy(x), torch.from_numpy(x).cuda(), torch.from_numpy(x).double(), strided, TensorXf(torch.from_numpy(x).cuda())):
        got = forward_project(form, *args, interpolation="linear")
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (8, 8, 64)
        assert rel_l2(got.cpu().numpy(), want) <= TOL
    # a ragged (nx, ny, nz): the resolution comes from the shape
    c2 = tiny_case(SINGLE, "nearest", True, res=(5, 3, 7))
    x2 = make_volume(c2)
    assert x2.shape == (7, 3, 5)
    assert rel_l2(forward_project(x2, tiny_geometry(c2), c2["vmin"], c2["vmax"]).cpu().numpy().reshape(64, 64), reference_T(c2, x2)) <= TOL


def test_exhaustive_tensor_layout():
    """the rows (s, l = laser_x * Ly + laser_y) of the C-ABI come back as (H, W, Lx, Ly, T)"""
    from mitransient_amd.nlos import forward_project
    case = tiny_case(EXHAUSTIVE, "linear", True)
    x = make_volume(case, "spiky")
    got = forward_project(x, tiny_geometry(case, (3, 2)), case["vmin"], case["vmax"], interpolation="linear")
    assert tuple(got.shape) == (8, 8, 3, 2, 64)
    direct = gpu_forward_project(case, x).reshape(8, 8, 3, 2, 64)
    assert rel_l2(got.cpu().numpy(), direct) <= TOL
    assert rel_l2(got.cpu().numpy(), reference_T(case, x).reshape(8, 8, 3, 2, 64)) <= TOL
    with pytest.raises(ValueError):
        forward_project(x, tiny_geometry(case), case["vmin"], case["vmax"])


def test_invalid_descriptions_leave_the_capture_untouched():
    import torch
    from mitransient_amd.runtime import get_context
    good = tiny_case(CONFOCAL)
    x = make_volume(good)
    bad = []
    for key, value in (("T", 0), ("S", 0), ("L", 0), ("bin_width", np.float32(0.0)), ("bin_width", np.float32(-0.04)),
                       ("res", (6, 0, 6)), ("vmax", np.array([1, -1, 1.5], np.float32)), ("capture_type", 7)):
        c = dict(good)
        c[key] = value
        bad.append(c)
    c = dict(good); c["L"] = 63; bad.append(c)
    c = dict(tiny_case(SINGLE)); c["L"] = 2; bad.append(c)
    ctx = get_context()
    dev = [torch.from_numpy(good[k]).cuda() for k in ("sp", "lp", "so", "lo")]
    vol = torch.from_numpy(x).cuda()
    out = torch.full((64, 64), 7.0, device="cuda")

    def call(d, v, o):
        return ctx.lib.mtr_forward_project(ctx.handle, d, v, o)
    for c in bad:
        d = desc_of(c, *(t.data_ptr() for t in dev))
        assert call(C.byref(d), C.c_void_p(vol.data_ptr()), C.c_void_p(out.data_ptr())) == -1
        assert b"mtr_forward_project:" in ctx.lib.mtr_last_error(ctx.handle)
    # NULL pointers
    for k in range(4):
        ptrs = [t.data_ptr() for t in dev]
        ptrs[k] = None
        d = desc_of(good, *ptrs)
        assert call(C.byref(d), C.c_void_p(vol.data_ptr()), C.c_void_p(out.data_ptr())) == -1
    d = desc_of(good, *(t.data_ptr() for t in dev))
    assert call(C.byref(d), None, C.c_void_p(out.data_ptr())) == -1
    assert call(C.byref(d), C.c_void_p(vol.data_ptr()), None) == -1
    assert call(None, C.c_void_p(vol.data_ptr()), C.c_void_p(out.data_ptr())) == -1
    assert b"mtr_forward_project:" in ctx.lib.mtr_last_error(ctx.handle)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------- reconstruct_cgls
def test_cgls_recovers_a_synthetic_patch():
    from mitransient_amd.nlos import reconstruct_cgls
    from test_forward_project import check_cgls
    case, x0 = cgls_case()
    y = gpu_forward_project(case, x0).reshape(8, 8, 64)
    x, residuals = reconstruct_cgls(y, tiny_geometry(case), case["vmin"], case["vmax"], 6, iterations=10)
    assert x.is_cuda and tuple(x.shape) == (6, 6, 6) and x.grad_fn is None and all(type(r) is float for r in residuals)
    check_cgls(x.cpu().numpy(), residuals)
    # a channel axis is averaged, an all-zero capture gives a zero volume
    x3, r3 = reconstruct_cgls(np.stack([y, 3 * y, 2 * y], axis=-1), tiny_geometry(case), case["vmin"], case["vmax"], 6, iterations=10)
    assert rel_l2(x3.cpu().numpy(), 2.0 * x.cpu().numpy()) <= 1e-3 and abs(r3[-1] - residuals[-1]) <= 1e-3
    z, rz = reconstruct_cgls(np.zeros_like(y), tiny_geometry(case), case["vmin"], case["vmax"], 6, iterations=2)
    assert not z.any() and rz == [1.0, 1.0, 1.0]


E2E_ITERATIONS = 5


@pytest.fixture(scope="module")
def rendered():
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    scene = e2e_scene("confocal")
    _, transient = mi.render(scene, spp=64, seed=0)
    return mitr.nlos.capture_geometry(scene), transient


def test_cgls_on_a_rendered_capture(rendered):
    from mitransient_amd.nlos import reconstruct_cgls
    g, transient = rendered
    assert transient.shape[:3] == (16, 16, 128)
    vol, residuals = reconstruct_cgls(transient, g, *E2E_BOX, iterations=E2E_ITERATIONS)
    print("residuals", residuals)
    assert all(b <= a * (1.0 + 1e-4) for a, b in zip(residuals, residuals[1:])) and residuals[-1] < 1.0
    z, prof = depth_peak(vol.cpu().numpy())
    print("depth profile peaks at z =", z)
    assert prof.max() > 0 and abs(z - 1.0) <= 1.0 / 16.0, (z, prof)


def test_a_loss_on_the_volume_reaches_a_scene_parameter():
    """render -> backproject -> the plane at z = 1 -> backward: a brighter hidden quad makes a brighter voxel plane"""
    import torch
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    scene = e2e_scene("confocal")
    key = "hidden.bsdf.reflectance.value"
    p = mi.traverse(scene)
    albedo = torch.tensor([0.7, 0.7, 0.7], requires_grad=True)
    p[key] = albedo
    p.update()
    _, transient = mi.render(scene, p, spp=16, seed=0, seed_grad=1, spp_grad=16)
    vol = mitr.nlos.backproject(transient.torch(), mitr.nlos.capture_geometry(scene), *E2E_BOX)
    assert vol.grad_fn is not None
    vol[7:9].sum().backward()                   # the two voxel planes that meet at z = 1
    assert albedo.grad is not None and bool(torch.isfinite(albedo.grad).all()) and bool((albedo.grad > 0).all()), albedo.grad
