"""nlos.phasor_forward_project on the GPU: the kernels of mtr_phasor_forward_project.hip against the host build of the same
arithmetic (tests/host_phasor_forward_project.cpp) and against numpy f64, the exact one-term identity with
mtr_phasor_backproject on the device, the kernels' edges (partial strides, partial frequency blocks, one and many scan points,
the slab path, the window, a NaN voxel), autograd through both functions, the input forms, the C-ABI's refusals and
phasor_reconstruct_cgls on a synthetic patch and on a rendered quad."""
import ctypes as C

import numpy as np
import pytest

import phasor_backproject_cases as pc
import phasor_forward_project_cases as fc
from phasor_backproject_cases import CONFOCAL, E2E_BOX, EXHAUSTIVE, FLT_MAX, PARITY, PB_TOL, SINGLE, depth_peak, desc_of, wall_points
from phasor_forward_project_cases import (host_phasor_forward_project, make_case, one_hot_phasors, one_hot_volume, parity_case,
                                          reference, rel_l2, rows_of, tiny_case, with_form, with_volume)
from test_gpu_phasor_backproject import gpu_phasor_backproject
from test_phasor_backproject import WINDOW_CUT, bad_descriptions
from test_phasor_forward_project import parity_reference

pytestmark = pytest.mark.gpu
KEYS = ("sp", "lp", "so", "lo", "freq")


def gpu_phasor_forward_project(case, expect=0, fill=None):
    """mtr_phasor_forward_project through the C-ABI on the arrays of a case: complex (rows, F) — or, refused, the (rows, F, 2) f32"""
    import torch
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    dev = [torch.from_numpy(case[k]).cuda() for k in KEYS + ("volume",)]
    w = None if case["weights"] is None else torch.from_numpy(case["weights"]).cuda()
    out = torch.full((max(rows_of(case), 1), max(case["F"], 1), 2), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    d = desc_of(case, *(t.data_ptr() for t in dev[:5]), None if w is None else w.data_ptr())
    ctx.bind_current_stream()
    rc = ctx.lib.mtr_phasor_forward_project(ctx.handle, C.byref(d), C.c_void_p(dev[5].data_ptr()), C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    assert rc == expect, (rc, ctx.lib.mtr_last_error(ctx.handle))
    return fc.as_complex(out.cpu().numpy()) if expect == 0 else out.cpu().numpy()


def plan(case):
    """(blocks, slabs, slab_len) mtr_phasor_forward_project chooses for a case on this device (pf_plan)"""
    import torch
    from mitransient_amd import _cabi
    lib = _cabi.load_library()
    lib.mtr_test_phasor_forward_project_plan.argtypes = fc.PLAN_ARGS
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return fc.plan_of(lib.mtr_test_phasor_forward_project_plan, *case["res"], rows_of(case), case["F"], n_cu)


def check(case, ref=None, host=None):
    got = gpu_phasor_forward_project(case)
    host = host_phasor_forward_project(case) if host is None else host
    ref = reference(case) if ref is None else ref
    assert np.abs(ref).max() > 0
    eh, er = rel_l2(got, host), rel_l2(got, ref)
    print(f"rel-L2 against the host build {eh:.3e}, against f64 {er:.3e}")
    assert eh <= PB_TOL and er <= PB_TOL, (eh, er)
    assert np.array_equal(got, gpu_phasor_forward_project(case))               # the same call twice: equal bits
    return got


def geometry_of(case, grid=None):
    from mitransient_amd.nlos import CaptureGeometry
    return CaptureGeometry(case["capture_type"], case["sp"].reshape(8, 8, 3), case["lp"], case["so"].reshape(8, 8), case["lo"],
                           float(case["start"]), 0.02, 256, grid)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("kind,offsets,F,weights", PARITY)
def test_kernel_matches_host_build_and_f64(kind, offsets, F, weights):
    ref = parity_reference(kind, offsets, F, weights)
    for form in ("uniform", "table"):
        case = parity_case(kind, offsets, F, weights, form)
        check(case, ref)
    assert plan(case)[:2] == ((F + 15) // 16, 1)                               # the tiny cases: one slab


# ---------------------------------------------------------------- bit-identical factors
@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_one_term_identity_is_exact(kind):
    """U = 1 in one voxel against P = 1 in one (p, k): Q[p, k] == conj(V(v0)) as numbers, between the two kernels"""
    v0 = (4, 1, 3)
    for form in ("uniform", "table"):
        base = with_form(pc.tiny_case(kind, F=151, offsets=True), form)
        assert base["weights"] is None and base["tau_max"] == FLT_MAX
        q = gpu_phasor_forward_project(with_volume(base, one_hot_volume(base, v0)))
        for p in (5, rows_of(base) - 2):
            for k in (0, 15, 16, 17, 150):
                c = dict(base)
                c["phasors"] = one_hot_phasors(base, p, k)
                v = gpu_phasor_backproject(c)[v0[2], v0[1], v0[0]]
                assert v != 0 and q[p, k] == np.conj(v), (form, p, k, q[p, k], v)


# ---------------------------------------------------------------- the kernels' edges
@pytest.mark.parametrize("res", [(5, 3, 7), (9, 17, 5)])
def test_ragged_volumes(res):
    for kind, form, weights in ((CONFOCAL, "uniform", "gaussian"), (EXHAUSTIVE, "table", None)):
        check(tiny_case(kind, offsets=True, form=form, weights=weights, res=res))


@pytest.mark.parametrize("F", [1, 16, 17, 151])
def test_frequency_block_edges(F):
    for kind in (CONFOCAL, EXHAUSTIVE):
        for weights in (None, np.linspace(0.5, 1.5, F)):
            case = tiny_case(kind, F=F, offsets=True, weights=weights)
            assert (case["freq_step"] > 0) == (F > 1)
            ref = reference(case)
            got, table = check(case, ref), check(with_form(case, "table"), ref)
            if F == 1:
                assert np.array_equal(got, table)


@pytest.mark.parametrize("n", [1, 65])
def test_scan_point_counts(n):
    sp = wall_points(n, 1) if n > 1 else np.array([[0.25, -0.25, 0.0]], np.float32)
    for kind, form, weights in ((CONFOCAL, "uniform", None), (SINGLE, "table", "gaussian"), (SINGLE, "uniform", "gaussian")):
        lp = sp if kind == CONFOCAL else np.array([[0.0, 0.5, 0.0]], np.float32)
        assert check(make_case(kind, sp, lp, offsets=True, form=form, weights=weights)).shape == (n, 28)


def slab_lasers(kind, sp):
    return sp if kind == CONFOCAL else (np.zeros((1, 3), np.float32) if kind == SINGLE else pc.tiny_case(EXHAUSTIVE)["lp"])


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_slab_path(kind):
    """2 scan points (Exhaustive: x 6 lasers) against 32 x 32 x 16 voxels: the voxels are split over workgroups and the planes
    added in slab order; then 600 scan points on the same volume, which one slab serves"""
    res = (32, 32, 16)
    sp = np.array([[0.25, -0.25, 0.0], [-0.5, 0.75, 0.0]], np.float32)
    for form, weights in (("uniform", "gaussian"), ("table", None)):
        case = make_case(kind, sp, slab_lasers(kind, sp), res=res, offsets=True, form=form, weights=weights)
        blocks, slabs, slab_len = plan(case)
        assert blocks == 2 and slabs > 1 and (slabs - 1) * slab_len < 32 * 32 * 16 <= slabs * slab_len
        check(case)
    # one slab: the kernel on all 600 scan points; the host build and f64 on the rows of five of them (a row depends on its own
    # scan point alone)
    n = 100 if kind == EXHAUSTIVE else 600
    sp = wall_points(n // 20, 20).reshape(-1, 3)
    case = make_case(kind, sp, slab_lasers(kind, sp), res=res, offsets=True, weights="gaussian")
    assert plan(case)[1] == 1
    got = gpu_phasor_forward_project(case)
    assert np.array_equal(got, gpu_phasor_forward_project(case))
    some = np.array([0, 1, n // 2, n - 2, n - 1])
    sub = make_case(kind, sp[some], slab_lasers(kind, sp[some]), res=res, offsets=True, weights="gaussian", volume=case["volume"])
    per = 6 if kind == EXHAUSTIVE else 1
    rows = (some[:, None] * per + np.arange(per)[None, :]).reshape(-1)
    eh, er = rel_l2(got[rows], host_phasor_forward_project(sub)), rel_l2(got[rows], reference(sub))
    print(f"one slab: rel-L2 against the host build {eh:.3e}, against f64 {er:.3e}")
    assert eh <= PB_TOL and er <= PB_TOL


def test_window():
    film = pc.FILMS[28]
    capture = (np.float32(0.0), np.float32(film["temporal_bins"] * film["bin_width_opl"]))
    for kind in (CONFOCAL, SINGLE, EXHAUSTIVE):
        for form in ("uniform", "table"):
            case = tiny_case(kind, form=form, window=capture, vmin=(100, 100, 100), vmax=(102, 102, 101))
            assert np.array_equal(gpu_phasor_forward_project(case), np.zeros((rows_of(case), 28)))
            case = tiny_case(kind, form=form, weights="gaussian", vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
            assert case["tau_max"] == FLT_MAX
            assert np.array_equal(gpu_phasor_forward_project(case), np.zeros((rows_of(case), 28)))
            case = tiny_case(kind, weights="gaussian", form=form, **WINDOW_CUT)
            m64 = pc.in_window(case, np.float64)
            assert np.array_equal(pc.in_window(case, np.float32), m64)
            check(case)
            # a NaN in one voxel reaches exactly the rows whose window contains that voxel
            vol = case["volume"].copy()
            vol[1, 3, 2, 0] = np.nan
            got = gpu_phasor_forward_project(with_volume(case, vol))
            reached = m64[(1 * 6 + 3) * 6 + 2]
            assert reached.any() and not reached.all()
            assert np.array_equal(np.isnan(got).all(axis=1), reached) and np.array_equal(np.isnan(got).any(axis=1), reached)


# ---------------------------------------------------------------- autograd
def pairs_of(z):
    z = np.asarray(z)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1), np.float32)


def test_autograd():
    import torch
    from mitransient_amd.nlos import phasor_backproject, phasor_forward_project
    case = tiny_case(CONFOCAL, F=28, weights="gaussian")
    g = geometry_of(case)
    args = (g, case["freq"], case["vmin"], case["vmax"])
    kw = dict(weights=case["weights"])
    # through phasor_backproject: loss = |A P|^2, d loss / d P = 2 A^H (A P) in torch's convention
    AP = gpu_phasor_backproject(case)
    want = 2.0 * gpu_phasor_forward_project(with_volume(case, pairs_of(AP)))
    P = torch.view_as_complex(torch.from_numpy(case["phasors"].reshape(8, 8, 28, 2))).cuda().requires_grad_(True)
    vol = phasor_backproject(P, *args, 6, **kw)
    assert vol.grad_fn is not None and vol.dtype == torch.complex64
    (vol.abs() ** 2).sum().backward()
    e = rel_l2(P.grad.cpu().numpy().reshape(64, 28), want)
    print(f"gradient through phasor_backproject (complex input): rel-L2 {e:.3e}")
    assert e <= PB_TOL
    Pr = torch.from_numpy(case["phasors"].reshape(8, 8, 28, 2)).cuda().requires_grad_(True)
    (phasor_backproject(Pr, *args, 6, **kw).abs() ** 2).sum().backward()
    assert Pr.grad.dtype == torch.float32 and tuple(Pr.grad.shape) == (8, 8, 28, 2)
    assert rel_l2(fc.as_complex(Pr.grad.cpu().numpy()).reshape(64, 28), want) <= PB_TOL
    # through phasor_forward_project: loss = |A^H U|^2, d loss / d U = 2 A (A^H U); a real volume receives the real part
    AHU = gpu_phasor_forward_project(case)
    c2 = dict(case)
    c2["phasors"] = pairs_of(AHU)
    want = 2.0 * gpu_phasor_backproject(c2)
    U = torch.view_as_complex(torch.from_numpy(case["volume"])).cuda().requires_grad_(True)
    Q = phasor_forward_project(U, *args, **kw)
    assert Q.grad_fn is not None and Q.dtype == torch.complex64 and tuple(Q.shape) == (8, 8, 28)
    (Q.abs() ** 2).sum().backward()
    assert rel_l2(U.grad.cpu().numpy(), want) <= PB_TOL
    real = with_volume(case, np.stack([case["volume"][..., 0], np.zeros((6, 6, 6), np.float32)], axis=-1))
    c3 = dict(case)
    c3["phasors"] = pairs_of(gpu_phasor_forward_project(real))
    want = 2.0 * gpu_phasor_backproject(c3).real
    X = torch.from_numpy(case["volume"][..., 0].copy()).cuda().requires_grad_(True)
    (phasor_forward_project(X, *args, **kw).abs() ** 2).sum().backward()
    assert X.grad.dtype == torch.float32 and tuple(X.grad.shape) == (6, 6, 6)
    assert rel_l2(X.grad.cpu().numpy(), want) <= PB_TOL
    # no requires_grad, or grad disabled: no graph, and the bits of the C-ABI called directly on the same numbers
    plain = phasor_backproject(P.detach(), *args, 6, **kw)
    with torch.no_grad():
        quiet = phasor_backproject(P, *args, 6, **kw)
    for v in (plain, quiet):
        assert v.grad_fn is None and not v.requires_grad and np.array_equal(v.cpu().numpy().astype(np.complex128), AP)
    plain = phasor_forward_project(U.detach(), *args, **kw)
    with torch.no_grad():
        quiet = phasor_forward_project(U, *args, **kw)
    for v in (plain, quiet):
        assert v.grad_fn is None and not v.requires_grad and np.array_equal(v.cpu().numpy().astype(np.complex128).reshape(64, 28), AHU)


# ---------------------------------------------------------------- input forms and the C-ABI
def test_input_forms():
    import torch
    from mitransient_amd.nlos import phasor_forward_project
    from mitransient_amd.tensor import TensorXf
    case = tiny_case(SINGLE, F=28, offsets=True, weights=np.linspace(0.5, 1.5, 28), **WINDOW_CUT)
    g = geometry_of(case)
    want = gpu_phasor_forward_project(case).reshape(8, 8, 28)
    v = torch.from_numpy(case["volume"])
    z = torch.view_as_complex(v)
    strided = torch.empty((2, 6, 6, 6), dtype=torch.float32).permute(1, 2, 3, 0)
    strided.copy_(v)
    assert not strided.is_contiguous()
    for form in (TensorXf(v.cuda()), case["volume"], v, v.cuda(), v.double(), strided, z, z.cuda(), z.numpy(), z.to(torch.complex128)):
        got = phasor_forward_project(form, g, case["freq"], case["vmin"], case["vmax"], weights=case["weights"], window=WINDOW_CUT["window"])
        assert got.is_cuda and got.dtype == torch.complex64 and tuple(got.shape) == (8, 8, 28) and got.grad_fn is None
        assert np.array_equal(got.cpu().numpy().astype(np.complex128), want)
    # a real (nz, ny, nx) volume: zero imaginary part
    real = with_volume(case, np.stack([case["volume"][..., 0], np.zeros((6, 6, 6), np.float32)], axis=-1))
    got = phasor_forward_project(case["volume"][..., 0], g, case["freq"], case["vmin"], case["vmax"], weights=case["weights"],
                                 window=WINDOW_CUT["window"])
    assert np.array_equal(got.cpu().numpy().astype(np.complex128).reshape(64, 28), gpu_phasor_forward_project(real))
    # a ragged (nx, ny, nz): the resolution comes from the shape
    c2 = tiny_case(SINGLE, offsets=True, res=(5, 3, 7))
    assert c2["volume"].shape == (7, 3, 5, 2)
    got = phasor_forward_project(c2["volume"], geometry_of(c2), c2["freq"], c2["vmin"], c2["vmax"])
    assert np.array_equal(got.cpu().numpy().astype(np.complex128).reshape(64, 28), gpu_phasor_forward_project(c2))


def test_exhaustive_tensor_layout():
    """the rows (s, l = laser_x * Ly + laser_y) of the C-ABI come back as (H, W, Lx, Ly, F)"""
    from mitransient_amd.nlos import phasor_forward_project
    case = tiny_case(EXHAUSTIVE, offsets=True, weights=np.linspace(0.5, 1.5, 28))
    got = phasor_forward_project(case["volume"], geometry_of(case, (3, 2)), case["freq"], case["vmin"], case["vmax"], weights=case["weights"])
    assert tuple(got.shape) == (8, 8, 3, 2, 28)
    direct = gpu_phasor_forward_project(case)
    got = got.cpu().numpy().astype(np.complex128)
    for s in range(64):
        for lx in range(3):
            for ly in range(2):
                assert np.array_equal(got[s // 8, s % 8, lx, ly], direct[s * 6 + lx * 2 + ly])
    assert rel_l2(got.reshape(384, 28), reference(case)) <= PB_TOL
    with pytest.raises(ValueError):
        phasor_forward_project(case["volume"], geometry_of(case), case["freq"], case["vmin"], case["vmax"])


def test_invalid_descriptions_leave_the_phasors_untouched():
    import torch
    from mitransient_amd.runtime import get_context
    good, bad = bad_descriptions()
    ctx = get_context()
    zeros = np.zeros((6, 6, 6, 2), np.float32)
    for c in bad:
        assert np.isnan(gpu_phasor_forward_project(with_volume(c, zeros), expect=-1)).all()
        assert b"mtr_phasor_forward_project" in ctx.lib.mtr_last_error(ctx.handle)
    out = torch.full((64, 28, 2), float("nan"), device="cuda")
    dev = [torch.from_numpy(good[k]).cuda() for k in KEYS] + [torch.from_numpy(zeros).cuda()]
    u, q = C.c_void_p(dev[5].data_ptr()), C.c_void_p(out.data_ptr())
    call = ctx.lib.mtr_phasor_forward_project
    for k in range(5):
        ptrs = [t.data_ptr() for t in dev[:5]]
        ptrs[k] = None
        d = desc_of(good, *ptrs, None)
        assert call(ctx.handle, C.byref(d), u, q) == -1
        assert b"mtr_phasor_forward_project" in ctx.lib.mtr_last_error(ctx.handle)
    d = desc_of(good, *(t.data_ptr() for t in dev[:5]), None)
    assert call(ctx.handle, C.byref(d), None, q) == -1 and call(ctx.handle, C.byref(d), u, None) == -1
    assert call(ctx.handle, None, u, q) == -1
    assert call(ctx.handle, C.byref(d), C.c_void_p(dev[5].data_ptr() + 4), q) == -1            # 8-byte alignment of both tensors
    assert call(ctx.handle, C.byref(d), u, C.c_void_p(out.data_ptr() + 4)) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------- phasor_reconstruct_cgls
def test_cgls_recovers_a_synthetic_patch():
    """the yardstick is phasor_forward_project_cases' CGLS in f64 on the dense operator: |r_10| / |y| = 4.6e-3 there; f32 noise is
    two orders below a residual of that size, so 2 x holds and a wrong adjoint does not.  Measured on the MI355X: 7.84e-3 — the host
    builds give the same figure on the CPU: the f32 phase rounding of the operator, not summation noise (HISTORY.md)"""
    import torch
    from mitransient_amd.nlos import phasor_reconstruct_cgls
    case, x_true = fc.cgls_case()
    y = gpu_phasor_forward_project(with_volume(case, np.stack([x_true, np.zeros_like(x_true)], axis=-1))).reshape(8, 8, 28)
    g = geometry_of(case)
    x, residuals = phasor_reconstruct_cgls(y, g, case["freq"], case["vmin"], case["vmax"], 6, iterations=10)
    assert x.is_cuda and x.dtype == torch.complex64 and tuple(x.shape) == (6, 6, 6) and x.grad_fn is None
    assert len(residuals) == 11 and residuals[0] == 1.0 and all(type(r) is float for r in residuals)
    print("residuals:", " ".join(f"{r:.3e}" for r in residuals))
    assert residuals[10] <= 2.0 * fc.CGLS_R10
    assert all(b <= a for a, b in zip(residuals, residuals[1:]))
    iz, iy, ix = np.unravel_index(int(np.argmax(np.abs(x.cpu().numpy()))), (6, 6, 6))
    assert iz == 3 and iy in (2, 3) and ix in (2, 3)
    # the real view of the same phasors: the same bits; phasors that are all zero: a zero volume
    x2, r2 = phasor_reconstruct_cgls(pairs_of(y), g, case["freq"], case["vmin"], case["vmax"], 6, iterations=10)
    assert np.array_equal(x2.cpu().numpy(), x.cpu().numpy()) and r2 == residuals
    z, rz = phasor_reconstruct_cgls(np.zeros_like(y), g, case["freq"], case["vmin"], case["vmax"], 6, iterations=2)
    assert not z.cpu().numpy().any() and rz == [1.0, 1.0, 1.0]


def test_cgls_on_the_rendered_quad():
    """render a quad at z = 1 into a phasor film, fit a volume with five CGLS iterations: the depth profile of |x| peaks at z = 1"""
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    try:
        scene = pc.e2e_scene("confocal")
        mi.set_variant("llvm_ad_mono")
        _, phasors = mi.render(scene, spp=64, seed=0)
        g, film = mitr.nlos.capture_geometry(scene), scene.sensors()[0].film()
    finally:
        mi.set_variant("llvm_ad_rgb")
    x, residuals = mitr.nlos.phasor_reconstruct_cgls(phasors, g, film, *E2E_BOX, iterations=5)
    z, prof = depth_peak(x.cpu().numpy())
    print("depth profile of |x| peaks at z =", z, "residuals:", " ".join(f"{r:.3e}" for r in residuals))
    assert prof.max() > 0 and abs(z - 1.0) <= 1.0 / 16.0, (z, prof)
    assert residuals[5] < residuals[0]
