"""nlos.phasor_backproject on the GPU: the kernels of mtr_phasor_backproject.hip against the host build of the same arithmetic
(tests/host_phasor_backproject.cpp) and against numpy f64, the kernels' own edges (ragged tiles, one and many scan points, the
anchor block's edges, both forms, weights NULL and given, the slab path, the window), render -> reconstruct -> depth peak end to
end, the input forms and the C-ABI's refusals."""
import ctypes as C

import numpy as np
import pytest

import phasor_backproject_cases as pc
from phasor_backproject_cases import (CONFOCAL, E2E, E2E_BOX, EXHAUSTIVE, FLT_MAX, PARITY, PB_TOL, SINGLE, depth_peak, desc_of,
                                      host_phasor_backproject, make_case, parity_case, reference, rel_l2, tiny_case, wall_points,
                                      with_form)
from test_phasor_backproject import WINDOW_CUT, bad_descriptions, parity_reference

pytestmark = pytest.mark.gpu
KEYS = ("sp", "lp", "so", "lo", "freq")


def gpu_phasor_backproject(case, expect=0, fill=None):
    """mtr_phasor_backproject through the C-ABI on the arrays of a case: complex (nz, ny, nx) — or, refused, the (nz, ny, nx, 2) f32"""
    import torch
    from mitransient_amd.runtime import get_context
    ctx = get_context()
    dev = [torch.from_numpy(case[k]).cuda() for k in KEYS + ("phasors",)]
    w = None if case["weights"] is None else torch.from_numpy(case["weights"]).cuda()
    nx, ny, nz = case["res"]
    vol = torch.full((nz, ny, nx, 2), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    d = desc_of(case, *(t.data_ptr() for t in dev[:5]), None if w is None else w.data_ptr())
    ctx.bind_current_stream()
    rc = ctx.lib.mtr_phasor_backproject(ctx.handle, C.byref(d), C.c_void_p(dev[5].data_ptr()), C.c_void_p(vol.data_ptr()))
    torch.cuda.synchronize()
    assert rc == expect, (rc, ctx.lib.mtr_last_error(ctx.handle))
    return pc.as_complex(vol.cpu().numpy()) if expect == 0 else vol.cpu().numpy()


def plan(case):
    """(tiles, slabs) mtr_phasor_backproject chooses for a case on this device (bp_plan, mtr_backproject.h)"""
    import torch
    from mitransient_amd import _cabi
    out = (C.c_uint32 * 4)()
    lib = _cabi.load_library()
    lib.mtr_test_backproject_plan.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    rows = case["phasors"].shape[0]
    assert lib.mtr_test_backproject_plan(*case["res"], rows, torch.cuda.get_device_properties(0).multi_processor_count, out) == 1
    return out[0], out[1]


def check(case, ref=None):
    got, host = gpu_phasor_backproject(case), host_phasor_backproject(case)
    ref = reference(case) if ref is None else ref
    assert np.abs(ref).max() > 0
    eh, er = rel_l2(got, host), rel_l2(got, ref)
    print(f"rel-L2 against the host build {eh:.3e}, against f64 {er:.3e}")
    assert eh <= PB_TOL and er <= PB_TOL, (eh, er)
    return got


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("kind,offsets,F,weights", PARITY)
def test_kernel_matches_host_build_and_f64(kind, offsets, F, weights):
    ref = parity_reference(kind, offsets, F, weights)
    for form in ("uniform", "table"):
        case = parity_case(kind, offsets, F, weights, form)
        got = check(case, ref)
        assert np.array_equal(got, gpu_phasor_backproject(case))          # the same call twice: equal bits
    assert plan(case) == (2, 6 if kind == EXHAUSTIVE else 1)               # 64 pairs: one slab; Exhaustive's 384: six of 64


# ---------------------------------------------------------------- the kernels' edges
@pytest.mark.parametrize("res", [(5, 3, 7), (9, 17, 5)])
def test_ragged_tiles(res):
    for kind, form, weights in ((CONFOCAL, "uniform", "gaussian"), (EXHAUSTIVE, "table", None)):
        check(tiny_case(kind, offsets=True, form=form, weights=weights, res=res))


@pytest.mark.parametrize("n", [1, 65])
def test_scan_point_counts(n):
    sp = wall_points(n, 1) if n > 1 else np.array([[0.25, -0.25, 0.0]], np.float32)
    for kind, form, weights in ((CONFOCAL, "uniform", None), (SINGLE, "table", "gaussian"), (SINGLE, "uniform", "gaussian")):
        lp = sp if kind == CONFOCAL else np.array([[0.0, 0.5, 0.0]], np.float32)
        check(make_case(kind, sp, lp, offsets=True, form=form, weights=weights))


@pytest.mark.parametrize("F", [1, 16, 17, 151])
def test_anchor_block_edges(F):
    for kind in (CONFOCAL, EXHAUSTIVE):
        for weights in (None, np.linspace(0.5, 1.5, F)):
            case = tiny_case(kind, F=F, offsets=True, weights=weights)
            assert (case["freq_step"] > 0) == (F > 1)
            ref = reference(case)
            got, table = check(case, ref), check(with_form(case, "table"), ref)
            assert rel_l2(got, table) <= PB_TOL
            if F == 1:
                assert np.array_equal(got, table)


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_slab_path(kind):
    """2 x 2 x 2 voxels against a 32 x 32 scan: the pairs are split over workgroups and the complex planes added in slab order"""
    sp = wall_points(32, 32)
    lp = sp if kind == CONFOCAL else (np.zeros((1, 3), np.float32) if kind == SINGLE else wall_points(2, 3).reshape(-1, 3))
    for form, weights in (("uniform", "gaussian"), ("table", None)):
        case = make_case(kind, sp, lp, res=(2, 2, 2), offsets=True, form=form, weights=weights)
        tiles, slabs = plan(case)
        assert tiles == 1 and slabs > 1
        got = check(case)
        assert np.array_equal(got, gpu_phasor_backproject(case))
    # a one-slab call on the same voxels: 9 (Exhaustive: 54) pairs are not worth splitting
    case = make_case(kind, wall_points(3, 3), wall_points(3, 3) if kind == CONFOCAL else lp, res=(2, 2, 2), offsets=True, weights="gaussian")
    assert plan(case) == (1, 1)
    check(case)


def test_window():
    film = pc.FILMS[28]
    capture = (np.float32(0.0), np.float32(film["temporal_bins"] * film["bin_width_opl"]))
    for kind in (CONFOCAL, SINGLE, EXHAUSTIVE):
        for form in ("uniform", "table"):
            case = tiny_case(kind, form=form, window=capture, vmin=(100, 100, 100), vmax=(102, 102, 101))
            assert np.array_equal(gpu_phasor_backproject(case), np.zeros((6, 6, 6)))
            case = tiny_case(kind, form=form, weights="gaussian", vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
            assert case["tau_max"] == FLT_MAX
            assert np.array_equal(gpu_phasor_backproject(case), np.zeros((6, 6, 6)))
            case = tiny_case(kind, weights="gaussian", form=form, **WINDOW_CUT)
            assert np.array_equal(pc.in_window(case, np.float32), pc.in_window(case, np.float64))
            check(case)


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def renders():
    """(name, mode) -> (geometry, film, the phasors mi.render returned): rendered once, in the mono variant"""
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    out = {}
    try:
        for name in sorted(E2E):
            for mode, number in (("wavefront", 2), ("auto", 0)):      # MTR_MODE_WAVEFRONT, MTR_MODE_AUTO
                scene = pc.e2e_scene(name)
                mi.set_variant("llvm_ad_mono")
                scene.integrator().mode = number
                _, phasors = mi.render(scene, spp=64, seed=0)
                out[name, mode] = (mitr.nlos.capture_geometry(scene), scene.sensors()[0].film(), phasors)
    finally:
        mi.set_variant("llvm_ad_rgb")
    return out


@pytest.mark.parametrize("mode", ["wavefront", "auto"])
@pytest.mark.parametrize("name", sorted(E2E))
def test_rendered_quad_reconstructs_at_its_depth(renders, name, mode):
    import torch
    import mitransient_amd as mitr
    g, film, phasors = renders[name, mode]
    assert phasors.shape == (16, 16, 28, 2)
    for weights in (None, "gaussian"):
        vol = mitr.nlos.phasor_backproject(phasors, g, film, *E2E_BOX, weights=weights)
        assert vol.is_cuda and vol.dtype == torch.complex64 and tuple(vol.shape) == (16, 16, 16) and not vol.requires_grad
        z, prof = depth_peak(vol.cpu().numpy())
        print(name, mode, weights, "depth profile of |V| peaks at z =", z)
        assert prof.max() > 0 and abs(z - 1.0) <= 1.0 / 16.0, (z, prof)


# ---------------------------------------------------------------- input forms and the C-ABI
def test_input_forms(renders):
    import torch
    from mitransient_amd.nlos import phasor_backproject
    g, film, phasors = renders["confocal", "auto"]
    t = phasors.torch()

    def run(p, frequencies=film, box=E2E_BOX, **kw):
        return phasor_backproject(p, g, frequencies, *box, **kw).cpu().numpy()
    want = run(t, weights="gaussian", window="capture")
    assert np.abs(want).max() > 0
    strided = torch.empty((2, 16, 28, 16), dtype=t.dtype, device=t.device).permute(1, 3, 2, 0)
    strided.copy_(t)
    assert not strided.is_contiguous()
    z = torch.view_as_complex(t.contiguous())
    assert z.shape == (16, 16, 28)
    for other in (phasors, np.array(phasors), t.double(), t.cpu(), strided, z, z.cpu().numpy(), z.to(torch.complex128)):
        assert np.array_equal(want, run(other, weights="gaussian", window="capture"))
    # a film object against a plain frequency list (gaussian weights then come as an array), the window spelled out
    w = np.exp(-0.5 * ((film.frequencies_f32.astype(np.float64) - 1.0 / film.wl_mean) * (6.0 * film.wl_sigma)) ** 2)
    assert np.array_equal(want, run(t, frequencies=[float(f) for f in film.frequencies_f32], weights=w, window=(0.0, 256 * 0.02)))
    assert np.array_equal(run(t), run(t, frequencies=film.frequencies_f32))
    assert not np.array_equal(want, run(t))
    assert run(t, box=(E2E_BOX[0], E2E_BOX[1], (5, 3, 7))).shape == (7, 3, 5)
    # the python surface against the C-ABI called directly on the same numbers
    for weights in (None, "gaussian"):
        case = make_case(g.capture_type, g.sensor_points, g.laser_points, F=28, start=g.start_opl, vmin=E2E_BOX[0], vmax=E2E_BOX[1],
                         res=(16,) * 3, phasors=t.cpu().numpy().reshape(256, 28, 2), weights=weights)
        assert np.array_equal(case["freq"], film.frequencies_f32) and case["freq_step"] > 0
        assert np.array_equal(run(t, weights=weights).astype(np.complex128), gpu_phasor_backproject(case))


def test_exhaustive_tensor_layout():
    """an (H, W, Lx, Ly, F, 2) tensor is read as rows (s, l = laser_x * Ly + laser_y)"""
    import torch
    from mitransient_amd.nlos import CaptureGeometry, phasor_backproject
    case = tiny_case(EXHAUSTIVE, offsets=True, weights=np.linspace(0.5, 1.5, 28))
    g = CaptureGeometry(EXHAUSTIVE, case["sp"].reshape(8, 8, 3), case["lp"], case["so"].reshape(8, 8), case["lo"], float(case["start"]),
                        0.02, 256, (3, 2))
    t6 = torch.from_numpy(case["phasors"].reshape(8, 8, 3, 2, 28, 2)).cuda()
    vol = phasor_backproject(t6, g, case["freq"], case["vmin"], case["vmax"], 6, weights=case["weights"])
    want = gpu_phasor_backproject(case)
    assert np.array_equal(vol.cpu().numpy().astype(np.complex128), want)
    assert np.array_equal(phasor_backproject(torch.view_as_complex(t6), g, case["freq"], case["vmin"], case["vmax"], 6,
                                             weights=case["weights"]).cpu().numpy().astype(np.complex128), want)


def test_invalid_descriptions_leave_the_volume_untouched():
    import torch
    from mitransient_amd.runtime import get_context
    good, bad = bad_descriptions()
    ctx = get_context()
    for c in bad:
        assert np.all(gpu_phasor_backproject(c, expect=-1, fill=7.0) == 7.0)
        assert b"mtr_phasor_backproject" in ctx.lib.mtr_last_error(ctx.handle)
    # NULL pointers (weights alone may be NULL)
    vol = torch.full((6, 6, 6, 2), 7.0, device="cuda")
    dev = [torch.from_numpy(good[k]).cuda() for k in KEYS + ("phasors",)]
    ph, out = C.c_void_p(dev[5].data_ptr()), C.c_void_p(vol.data_ptr())
    for k in range(5):
        ptrs = [t.data_ptr() for t in dev[:5]]
        ptrs[k] = None
        d = desc_of(good, *ptrs, None)
        assert ctx.lib.mtr_phasor_backproject(ctx.handle, C.byref(d), ph, out) == -1
        assert b"mtr_phasor_backproject" in ctx.lib.mtr_last_error(ctx.handle)
    d = desc_of(good, *(t.data_ptr() for t in dev[:5]), None)
    assert ctx.lib.mtr_phasor_backproject(ctx.handle, C.byref(d), None, out) == -1
    assert ctx.lib.mtr_phasor_backproject(ctx.handle, C.byref(d), ph, None) == -1
    assert ctx.lib.mtr_phasor_backproject(ctx.handle, None, ph, out) == -1
    torch.cuda.synchronize()
    assert bool((vol == 7.0).all())
