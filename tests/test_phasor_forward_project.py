"""nlos.phasor_forward_project on the CPU: the host build of mtr_phasor_forward_project.h
(tests/host_phasor_forward_project.cpp) against an independent numpy f64 restatement in both forms, the numpy f32 restatement
against the bar on its own, the exact one-term identity with the host build of mtr_phasor_backproject.h, the adjoint identity
between the two host builds, the edges (frequency blocks, scan-point counts, volumes, the window, a NaN voxel), pf_plan, the
refusals, the additive C-ABI, the Python refusals that need no GPU, and CGLS in f64 on the dense operator — the yardstick of the
GPU test of phasor_reconstruct_cgls."""
import ctypes as C
import functools

import numpy as np
import pytest

import phasor_backproject_cases as pc
import phasor_forward_project_cases as fc
from phasor_backproject_cases import CONFOCAL, EXHAUSTIVE, FLT_MAX, PARITY, PB_TOL, SINGLE, host_phasor_backproject, wall_points
from phasor_forward_project_cases import (adjoint_gap, host_phasor_forward_project, make_case, one_hot_phasors, one_hot_volume,
                                          parity_case, reference, reference_f32, rel_l2, rows_of, tiny_case, with_form)
from test_phasor_backproject import WINDOW_CUT, bad_descriptions


@functools.lru_cache(maxsize=None)
def parity_reference(kind, offsets, F, weights):
    """the f64 phasors of a parity case (the form does not enter them), computed once"""
    ref = reference(parity_case(kind, offsets, F, weights))
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------- the host build against numpy f64
@pytest.mark.parametrize("kind,offsets,F,weights", PARITY)
def test_host_build_matches_f64(kind, offsets, F, weights):
    ref = parity_reference(kind, offsets, F, weights)
    assert np.abs(ref).min() > 0
    got = {}
    for form in ("uniform", "table"):
        case = parity_case(kind, offsets, F, weights, form)
        assert (case["freq_step"] > 0) == (form == "uniform")
        got[form] = host_phasor_forward_project(case)
        e = rel_l2(got[form], ref)
        print(f"{kind} offsets={offsets} F={F} weights={weights} {form}: rel-L2 {e:.3e}")
        assert e <= PB_TOL, e
        assert np.array_equal(got[form], host_phasor_forward_project(case))
    assert rel_l2(got["uniform"], got["table"]) <= PB_TOL


def test_f32_restatement_is_within_the_bar():
    """the tolerance holds for the reference alone, with room: numpy in f32 (the header's operation order, both forms) against
    f64 stays below PB_TOL / 4"""
    worst = 0.0
    for kind, offsets, F, weights in PARITY:
        for form in ("uniform", "table"):
            e = rel_l2(reference_f32(parity_case(kind, offsets, F, weights, form)), parity_reference(kind, offsets, F, weights))
            worst = max(worst, e)
    print(f"worst rel-L2 of the f32 restatement: {worst:.3e}")
    assert worst <= fc.F32_WORST


# ---------------------------------------------------------------- bit-identical factors
@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_one_term_identity_is_exact(kind):
    """U = 1 in one voxel: Q[p, k] is conj(z(v0, p, k)); P = 1 in one (p, k): V(v0) is z(v0, p, k) — both are fmaf(1, z, 0)
    chains over the same z, so the two host builds agree as numbers, in both forms"""
    v0 = (4, 1, 3)
    for form in ("uniform", "table"):
        base = with_form(pc.tiny_case(kind, F=151, offsets=True), form)
        assert base["weights"] is None and base["tau_max"] == FLT_MAX
        q = host_phasor_forward_project(fc.with_volume(base, one_hot_volume(base, v0)))
        for p in (5, rows_of(base) - 2):
            for k in (0, 15, 16, 17, 150):
                c = dict(base)
                c["phasors"] = one_hot_phasors(base, p, k)
                v = host_phasor_backproject(c)[v0[2], v0[1], v0[0]]
                assert v != 0 and q[p, k] == np.conj(v), (form, p, k, q[p, k], v)


# ---------------------------------------------------------------- the adjoint identity between the two host builds
def test_adjoint_identity_between_the_host_builds():
    """|<A y, x> - <y, A^H x>| <= 1e-5 (|Ay| |x| + |y| |A^H x|) over the parity grid and with the window that cuts the box.
    Measured: the largest gap is 1.2e-2 of the bound, i.e. 1.2e-7 of the norms' product (printed)."""
    cases = [parity_case(k, o, F, w, form) for k, o, F, w in PARITY for form in ("uniform", "table")]
    cases += [tiny_case(k, weights="gaussian", form=form, **WINDOW_CUT) for k in (CONFOCAL, SINGLE, EXHAUSTIVE) for form in ("uniform", "table")]
    worst = 0.0
    for c in cases:
        Ay, AHx = host_phasor_backproject(c), host_phasor_forward_project(c)
        x, y = fc.volume_complex(c), fc.as_complex(c["phasors"])
        gap, bound = adjoint_gap(Ay, x, y, AHx)
        worst = max(worst, gap / bound)
        assert gap <= bound, (c["capture_type"], c["F"], float(c["freq_step"]), gap, bound)
    print(f"largest gap / bound: {worst:.3e}")


# ---------------------------------------------------------------- edges
def check(case):
    got, ref = host_phasor_forward_project(case), reference(case)
    assert np.abs(ref).max() > 0
    e = rel_l2(got, ref)
    assert e <= PB_TOL, e
    return got


@pytest.mark.parametrize("F", [1, 16, 17])
def test_frequency_block_edges(F):
    for kind in (CONFOCAL, EXHAUSTIVE):
        for weights in (None, np.linspace(0.5, 1.5, F)):
            case = tiny_case(kind, F=F, offsets=True, weights=weights)
            assert (case["freq_step"] > 0) == (F > 1)
            got, table = check(case), check(with_form(case, "table"))
            if F == 1:
                assert np.array_equal(got, table)


@pytest.mark.parametrize("n", [1, 65])
def test_scan_point_counts(n):
    sp = wall_points(n, 1) if n > 1 else np.array([[0.25, -0.25, 0.0]], np.float32)
    for kind, form, weights in ((CONFOCAL, "uniform", None), (SINGLE, "table", "gaussian"), (SINGLE, "uniform", "gaussian")):
        lp = sp if kind == CONFOCAL else np.array([[0.0, 0.5, 0.0]], np.float32)
        assert check(make_case(kind, sp, lp, offsets=True, form=form, weights=weights)).shape == (n, 28)


@pytest.mark.parametrize("res", [(5, 3, 7), (1, 1, 1)])
def test_volume_shapes(res):
    for kind, form, weights in ((CONFOCAL, "uniform", "gaussian"), (EXHAUSTIVE, "table", None)):
        check(tiny_case(kind, offsets=True, form=form, weights=weights, res=res))


def test_boxes_beyond_the_window_give_exact_zeros():
    film = pc.FILMS[28]
    capture = (np.float32(0.0), np.float32(film["temporal_bins"] * film["bin_width_opl"]))      # window="capture"
    for kind in (CONFOCAL, SINGLE, EXHAUSTIVE):
        for form in ("uniform", "table"):
            case = tiny_case(kind, form=form, window=capture, vmin=(100, 100, 100), vmax=(102, 102, 101))
            assert np.array_equal(host_phasor_forward_project(case), np.zeros((rows_of(case), 28)))
            case = tiny_case(kind, form=form, weights="gaussian", vmin=(3e38, -1, 0.5), vmax=(3.2e38, 1, 1.5))
            assert case["tau_min"] == -FLT_MAX and case["tau_max"] == FLT_MAX
            assert np.array_equal(host_phasor_forward_project(case), np.zeros((rows_of(case), 28)))


@pytest.mark.parametrize("kind", [CONFOCAL, SINGLE, EXHAUSTIVE])
def test_window_that_cuts_through_the_box(kind):
    for form in ("uniform", "table"):
        case = tiny_case(kind, weights="gaussian", form=form, **WINDOW_CUT)
        m32, m64 = pc.in_window(case, np.float32), pc.in_window(case, np.float64)
        assert np.array_equal(m32, m64) and 0.2 < m64.mean() < 0.8
        check(case)
        # a NaN in one voxel reaches exactly the rows whose window contains that voxel
        v0 = (2, 3, 1)
        lin = (v0[2] * 6 + v0[1]) * 6 + v0[0]
        reached = m64[lin]
        assert reached.any() and not reached.all()
        vol = case["volume"].copy()
        vol[v0[2], v0[1], v0[0], 0] = np.nan
        got = host_phasor_forward_project(fc.with_volume(case, vol))
        assert np.array_equal(np.isnan(got).all(axis=1), reached) and np.array_equal(np.isnan(got).any(axis=1), reached)


# ---------------------------------------------------------------- pf_plan
def test_plan():
    from mitransient_amd import _cabi
    lib = C.CDLL(_cabi.LIB_PATH)
    lib.mtr_test_phasor_forward_project_plan.argtypes = fc.PLAN_ARGS
    host = fc.host_lib().hpf_plan
    for kind in (CONFOCAL, SINGLE, EXHAUSTIVE):
        for F, blocks in ((1, 1), (16, 1), (17, 2), (28, 2), (151, 10)):
            rows = 384 if kind == EXHAUSTIVE else 64
            assert fc.plan_of(host, 6, 6, 6, rows, F, 256) == (blocks, 1, 216)          # the tiny cases: one slab
    assert fc.plan_of(host, 6, 6, 6, 65, 28, 256) == (2, 1, 216)
    # 2 rows against 32 x 32 x 16 voxels: the voxels are cut, the slabs cover them exactly
    for rows in (2, 12):
        blocks, slabs, slab_len = fc.plan_of(host, 32, 32, 16, rows, 28, 256)
        assert blocks == 2 and slabs > 1 and (slabs - 1) * slab_len < 32 * 32 * 16 <= slabs * slab_len
    # many rows: one slab whatever the volume
    assert fc.plan_of(host, 128, 128, 128, 65536, 28, 256) == (2, 1, 128 ** 3)
    # zero sizes, and counts the grid cannot index
    for args in ((0, 32, 16, 2, 28, 256), (32, 0, 16, 2, 28, 256), (32, 32, 0, 2, 28, 256), (32, 32, 16, 0, 28, 256),
                 (32, 32, 16, 2, 0, 256), (32, 32, 16, 2, 28, 0), (2048, 2048, 512, 2, 28, 256), (6, 6, 6, 2 ** 31, 28, 256),
                 (6, 6, 6, 2 ** 30, 151, 256)):
        assert fc.plan_of(host, *args) is None and fc.plan_of(lib.mtr_test_phasor_forward_project_plan, *args) is None
    # the library's hook agrees with the host's plan
    for args in ((6, 6, 6, 64, 28, 256), (32, 32, 16, 2, 28, 256), (32, 32, 16, 12, 151, 304), (128, 128, 128, 3, 28, 256),
                 (5, 3, 7, 1, 1, 64), (1024, 1024, 1024, 1, 4096, 256)):
        assert fc.plan_of(host, *args) == fc.plan_of(lib.mtr_test_phasor_forward_project_plan, *args) is not None


# ---------------------------------------------------------------- refusals
def test_invalid_descriptions_leave_the_phasors_untouched():
    good, bad = bad_descriptions()
    lib = fc.host_lib()
    for c in bad:
        out = host_phasor_forward_project(fc.with_volume(c, np.zeros((6, 6, 6, 2))), expect=-1, fill=np.nan)
        assert np.isnan(out).all()
    out = np.full((64, 28, 2), np.nan, np.float32)
    vol = np.zeros((6, 6, 6, 2), np.float32)
    ptrs = [good[k].ctypes.data for k in ("sp", "lp", "so", "lo", "freq")]
    u, q = C.c_void_p(vol.ctypes.data), C.c_void_p(out.ctypes.data)
    d = pc.desc_of(good, *ptrs, None)
    assert lib.hpf_check(C.byref(d), u, q) == b""
    for k in range(5):
        broken = list(ptrs)
        broken[k] = None
        d = pc.desc_of(good, *broken, None)
        assert b"NULL" in lib.hpf_check(C.byref(d), u, q)
        assert lib.hpf_forward_project(C.byref(d), u, q) == -1
    d = pc.desc_of(good, *ptrs, None)
    assert lib.hpf_forward_project(C.byref(d), None, q) == -1 and lib.hpf_forward_project(C.byref(d), u, None) == -1
    assert lib.hpf_forward_project(None, u, q) == -1
    # both tensors are (Re, Im) pairs, 8-byte aligned
    for a, b in ((vol.ctypes.data + 4, out.ctypes.data), (vol.ctypes.data, out.ctypes.data + 4)):
        assert b"aligned" in lib.hpf_check(C.byref(d), C.c_void_p(a), C.c_void_p(b))
        assert lib.hpf_forward_project(C.byref(d), C.c_void_p(a), C.c_void_p(b)) == -1
    assert np.isnan(out).all()
    assert lib.hpf_forward_project(C.byref(d), u, q) == 0 and np.all(out == 0)


def test_abi_is_additive():
    from mitransient_amd import _cabi
    assert _cabi.MTR_ABI_VERSION == 24
    assert "mtr_phasor_forward_project" in _cabi.EXPORTS
    lib = C.CDLL(_cabi.LIB_PATH)
    assert hasattr(lib, "mtr_phasor_forward_project") and hasattr(lib, "mtr_test_phasor_forward_project_plan")
    lib.mtr_abi_version.restype = C.c_int
    assert lib.mtr_abi_version() == 24
    header = open(pc.ROOT + "/include/mitransient_amd.h").read()
    assert "int  mtr_phasor_forward_project(mtr_ctx *, const mtr_phasor_backproject_desc *, const float *volume_dev, float *phasors_dev);" in header


def test_python_validates_before_touching_the_gpu(monkeypatch):
    import mitransient_amd as mitr
    from mitransient_amd import runtime
    from mitransient_amd.nlos import CaptureGeometry, phasor_forward_project, phasor_reconstruct_cgls

    def no_context(*a, **k):
        raise AssertionError("the context was asked for before the arguments were checked")
    monkeypatch.setattr(runtime, "get_context", no_context)
    sp = wall_points(4, 2).astype(np.float64)
    g = CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16)
    gx = CaptureGeometry(EXHAUSTIVE, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16)
    gx_bad = CaptureGeometry(EXHAUSTIVE, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), 1.2, 0.04, 16, (3, 2))
    box = ((-1, -1, 0.5), (1, 1, 1.5))
    f = [1.0, 1.5, 2.0]
    ok = np.zeros((4, 4, 4), np.complex64)
    for volume, geom, freq, args, kw in (
            (np.zeros((4, 4), np.float32), g, f, box, {}),                                # wrong rank
            (np.zeros((4, 4, 4, 2, 1), np.float32), g, f, box, {}),
            (np.zeros((4, 4, 4, 3), np.float32), g, f, box, {}),                          # a real 4-d volume without a (Re, Im) axis
            (np.zeros((4, 4, 4, 2), np.complex64), g, f, box, {}),                        # complex with one
            (np.zeros((4, 0, 4), np.float32), g, f, box, {}),
            (ok, gx, f, box, {}),                                                         # Exhaustive without laser_grid
            (ok, gx_bad, f, box, {}),                                                     # ... and with one that does not match
            (ok, g, [], box, {}),
            (ok, g, [1.0, np.inf], box, {}),
            (ok, g, f, ((-1, -1, 0.5), (1, 1, 0.5)), {}),                                 # empty box
            (ok, g, f, box, {"weights": [1.0, 1.0]}),                                     # bad weights
            (ok, g, f, box, {"weights": "gaussian"}),                                     # needs a film
            (ok, g, f, box, {"weights": "hann"}),
            (ok, g, f, box, {"window": (2.0, 1.0)}),                                      # bad window
            (ok, g, f, box, {"window": "film"}),
            (ok, CaptureGeometry(CONFOCAL, sp, sp.reshape(-1, 3), np.zeros((2, 4)), np.zeros(8), np.inf, 0.04, 16), f, box, {}),
            (ok, CaptureGeometry(SINGLE, sp, sp.reshape(-1, 3)[:2], np.zeros((2, 4)), np.zeros(2), 1.2, 0.04, 16), f, box, {}),
            (ok, "geometry", f, box, {})):
        with pytest.raises(ValueError, match="phasor_forward_project"):
            phasor_forward_project(volume, geom, freq, *args, **kw)
    ph = np.zeros((2, 4, 3, 2), np.float32)
    for phasors, freq, kw in ((ph, f, {"iterations": 0}), (ph, f, {"iterations": 2.5}), (ph, f, {"iterations": True}),
                              (np.zeros((2, 4, 4, 2), np.float32), f, {}),                # frequency-count mismatch
                              (np.zeros((2, 4, 3), np.float32), f, {}),                   # wrong rank
                              (ph, f, {"weights": [1.0]}), (ph, f, {"window": (2.0, 1.0)})):
        with pytest.raises(ValueError, match="phasor_reconstruct_cgls"):
            phasor_reconstruct_cgls(phasors, g, freq, *box, 4, **kw)
    assert mitr.nlos.phasor_forward_project is phasor_forward_project and mitr.nlos.phasor_reconstruct_cgls is phasor_reconstruct_cgls
    monkeypatch.undo()
    import torch
    if not torch.cuda.is_available():           # a valid call without a GPU: the product has no CPU path
        from mitransient_amd._cabi import MitransientAMDError
        with pytest.raises(MitransientAMDError):
            phasor_forward_project(ok, g, f, *box)


# ---------------------------------------------------------------- CGLS in f64 on the dense operator
def test_cgls_on_the_dense_operator():
    """the yardstick of the GPU test: phasors of a 2 x 2 patch at iz = 3, CGLS in numpy f64 on the dense A^H"""
    case, x_true = fc.cgls_case()
    M = fc.dense_operator(case)
    # the dense matrix is the operator the host build computes
    c = fc.with_volume(case, np.stack([x_true, np.zeros_like(x_true)], axis=-1))
    y = M @ x_true.reshape(-1)
    assert rel_l2(host_phasor_forward_project(c), y.reshape(64, 28)) <= PB_TOL
    x, residuals = fc.cgls_dense(M, y, 20)
    err = np.linalg.norm(x - x_true.reshape(-1)) / np.linalg.norm(x_true)
    cond = np.linalg.cond(M)
    print(f"|r_10| / |y| = {residuals[10]:.3e}, |r_20| / |y| = {residuals[20]:.3e}, volume to {err:.3e}, condition number {cond:.3f}")
    assert residuals[10] == pytest.approx(fc.CGLS_R10, rel=0.02) and residuals[20] == pytest.approx(fc.CGLS_R20, rel=0.05)
    assert err == pytest.approx(fc.CGLS_X20, rel=0.05) and cond == pytest.approx(fc.CGLS_COND, rel=0.01)
    assert all(b <= a for a, b in zip(residuals, residuals[1:]))
    iz, iy, ix = np.unravel_index(int(np.argmax(np.abs(x))), (6, 6, 6))
    assert iz == 3 and iy in (2, 3) and ix in (2, 3)
