"""nlos.fk_migration without a GPU: the host build of csrc/mtr_fk.h (tests/host_fk.cpp) stage by stage and, around torch's CPU
FFT, as a pipeline against the independent f64 reference of tests/fk_cases.py; the wrong readings of the operator the product
is held away from; point scatterers and oracle-rendered captures on the reference; the invariances of the time origin, the
binning and the depth range; the Python surface and the C ABI.  The kernels themselves: tests/test_gpu_fk_migration.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fk_cases as K  # noqa: E402

U = 2.0 ** -24            # the unit roundoff of f32


# ---------------------------------------------------------------- stages
def numpy_prepare_f32(Y, shift, q, Tp):
    """P in f32 NumPy: the q terms of a sample added one at a time in increasing j, as the operator fixes the order"""
    H, W, T = Y.shape
    S = np.zeros((H, W, Tp), np.float32)
    k = np.arange(Tp)
    for i in range(q):
        b = k[None, None, :] * q + i - shift[:, :, None]
        ok = (b >= 0) & (b < T)
        S = S + np.where(ok, np.take_along_axis(Y, np.clip(b, 0, T - 1), 2), np.float32(0.0)).astype(np.float32)
    psi = np.sqrt(np.maximum(S, np.float32(0.0))) * ((k.astype(np.float32) + np.float32(0.5)) / np.float32(Tp))
    P = np.zeros((2 * H, 2 * W, 2 * Tp), np.float32)
    P[:H, :W, :Tp] = psi
    return P


@pytest.mark.parametrize("q,Tp", [(1, 60), (3, 20), (3, 15), (4, 27)])
def test_host_prepare_is_f32_numpy_bit_for_bit(q, Tp):
    """ragged shifts of both signs; q = 3 on T = 50 leaves a ragged last group; T' odd and T' cutting the capture short"""
    Y, g, d = K.ragged_case()
    Y = Y - np.float32(0.1)                     # (some negative bins: max(S, 0))
    desc = K.make_desc(6, 10, 50, q, Tp, 0, Tp, 0.3, 0.2)
    got = K.host_prepare(desc, Y, d)
    want = numpy_prepare_f32(Y, d, q, Tp)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(got[:6, :10, :Tp]) > 0 and np.count_nonzero(got[6:]) == 0 and np.count_nonzero(got[:, :, Tp:]) == 0


@pytest.mark.parametrize("z0,nz", [(0, 45), (7, 30), (44, 1)])
def test_host_finish_is_f32_numpy_bit_for_bit(z0, nz):
    rng = np.random.default_rng(5)
    H, W, Tp = 6, 10, 45
    field = (rng.standard_normal((2 * H, 2 * W, 2 * Tp)) + 1j * rng.standard_normal((2 * H, 2 * W, 2 * Tp))).astype(np.complex64)
    got = K.host_finish(K.make_desc(H, W, 50, 1, Tp, z0, nz, 0.3, 0.2), field)
    re, im = field.real[:H, :W, z0:z0 + nz], field.imag[:H, :W, z0:z0 + nz]
    want = np.transpose(re * re + im * im, (2, 0, 1))
    assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize("H,W,Tp,ax,ay", [(6, 10, 45, 0.3, 0.2), (2, 2, 1200, 0.05, 0.07), (3, 2, 64, 1.7, 0.9)])
def test_host_stolt_is_held_to_the_f64_formula(H, W, Tp, ax, ay):
    """Element by element, on a random complex64 spectrum.  The bound is f32's own: the source index p = k' T' carries at most 6
    roundings' worth of relative error (three per squared term, the sums, the root, the product: 6 U p), which moves the
    interpolated value by that much of the steepest neighbouring segment; the weights, the two products, the sum and the
    Jacobian (kz / k', 6.5 U) add at most 12 U (|F0| + |F1|).  Where p is within its error of T' — the one place the formula
    itself jumps, to zero — the element is left out."""
    rng = np.random.default_rng(11)
    shape = (2 * H, 2 * W, Tp + 1)
    F = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    d = K.make_desc(H, W, 50, 1, Tp, 0, Tp, ax, ay)
    got = K.host_stolt(d, F).astype(np.complex128)
    want, p = K.stolt_f64(F, H, W, Tp, float(np.float32(ax)), float(np.float32(ay)))
    dp = 6.0 * U * p
    F64 = F.astype(np.complex128)
    seg = np.abs(np.diff(F64, axis=2))                                        # (2H, 2W, T'): segment i joins F[i] and F[i + 1]
    seg = np.concatenate([seg[..., :1], seg, seg[..., -1:], seg[..., -1:]], axis=2)     # index i + 1: segment i, clipped at the ends
    i0 = np.clip(np.floor(p).astype(np.int64), 0, Tp - 1)
    steep = np.maximum(np.maximum(np.take_along_axis(seg, i0, 2), np.take_along_axis(seg, i0 + 1, 2)), np.take_along_axis(seg, i0 + 2, 2))
    mag = np.abs(np.take_along_axis(F64, i0, 2)) + np.abs(np.take_along_axis(F64, i0 + 1, 2))
    bound = np.sqrt(2.0) * (dp * steep + 12.0 * U * mag)                      # (jac <= 1; sqrt 2: the bound holds per component)
    jump = np.abs(p - Tp) <= dp
    err = np.abs(got - want)
    assert np.count_nonzero(want) > H * W * Tp // 4 and np.all(np.isfinite(got.view(np.float64)))
    assert np.all(got[:, :, Tp:] == 0) and np.all(got[:, :, 0] == 0)          # kz <= 0
    worst = float(np.max(np.where(jump, 0.0, err / np.maximum(bound, 1e-300))))
    print("worst error over its bound:", worst, "elements at the jump:", int(jump.sum()))
    assert worst <= 1.0
    assert np.array_equal((got != 0), (want != 0)) or np.all(jump[(got != 0) != (want != 0)])


# ---------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def points():
    Y, g = K.point_case()
    return {"Y": Y, "g": g, "ref": K.reference(Y, g), "host": K.host_volume(Y, g)}


@pytest.fixture(scope="module")
def renders(oracle):
    """the quad and the 'Z' rendered by the CPU oracle at seed 0, channel 0, with their reference and host volumes"""
    import mitransient_amd as mitr
    out = {}
    for hidden in ("quad", "z"):
        scene = K.render_scene(hidden)
        sd = scene.data()
        p = scene.integrator().render_params(scene.sensors()[0].film(), 0, K.RENDER_SPP)
        t4, s4, _ = oracle.render(sd, p)
        t3, _ = oracle.develop(sd.film, t4, s4)
        assert t3.shape == (16, 16, 128, 3)
        Y = np.ascontiguousarray(t3[..., 0], np.float32)
        g = mitr.nlos.capture_geometry(scene)
        out[hidden] = {"Y": Y, "g": g, "ref": K.reference(Y, g), "host": K.host_volume(Y, g)}
    return out


def test_pipeline_points_against_the_f64_reference(points):
    rel = K.rel_l2(points["host"], points["ref"])
    print("points: host pipeline vs f64 reference, rel-L2", rel)
    assert points["host"].shape == points["ref"].shape == (256, 32, 32)
    assert rel <= 1e-5


@pytest.mark.parametrize("hidden", ["quad", "z"])
def test_pipeline_renders_against_the_f64_reference(renders, hidden):
    """measured with the host build: 3.4e-7 (quad), 4.5e-7 (z)"""
    r = renders[hidden]
    rel = K.rel_l2(r["host"], r["ref"])
    print(hidden, ": host pipeline vs f64 reference, rel-L2", rel)
    assert rel <= 1e-5


@pytest.mark.parametrize("misread", ["spacing", "shift", "jacobian", "edge"])
@pytest.mark.parametrize("hidden", ["quad", "z"])
def test_misreadings_land_far_away(renders, hidden, misread):
    """the host pipeline against the f64 reference of a WRONG reading of the operator: at least 1e-3 away.  Measured
    (quad / z): spacing 0.53 / 0.79, shift 0.68 / 0.66, jacobian 0.119 / 0.126, edge 3.1e-3 / 3.7e-3"""
    r = renders[hidden]
    wrong = K.reference(r["Y"], r["g"], misread=misread)
    rel = K.rel_l2(r["host"], wrong)
    print(hidden, misread, "rel-L2 to the misreading", rel)
    assert rel >= 1e-3


def test_point_scatterers_are_where_they_were_put(points):
    """on the reference and on the host pipeline: the expected voxel centres are (99.5, 12.3, 20.3) and (59.5, 23.5, 9.1)"""
    for name in ("ref", "host"):
        first, second = K.two_peaks(points[name])
        print(name, first, second)
        assert first == (100, 12, 20) and second == (60, 24, 9)


@pytest.mark.parametrize("hidden", ["quad", "z"])
def test_rendered_captures_focus_at_their_depth(renders, hidden):
    """asserted on the f64 reference (and the host pipeline follows it to 1e-5, above)"""
    V = renders[hidden]["ref"]
    profile = V.sum(axis=(1, 2))
    k = int(np.argmax(profile))
    share = float(V[k, 4:12, 4:12].sum() / V[k].sum())
    print(hidden, "brightest depth sample", k, "share of the quad's footprint", share)
    assert abs(k - K.Z1_SAMPLE) <= 1.0
    assert share >= 0.85


# ---------------------------------------------------------------- invariances, bit for bit on the host pipeline
def test_offsets_move_the_capture_by_whole_bins():
    """Y2[y, x, b] = Y[y, x, b - d[y, x]] with d bin_width added to the sensor offset is the same capture"""
    rng = np.random.default_rng(2)
    H, W, T, bw = 6, 10, 50, 0.03125
    Y = rng.random((H, W, T), dtype=np.float32)
    Y[..., 40:] = 0.0                                       # (room for the delays: nothing leaves the capture)
    d = rng.integers(0, 9, size=(H, W))
    d[0, 0] = 0                                             # (the largest shift, and with it T', stays)
    Y2 = np.zeros_like(Y)
    for y in range(H):
        for x in range(W):
            Y2[y, x, d[y, x]:] = Y[y, x, :T - d[y, x]]
    g = K.grid_geometry(H, W, 0.07, 0.05, T, bw, start=0.5, offset=np.full((H, W), 0.25))
    g2 = K.grid_geometry(H, W, 0.07, 0.05, T, bw, start=0.5, offset=0.25 + d * bw)
    a, b = K.host_volume(Y, g), K.host_volume(Y2, g2)
    assert np.count_nonzero(a) > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, K.host_volume(Y2, g))


@pytest.mark.parametrize("q", [2, 3])
def test_bin_factor_is_summing_first(q):
    """bin_factor = q equals the migration, with bin_factor = 1, of the capture summed on the host in the same f32 order"""
    Y, g, d = K.ragged_case()
    T = Y.shape[2]
    n = -(-(T + int(d.max())) // q)
    S = np.zeros(Y.shape[:2] + (n,), np.float32)
    k = np.arange(n)
    for i in range(q):
        b = k[None, None, :] * q + i - d[:, :, None]
        ok = (b >= 0) & (b < T)
        S = S + np.where(ok, np.take_along_axis(Y, np.clip(b, 0, T - 1), 2), np.float32(0.0)).astype(np.float32)
    gs = K.grid_geometry(6, 10, 0.07, 0.05, n, q * g.bin_width_opl)
    a, b = K.host_volume(Y, g, bin_factor=q), K.host_volume(S, gs)
    assert a.shape == b.shape and np.count_nonzero(a) > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_depth_range_returns_rows_of_the_full_volume():
    import mitransient_amd as mitr
    Y, g, d = K.ragged_case()
    full, z = K.host_volume(Y, g), mitr.nlos.fk_depths(g)
    assert full.shape == (60, 6, 10) and z.shape == (60,)              # T + max shift = 58 -> T' = 60
    assert np.allclose(z, (np.arange(60) + 0.5) * g.bin_width_opl / 2, rtol=0, atol=1e-15)
    for rng_ in ((0.2, None), (0.2, 0.915), (None, 0.92), (z[57], 0.92)):
        lo = 0.0 if rng_[0] is None else rng_[0]
        hi = np.inf if rng_[1] is None else rng_[1]
        keep = (z >= lo) & (z <= hi)                                    # (every zmax here keeps T' at 60)
        part = K.host_volume(Y, g, depth_range=rng_)
        assert 0 < keep.sum() < 60 and part.shape == (keep.sum(), 6, 10)
        assert np.array_equal(part.view(np.uint32), full[keep].view(np.uint32))
        assert np.array_equal(mitr.nlos.fk_depths(g, rng_), z[keep])
    short = mitr.nlos.fk_depths(g, (0.1, 0.4))                         # a zmax that shortens the depth grid: ceil(0.4 / dz) = 26 -> 27
    assert K.reference(Y, g, (0.1, 0.4)).shape[0] == len(short) == np.count_nonzero((z >= 0.1) & (z <= 0.4))
    assert K.rel_l2(K.host_volume(Y, g, depth_range=(0.1, 0.4)), K.reference(Y, g, (0.1, 0.4))) <= 1e-5


# ---------------------------------------------------------------- surface
def test_python_validates_before_touching_the_gpu(monkeypatch):
    import torch
    import mitransient_amd as mitr
    from mitransient_amd import runtime
    from mitransient_amd.nlos import CaptureGeometry, fk_depths, fk_migration

    def no_context(*a, **k):
        raise AssertionError("the context was asked for before the arguments were checked")
    monkeypatch.setattr(runtime, "get_context", no_context)
    g = K.grid_geometry(4, 6, 0.1, 0.1, 16, 0.04, start=0.2)
    sp = g.sensor_points
    ok = np.zeros((4, 6, 16), np.float32)

    def geom(ct=K.CONFOCAL, pts=sp, lp=None, T=16, bw=0.04):
        lp = pts.reshape(-1, 3) if lp is None else lp
        return CaptureGeometry(ct, pts, lp, np.zeros(pts.shape[:2]), np.zeros(len(lp)), 0.2, bw, T)
    bent, skew, line = sp.copy(), sp.copy(), sp[:1]
    bent[2, 3, 2] += 1e-5                                       # one point off the plane by 1e-4 of the spacing
    skew[..., 0] += 0.01 * sp[..., 1]                           # a sheared grid: affine, not orthogonal
    for capture, geometry, kw in (
            (ok, "geometry", {}),
            (ok, geom(1, lp=sp.reshape(-1, 3)[:1]), {}),                     # Single
            (np.zeros((4, 6, 2, 12, 16), np.float32), geom(3), {}),          # Exhaustive
            (ok, geom(pts=bent), {}), (ok, geom(pts=skew), {}),
            (np.zeros((1, 6, 16), np.float32), geom(pts=line), {}),          # H < 2
            (np.zeros((6, 1, 16), np.float32), geom(pts=np.ascontiguousarray(np.transpose(line, (1, 0, 2)))), {}),       # W < 2
            (np.zeros((4, 6), np.float32), g, {}), (np.zeros((4, 5, 16), np.float32), g, {}),
            (np.zeros((4, 6, 15), np.float32), g, {}), (ok, geom(T=15), {}), (ok, geom(bw=0.0), {}),
            (np.zeros((4, 6, 16, 0), np.float32), g, {}),
            (ok, g, {"channel": 0}), (np.zeros((4, 6, 16, 3), np.float32), g, {"channel": 3}),
            (ok, g, {"bin_factor": 0}), (ok, g, {"bin_factor": 1.5}), (ok, g, {"bin_factor": 2.0}), (ok, g, {"bin_factor": True}),
            (ok, g, {"depth_range": (0.3, 0.3)}), (ok, g, {"depth_range": (0.3, 0.1)}), (ok, g, {"depth_range": (-0.5, -0.1)}),
            (ok, g, {"depth_range": (None, 0.0)}), (ok, g, {"depth_range": 0.4}), (ok, g, {"depth_range": (0.111, 0.129)}),
            (ok, g, {"depth_range": (5.0, None)}),
            (torch.zeros((4, 6, 16), requires_grad=True), g, {})):
        with pytest.raises(ValueError, match="fk_migration"):
            fk_migration(capture, geometry, **kw)
    for geometry, kw in (("geometry", {}), (geom(3), {}), (geom(pts=bent), {}), (g, {"bin_factor": 0}), (g, {"depth_range": (0.3, 0.1)})):
        with pytest.raises(ValueError, match="fk_depths"):
            fk_depths(geometry, **kw)
    assert mitr.nlos.fk_migration is fk_migration and mitr.nlos.fk_depths is fk_depths
    monkeypatch.undo()
    if not torch.cuda.is_available():           # a valid call without a GPU: the product has no CPU path
        from mitransient_amd._cabi import MitransientAMDError
        with pytest.raises(MitransientAMDError):
            fk_migration(ok, g)


def test_fk_depths_agrees_with_the_volume():
    import mitransient_amd as mitr
    Y, g, d = K.ragged_case()
    for kw in ({}, {"bin_factor": 3}, {"bin_factor": 3, "depth_range": (0.2, 0.6)}, {"depth_range": (None, 0.35)}):
        z = mitr.nlos.fk_depths(g, **kw)
        V = K.host_volume(Y, g, **kw)
        q = kw.get("bin_factor", 1)
        assert z.dtype == np.float64 and V.shape == (len(z), 6, 10) == K.reference(Y, g, kw.get("depth_range"), q).shape
        step = q * g.bin_width_opl / 2
        assert np.allclose(np.diff(z), step, rtol=0, atol=1e-12) and abs((z[0] / step - 0.5) - round(z[0] / step - 0.5)) < 1e-9
    assert mitr.nlos._next_5_smooth(1031) == 1080 and all(mitr.nlos._next_5_smooth(n) == K.next_5_smooth(n) for n in range(1, 700))


def test_header_and_cabi_agree():
    from mitransient_amd import _cabi
    header = open(os.path.join(K.ROOT, "include", "mitransient_amd.h")).read()
    for line in ("int  mtr_fk_prepare(mtr_ctx *, const mtr_fk_desc *, const float *capture_dev, const int32_t *shift_dev, float *padded_dev);",
                 "int  mtr_fk_stolt(mtr_ctx *, const mtr_fk_desc *, const float *spectrum_dev, float *resampled_dev);",
                 "int  mtr_fk_finish(mtr_ctx *, const mtr_fk_desc *, const float *field_dev, float *volume_dev);"):
        assert line in header
    for name in ("mtr_fk_prepare", "mtr_fk_stolt", "mtr_fk_finish"):
        assert name in _cabi.EXPORTS
    body = re.search(r"typedef struct mtr_fk_desc \{(.*?)\} mtr_fk_desc;", header, re.S).group(1)
    fields = [n for decl in re.sub(r"/\*.*?\*/", "", body).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [f[0] for f in _cabi.mtr_fk_desc._fields_]
    assert K.host_lib().hfk_desc_size() == C.sizeof(_cabi.mtr_fk_desc) == 36
    assert _cabi.MTR_ABI_VERSION == 24 and re.search(r"#define\s+MTR_ABI_VERSION\s+24\b", header)


def test_entry_points_refuse_without_launching():
    """fk_check, the test all three entry points make before any launch, through the host build (no device needed)"""
    lib = K.host_lib()
    a = 4096                                    # a 16-byte aligned address: fk_check looks at pointers, never through them
    good = K.make_desc(4, 6, 16, 1, 18, 2, 16, 0.2, 0.2)
    assert lib.hfk_check(C.byref(good), a, a) is None
    for field, value in (("height", 1), ("width", 1), ("height", 0x8000), ("width", 0x8000), ("temporal_bins", 0), ("bin_factor", 0),
                         ("depth_bins", 0), ("nz", 0), ("nz", 17), ("z_begin", 3), ("ax", 0.0), ("ay", -1.0), ("ax", np.inf), ("ay", np.nan)):
        bad = K.make_desc(4, 6, 16, 1, 18, 2, 16, 0.2, 0.2)
        setattr(bad, field, value)
        assert lib.hfk_check(C.byref(bad), a, a) is not None, (field, value)
    assert lib.hfk_check(C.byref(good), None, a) and lib.hfk_check(C.byref(good), a, None) and lib.hfk_check(C.byref(good), a + 8, a)
