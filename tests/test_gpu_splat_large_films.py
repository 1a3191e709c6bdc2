"""mtr_splat_add (film.add_transient_data -> put_opl) on films ABOVE 2^16 pixels against a float64 reference film.

The partition path (mtr_splat.hip) splits the pixel index into two digits of at most 2048 values; a thread of the tile scan
owns per = ceil(n_digits / 256) digit counters.  per stays 1 up to 2^16 pixels — every other GPU test of the path — while the
published benchmark (512 x 512 x 1024) runs at per = 2 in both passes.  The cases (tests/splat_cases.py; checked on the CPU by
tests/test_splat_cases.py, the digit counts by tests/test_splat_plan.py):

    case          W x H x T         n     what it reaches
    last_single   256 x 256 x 8     2^20  control: per 1 / 1
    ragged_257    331 x 198 x 8     2^20  n_hi = 257, per_hi = 2, one digit in the second slot
    hi_512        512 x 256 x 8     2^20  n_hi = 512, n_lo = 256
    bench_pixels  512 x 512 x 64    5x2^20 the benchmark's pixel count; 1280 tiles for 512 workgroups: the tile loop's second and third trip
    ragged_513    513 x 512 x 3     2^21  per_hi = 3
    per_4         1024 x 1024 x 4   2^21  per 4 / 4; 257 scan blocks
    ragged_1025   1025 x 1024 x 2   2^21  per_hi = 5
    hi_2048       2048 x 1024 x 2   3x2^20 per 8 / 4
    limit         2048 x 2048 x 2   5x2^20 the largest supported film; 1025 scan blocks
    beyond        2049 x 2048 x 2   5x2^20 not supported: the atomics must give the same film

Every case: variant 1, shuffled, onto a zero film without MTR_SPLAT_FILM_ZERO.  bench_pixels and limit also: pixel-sorted input
(the persistent pixel loop of k_splat_rows, more pixels than workgroups) with and without the flag, descending input,
shuffled with the flag, shuffled through variant 0; bench_pixels also a second batch accumulating onto the first.
Bars: support equal to the reference, channel 3 zero, rel-L2 <= 1e-5 (the parity bar; the reference is float64)."""
import numpy as np
import pytest

import splat_cases as sc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5                    # tests/test_gpu_parity.py: TOL
GIB = 1 << 30

# leg -> (order, variant bits)
FILM_ZERO = 0x100             # _cabi.MTR_SPLAT_FILM_ZERO (asserted below)
LEGS = {
    "shuffled": ("shuffled", 1),
    "sorted": ("sorted", 1),
    "sorted_zero": ("sorted", 1 | FILM_ZERO),
    "descending": ("descending", 1),
    "shuffled_zero": ("shuffled", 1 | FILM_ZERO),
    "shuffled_v0": ("shuffled", 0),
    "accumulate": ("shuffled", 1),
}
RUNS = []
for _case in sc.CASES:
    RUNS.append((_case, "shuffled"))
    if _case in ("bench_pixels", "limit"):
        RUNS += [(_case, leg) for leg in ("sorted", "sorted_zero", "descending", "shuffled_zero", "shuffled_v0")]
    if _case == "bench_pixels":
        RUNS.append((_case, "accumulate"))


def bare_film(W, H, T):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    from mitransient_amd.scene import Properties
    mi.set_variant("llvm_ad_rgb")
    film = mitr.TransientHDRFilm(Properties("transient_hdr_film", {"width": W, "height": H, "temporal_bins": T, "start_opl": sc.START_OPL,
                                                                   "bin_width_opl": sc.bin_width(T), "rfilter": {"type": "box"}}))
    film.prepare([])
    return film


def to_device(x):
    import torch
    return torch.tensor(x.view(np.int32) if x.dtype == np.uint32 else x, device="cuda")


@pytest.mark.parametrize("case,leg", RUNS, ids=[f"{c}-{l}" for c, l in RUNS])
def test_large_film_matches_the_f64_reference(case, leg):
    import torch
    from mitransient_amd import _cabi
    assert _cabi.MTR_SPLAT_FILM_ZERO == FILM_ZERO
    W, H, T, n = sc.CASES[case]
    order, variant = LEGS[leg]
    pixel, opl, r, g, b, ref = sc.make(W, H, T, n, order)
    if order == "shuffled":
        assert np.any(np.diff(pixel.astype(np.int64)) < 0)              # the partition (or, beyond its limit, the atomics) runs
    film = bare_film(W, H, T)
    film.transient_storage.put_opl(to_device(pixel), to_device(opl), to_device(r), to_device(g), to_device(b), film.desc(), variant)
    if leg == "accumulate":                                              # a second batch lands on the first: read-modify-write flush
        p2, o2, r2, g2, b2, ref2 = sc.make(W, H, T, 1 << 20, "shuffled", seed=1)
        film.transient_storage.put_opl(to_device(p2), to_device(o2), to_device(r2), to_device(g2), to_device(b2), film.desc(), 1)
        ref = ref + ref2
    torch.cuda.synchronize()
    got = film.transient_storage.torch_tensor().cpu().numpy()
    assert got.shape == (H, W, T, 4)
    err = rel_l2(got[..., :3], ref)
    same_support = np.array_equal(got[..., :3] != 0, ref != 0)
    print(f"{case}-{leg}: rel-L2 vs f64 {err:.3e}, same support {same_support}, non-zero bins {np.count_nonzero(ref[..., 0])}")
    assert same_support
    assert not got[..., 3].any()
    assert err <= TOL
    if case == "limit":           # the workspace the context kept for the partition can be handed back
        from mitransient_amd.runtime import get_context
        ctx = get_context()
        ctx.check(ctx.lib.mtr_ctx_trim(ctx.handle), "mtr_ctx_trim")


def test_benchmark_film_through_add_transient_data(oracle):
    """the benchmark's own film (512 x 512 x 1024, 4 GiB) through the benchmark's own call, film.add_transient_data(pos, opl,
    None, rgb, variant=1), with 2^22 shuffled contributions: against a second film that got the same input through variant 0
    (equal support, rel-L2 <= 2e-6: tools/soak_splat.py's bar for this comparison; norms accumulated in float64 over slabs,
    no f64 copy of a film), and 68 rows — pixels 0, 2^17 - 1, 2^17, 2^18 - 1 and 64 drawn — against the oracle at 1e-5."""
    import gc
    import torch
    W = H = 512
    T = 1024
    npix = W * H
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB of device memory free: the two 4 GiB films need 12")
    torch.cuda.reset_peak_memory_stats()
    pixel, opl, r, g, b, _ = sc.make(W, H, T, 1 << 22, "shuffled", reference=False)
    pixels = to_device(pixel)
    pos = torch.stack(((pixels % W).float() + 0.5, (pixels // W).float() + 0.5), dim=1)       # as bench.py: ids >= npix fall below the film
    opl_d = to_device(opl)
    rgb = torch.stack((to_device(r), to_device(g), to_device(b)), dim=1)
    film1, film0 = bare_film(W, H, T), bare_film(W, H, T)
    film1.add_transient_data(pos, opl_d, None, rgb, variant=1)
    film0.add_transient_data(pos, opl_d, None, rgb, variant=0)
    torch.cuda.synchronize()
    a, c = film1.transient_storage.torch_tensor(), film0.transient_storage.torch_tensor()
    assert tuple(a.shape) == (H, W, T, 4)
    same_support, num, den = True, 0.0, 0.0
    for y in range(0, H, 32):                                            # slabs of 256 MiB
        x1, x0 = a[y:y + 32], c[y:y + 32]
        same_support = same_support and bool(((x1 != 0) == (x0 != 0)).all())
        num += float(torch.linalg.vector_norm(x1 - x0, dtype=torch.float64)) ** 2
        den += float(torch.linalg.vector_norm(x0, dtype=torch.float64)) ** 2
    err = (num / max(den, 1e-300)) ** 0.5
    # 68 rows against the oracle's scatter-add on a 68 x 1 film of the same time axis
    rng = np.random.default_rng(2024)
    fixed = np.array([0, (1 << 17) - 1, 1 << 17, npix - 1])
    rows = np.concatenate([fixed, rng.choice(np.setdiff1d(np.arange(npix), fixed), 64, replace=False)])
    got = a.view(npix, T, 4)[torch.tensor(rows, device="cuda")].cpu().numpy()
    by_id = np.argsort(rows)
    sel = np.isin(pixel, rows)
    renumbered = by_id[np.searchsorted(rows[by_id], pixel[sel])].astype(np.uint32)
    ref = np.zeros((1, len(rows), T, 4), np.float32)
    oracle.splat_add(sc.film_desc(len(rows), 1, T), renumbered, opl[sel], r[sel], g[sel], b[sel], ref)
    err_rows = rel_l2(got[..., :3], ref[0][..., :3])
    rows_support = np.array_equal(got != 0, ref[0] != 0)
    peak = torch.cuda.max_memory_allocated()
    print(f"benchmark film: variant 1 vs variant 0 rel-L2 {err:.3e}, same support {same_support}; 68 rows vs oracle {err_rows:.3e}, "
          f"same support {rows_support}, {np.count_nonzero(sel)} contributions in them; peak {peak / GIB:.2f} GiB")
    assert den > 0 and np.count_nonzero(sel) > 3 * sc.HOT
    assert same_support and err <= 2e-6
    assert rows_support and err_rows <= TOL
    assert peak < 10 * GIB
    del a, c, film1, film0
    torch.cuda.empty_cache()
