"""What tests/test_gpu_splat_large_films.py rests on, checked on the CPU for every case of its table: the float64 reference
film of tests/splat_cases.py agrees with the oracle's own scatter-add, the film is dense enough for the support comparison to
mean something, and a kernel that MISREAD one of the paths the cases are there for would land far outside the parity bar."""
import numpy as np
import pytest

import splat_cases as sc
from conftest import rel_l2

TOL = 1e-5                    # the parity bar of the GPU test (tests/test_gpu_parity.py)
FAR = 100 * TOL               # a misread film lies at least this far from the reference, or differs in support

# (case, misreading) pairs that CANNOT show: the case does not take the path.  Everything else must show.
#   per = 1 in the half concerned: no second counter, no ragged thread
#   2^20 or 2^21 contributions: at most 512 tiles, the first trip of the tile loop takes them all (the four cases with more
#   contributions have 768 or 1280 tiles)
NO_EFFECT = {
    "last_single": {"hi_digits_from_256", "lo_digits_from_256", "thread_255", "last_active_thread", "tiles_past_the_grid"},
    "ragged_257": {"lo_digits_from_256", "thread_255", "tiles_past_the_grid"},
    "hi_512": {"lo_digits_from_256", "tiles_past_the_grid"},
    "bench_pixels": set(),
    "ragged_513": {"tiles_past_the_grid"},
    "per_4": {"tiles_past_the_grid"},
    "ragged_1025": {"tiles_past_the_grid"},
    "hi_2048": set(),
    "limit": set(),
    "beyond": set(),
}


@pytest.mark.parametrize("case", list(sc.CASES))
def test_reference_and_misreadings(oracle, case):
    W, H, T, n = sc.CASES[case]
    npix = W * H
    pixel, opl, r, g, b, ref = sc.make(W, H, T, n)
    assert ref.shape == (H, W, T, 3) and ref.dtype == np.float64 and len(pixel) == n
    assert pixel.max() == npix + 1                                       # ids out of range are there
    tbin = sc.bins_of(opl, T)
    assert tbin.min() == -1 and tbin.max() == T
    for p in sc.hot_pixels(npix):
        assert np.count_nonzero(pixel == p) >= sc.HOT > 2048             # more than one batch of k_splat_rows_rec
    kept = (pixel < npix) & (tbin >= 0) & (tbin < T)
    share = np.count_nonzero(kept) / n
    counts = np.bincount(pixel[kept].astype(np.int64) * T + tbin[kept], minlength=npix * T)
    filled = np.count_nonzero(counts) / counts.size
    # the oracle's scatter-add (f32 adds in input order, its own f32 bin arithmetic) against the float64 film
    got = np.zeros((H, W, T, 4), np.float32)
    oracle.splat_add(sc.film_desc(W, H, T), pixel, opl, r, g, b, got)
    err = rel_l2(got[..., :3], ref)
    print(f"{case}: kept {share:.3f}, bins filled {filled:.3f}, most per bin {counts.max()}, oracle vs f64 {err:.2e}")
    assert np.array_equal(got[..., :3] != 0, ref != 0) and np.all(got[..., 3] == 0)
    assert err <= 0.1 * TOL
    assert 0.4 <= share <= 0.98
    # a bin's f32 sum in input order is off by at most (count - 1) half-ulps of the running sum: 1000 x 2^-24 = 6e-5 of that
    # bin at the very worst, a few 1e-7 over the film; the hot pixels' bins hold 3000 / (T + 2) <= 750 + 10 sigma
    assert counts.max() <= 1000
    bits_pix, bits_lo, n_lo, n_hi = sc.digits(npix)
    shown = {}
    for name in sc.MISREADINGS:
        dist, support = sc.misreading_distance(name, pixel, opl, r, g, b, ref, T)
        shown[name] = (dist, support)
        if name in NO_EFFECT[case]:
            assert dist == 0.0 and not support, name
        else:
            assert dist >= FAR or support, (name, dist)
    print(f"{case}: n_hi {n_hi} (per {sc.per(n_hi)}), n_lo {n_lo} (per {sc.per(n_lo)}); misreadings: "
          + ", ".join(f"{k} {d:.2e}{' +support' if s else ''}" for k, (d, s) in shown.items()))


@pytest.mark.parametrize("case", list(sc.CASES))
def test_film_is_dense_enough(case):
    """more than a quarter of the film's bins are non-zero (and, with the out-of-range ids and path lengths, well short of
    all): the comparison of supports in the GPU test has both kinds of bin to tell apart.

    Uniform contributions of which a share k is kept fill 1 - exp(-k n / (W H T)) of the bins, so this bar decides n for the
    four sparsest films (tests/splat_cases.py: CASES): bench_pixels, hi_2048, limit and beyond fill 0.26 to 0.31, the other
    six 0.28 to 0.79."""
    W, H, T, n = sc.CASES[case]
    npix = W * H
    pixel, opl, *_ = sc.make(W, H, T, n, reference=False)
    tbin = sc.bins_of(opl, T)
    kept = (pixel < npix) & (tbin >= 0) & (tbin < T)
    counts = np.bincount(pixel[kept].astype(np.int64) * T + tbin[kept], minlength=npix * T)
    filled = np.count_nonzero(counts) / counts.size
    print(f"{case}: bins filled {filled:.4f}")
    assert filled < 0.9
    assert filled > 0.25


def test_every_misreading_is_caught_by_a_case():
    for name in sc.MISREADINGS:
        assert any(name not in NO_EFFECT[c] for c in sc.CASES), name


def test_orders_hold_the_same_records():
    W, H, T, n = 331, 198, 8, 1 << 16
    base = sc.make(W, H, T, n, seed=5)
    npix = W * H
    key = lambda c: np.sort(c[0].astype(np.int64) * 1000003 + np.round(c[2] * 1e6).astype(np.int64))
    for order in ("sorted", "descending"):
        c = sc.make(W, H, T, n, order, seed=5)
        assert c[5] is base[5] and not c[5].flags.writeable
        assert np.array_equal(key(c), key(base))
        again = sc.film_f64(c[0], sc.bins_of(c[1], T), c[2], c[3], c[4], npix, T).reshape(H, W, T, 3)
        assert rel_l2(again, base[5]) < 1e-14
    s = sc.make(W, H, T, n, "sorted", seed=5)[0]
    assert np.all(np.diff(np.minimum(s, npix).astype(np.int64)) >= 0) and s[-1] >= npix          # out-of-range ids last
    d = sc.make(W, H, T, n, "descending", seed=5)[0]
    assert np.all(np.diff(d.astype(np.int64)) <= 0) and d[0] == npix + 1
    assert np.any(np.diff(base[0].astype(np.int64)) < 0)


def test_digits_match_the_plan_table():
    assert sc.digits(65536) == (16, 8, 256, 256) and sc.digits(331 * 198) == (17, 8, 256, 257)
    assert sc.digits(513 * 512)[2:] == (512, 513) and sc.digits(1025 * 1024)[2:] == (1024, 1025)
    assert sc.digits(1 << 22) == (22, 11, 2048, 2048)
    assert [sc.per(v) for v in (256, 257, 512, 513, 1025, 2048)] == [1, 2, 2, 3, 5, 8]
