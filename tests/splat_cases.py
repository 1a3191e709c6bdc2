"""Contributions and float64 reference films for the tests of mtr_splat_add on films ABOVE 2^16 pixels
(tests/test_splat_cases.py on the CPU, tests/test_gpu_splat_large_films.py on the GPU).  No torch in here.

The subject is WHERE a contribution lands by pixel: the two-digit split of the pixel index (mtr_splat_plan.h), threads of the
tile scan that own more than one digit counter, the ragged last bucket, tiles and pixels handed to a second loop trip.  So
path lengths are bin centres (bin-edge semantics are pinned at small sizes elsewhere), a few pixel ids are out of range, and
six HOT pixels — either side of a bucket boundary, the first pixel of the last bucket, the last pixel, the middle — hold 3000
contributions each (more than one 2048-record batch of k_splat_rows_rec)."""
import functools

import numpy as np

START_OPL = 3.5
WINDOW = 6.0
HOT = 3000                    # contributions per hot pixel
BLOCK = 256                   # threads per workgroup: tile_scan_claim gives each ceil(n_digits / 256) digit counters
TILE = 4096                   # records of a staging tile of the scatters

# name -> (W, H, T, n): what each reaches is in the docstring of tests/test_gpu_splat_large_films.py.
# n is 2^20 for the films up to 2^17 pixels, 2^21 above — and MORE where 2^21 (2^22 for bench_pixels, whose point is more tiles
# than workgroups) would leave the film too empty for tests/test_splat_cases.py::test_film_is_dense_enough: uniform
# contributions of which a share k is kept fill 1 - exp(-k n / (W H T)) of the bins, and a quarter needs k n > 0.288 W H T.
#   bench_pixels  k 0.970, 2^24 bins: n > 4.98 M -> 5 x 2^20      hi_2048        k 0.500, 2^22 bins: n > 2.41 M -> 3 x 2^20
#   limit, beyond k 0.500, 2^23 bins: n > 4.83 M -> 5 x 2^20 (2^21 could not reach a quarter with every contribution kept)
# More contributions reach everything fewer did: digit counts, scan blocks and the support limit depend on W x H alone, and
# the tile loop only makes more trips.
CASES = {
    "last_single": (256, 256, 8, 1 << 20),
    "ragged_257": (331, 198, 8, 1 << 20),
    "hi_512": (512, 256, 8, 1 << 20),
    "bench_pixels": (512, 512, 64, 5 << 20),
    "ragged_513": (513, 512, 3, 1 << 21),
    "per_4": (1024, 1024, 4, 1 << 21),
    "ragged_1025": (1025, 1024, 2, 1 << 21),
    "hi_2048": (2048, 1024, 2, 3 << 20),
    "limit": (2048, 2048, 2, 5 << 20),
    "beyond": (2049, 2048, 2, 5 << 20),
}
ORDERS = ("shuffled", "sorted", "descending")


def bin_width(T):
    return WINDOW / T


def digits(npix):
    """(bits_pix, bits_lo, n_lo, n_hi) of launch_splat_partitioned, written apart from it (tests/test_splat_plan.py holds the
    header to the same table)"""
    bits_pix = max(1, (npix - 1).bit_length())
    bits_lo = bits_pix // 2
    return bits_pix, bits_lo, 1 << bits_lo, ((npix - 1) >> bits_lo) + 1


def per(n_digits):
    return (n_digits + BLOCK - 1) // BLOCK


def hot_pixels(npix):
    _, bits_lo, n_lo, n_hi = digits(npix)
    return [0, n_lo - 1, n_lo, (n_hi - 1) << bits_lo, npix - 1, npix // 2]


def bins_of(opl, T):
    """time bin of a bin-centre path length (-1 and T: outside the window by half a bin)"""
    return np.floor((opl.astype(np.float64) - START_OPL) / bin_width(T)).astype(np.int64)


def film_f64(pixel, tbin, r, g, b, npix, T, keep=None):
    """np.bincount in float64 over pixel * T + bin of the kept records -> (npix, T, 3)"""
    ok = (pixel < npix) & (tbin >= 0) & (tbin < T)
    if keep is not None:
        ok &= keep
    key = pixel[ok].astype(np.int64) * T + tbin[ok]
    out = np.empty((npix * T, 3), np.float64)
    for c, v in enumerate((r, g, b)):
        out[:, c] = np.bincount(key, weights=v[ok].astype(np.float64), minlength=npix * T)
    return out.reshape(npix, T, 3)


@functools.lru_cache(maxsize=2)
def _base(W, H, T, n, seed, reference):
    npix = W * H
    rng = np.random.default_rng(seed)
    pixel = rng.integers(0, npix + 2, n).astype(np.uint32)             # npix, npix + 1: out of range
    hot = hot_pixels(npix)
    assert n >= 2 * HOT * len(hot)
    for k, p in enumerate(hot):
        pixel[k * HOT:(k + 1) * HOT] = p
    rng.shuffle(pixel)
    tbin = rng.integers(-1, T + 1, n)                                  # -1 and T: outside the window
    opl = (START_OPL + (tbin + 0.5) * bin_width(T)).astype(np.float32)
    r, g, b = (rng.random(n, dtype=np.float32) for _ in range(3))
    ref = film_f64(pixel, tbin, r, g, b, npix, T).reshape(H, W, T, 3) if reference else None
    for a in (pixel, opl, r, g, b) + ((ref,) if reference else ()):
        a.flags.writeable = False
    return pixel, opl, r, g, b, ref


def make(W, H, T, n, order="shuffled", seed=0, reference=True):
    """pixel (u32), opl, r, g, b (f32) and the float64 reference film (H, W, T, 3) — None with reference=False.
    order: "shuffled"; "sorted" = stable by pixel, out-of-range ids last; "descending" = by falling pixel id (every change of
    pixel trips the unsorted flag, and a staging tile falls into one or two digits: the opposite extreme from uniform input).
    The three orders hold the SAME records: one reference film (cached, read-only) serves them all."""
    pixel, opl, r, g, b, ref = _base(W, H, T, n, seed, reference)
    if order == "shuffled":
        return pixel, opl, r, g, b, ref
    npix = W * H
    if order == "sorted":
        perm = np.argsort(np.minimum(pixel, npix), kind="stable")
    elif order == "descending":
        perm = np.argsort(-pixel.astype(np.int64), kind="stable")
    else:
        raise ValueError(order)
    return pixel[perm], opl[perm], r[perm], g[perm], b[perm], ref


def film_desc(W, H, T):
    """mtr_film_desc of the bare film the GPU test builds (width W, height H, T bins over [3.5, 9.5))"""
    from mitransient_amd import _cabi
    f = _cabi.mtr_film_desc()
    f.width, f.height, f.crop_width, f.crop_height = W, H, W, H
    f.temporal_bins = T
    f.start_opl = np.float32(START_OPL)
    f.bin_width_opl = np.float32(bin_width(T))
    return f


# ---------------------------------------------------------------------------------------------------------------------------
# MISREADINGS: what a film would look like if a kernel got one of the untested paths wrong.  Each maps every record to the
# pixel it would land in (npix: lost); `misreading_distance` gives the rel-L2 distance of that film from the reference and
# whether its support differs, touching only the records that moved.
N_CU = 256                    # compute units of an MI355X: k_part_scatter_hi runs n_cu * 2 workgroups at n_hi <= 512


def _lose(pixel, npix, lost):
    out = pixel.copy()
    out[lost & (pixel < npix)] = npix
    return out


def mis_hi_digits_from_256(pixel, npix):
    """tile_scan_claim scans only each thread's FIRST counter of the high half: digits >= 256 never get a range"""
    _, bits_lo, _, _ = digits(npix)
    return _lose(pixel, npix, (pixel >> bits_lo) >= BLOCK)


def mis_lo_digits_from_256(pixel, npix):
    _, _, n_lo, _ = digits(npix)
    return _lose(pixel, npix, (pixel & (n_lo - 1)) >= BLOCK)


def mis_thread_255(pixel, npix):
    """the counters of the scan's last thread (idx >= per * 255) are lost, in either half that has per > 1"""
    _, bits_lo, n_lo, n_hi = digits(npix)
    lost = np.zeros(len(pixel), bool)
    if per(n_hi) > 1:
        lost |= (pixel >> bits_lo) >= per(n_hi) * (BLOCK - 1)
    if per(n_lo) > 1:
        lost |= (pixel & (n_lo - 1)) >= per(n_lo) * (BLOCK - 1)
    return _lose(pixel, npix, lost)


def mis_last_active_thread(pixel, npix):
    """the counters of the last thread that HAS any (the ragged one: digit 256 of 257, 512 of 513, 1024 of 1025) are lost"""
    _, bits_lo, n_lo, n_hi = digits(npix)
    lost = np.zeros(len(pixel), bool)
    if per(n_hi) > 1:
        lost |= (pixel >> bits_lo) >= per(n_hi) * ((n_hi - 1) // per(n_hi))
    if per(n_lo) > 1:
        lost |= (pixel & (n_lo - 1)) >= per(n_lo) * ((n_lo - 1) // per(n_lo))
    return _lose(pixel, npix, lost)


def mis_tiles_past_the_grid(pixel, npix):
    """k_part_scatter_hi's loop makes one trip: the records of every tile beyond the first n_cu * 2 are lost"""
    return _lose(pixel, npix, np.arange(len(pixel)) >= N_CU * 2 * TILE)


def mis_last_pixel(pixel, npix):
    return _lose(pixel, npix, pixel == npix - 1)


def mis_swap_across_bucket(pixel, npix):
    """the last pixel of bucket 0 and the first of bucket 1 change places"""
    _, _, n_lo, _ = digits(npix)
    out = pixel.copy()
    out[pixel == n_lo - 1] = n_lo
    out[pixel == n_lo] = n_lo - 1
    return out


MISREADINGS = {
    "hi_digits_from_256": mis_hi_digits_from_256,
    "lo_digits_from_256": mis_lo_digits_from_256,
    "thread_255": mis_thread_255,
    "last_active_thread": mis_last_active_thread,
    "tiles_past_the_grid": mis_tiles_past_the_grid,
    "last_pixel": mis_last_pixel,
    "swap_across_bucket": mis_swap_across_bucket,
}


def misreading_distance(name, pixel, opl, r, g, b, ref, T):
    """(rel-L2 of the misread film from ref, support differs); (0.0, False): no effect at this case"""
    H, W = ref.shape[:2]
    npix = W * H
    moved_to = MISREADINGS[name](pixel, npix)
    tbin = bins_of(opl, T)
    m = (moved_to != pixel) & (tbin >= 0) & (tbin < T)
    if not m.any():
        return 0.0, False
    old, new, tb = pixel[m].astype(np.int64), moved_to[m].astype(np.int64), tbin[m]
    vals = np.stack([v[m].astype(np.float64) for v in (r, g, b)], axis=1)
    keys = np.concatenate([old * T + tb, (new * T + tb)[new < npix]])
    delta = np.concatenate([-vals, vals[new < npix]])
    cells, inv = np.unique(keys, return_inverse=True)
    diff = np.stack([np.bincount(inv, weights=delta[:, c], minlength=len(cells)) for c in range(3)], axis=1)
    at = ref.reshape(-1, 3)[cells]
    # (a cell all of whose records left holds an exact 0 in a film built without them; here it is ref - the same sum in
    # another order: anything below 1e-9 of a single contribution's scale counts as 0)
    mis = np.where(np.abs(at + diff) < 1e-9, 0.0, at + diff)
    support_differs = bool(np.any((mis != 0) != (at != 0)))
    return float(np.linalg.norm(mis - at) / np.linalg.norm(ref)), support_differs
