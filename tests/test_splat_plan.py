"""The plan of mtr_splat_add's partition path (mitransient_amd/csrc/mtr_splat_plan.h: digit split of the pixel index,
workspace layout, support rule) on the CPU, through tests/host_splat_plan.cpp: EVERY pixel count the path supports, and the
support rule against the 32-bit record key — the part of the path that no GPU test can reach (a film whose key fills 32 bits
has 8 GiB or more)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_PIX = 1 << 22
BLOCK = 256                      # threads of a workgroup: tile_scan_claim gives each ceil(n_digits / 256) digit counters


class PlanOut(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("supported", "bits_pix", "bits_lo", "n_lo", "n_hi", "rec_a", "rec_b", "hist_hi", "base_hi",
                                          "starts", "cur_lo", "block_sums", "n_scan", "total_bytes")]


class SweepOut(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("checked", "bad_supported", "bad_digits", "bad_bits", "bad_layout", "bad_scan",
                                          "max_n_lo", "max_n_hi", "max_n_scan", "min_spare_words", "max_spare_words")]


def build_host_splat_plan():
    """tests/host_splat_plan.cpp into tests/_build/, as tests/test_polarized.py builds its host library"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_splat_plan.so")
    deps = [os.path.join(ROOT, "tests", "host_splat_plan.cpp"), os.path.join(ROOT, "mitransient_amd", "csrc", "mtr_splat_plan.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", tmp, deps[0]], check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hsp():
    lib = C.CDLL(build_host_splat_plan())
    lib.hsp_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(PlanOut)]
    lib.hsp_plan.restype = None
    lib.hsp_sweep.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(SweepOut)]
    lib.hsp_sweep.restype = None
    return lib


def plan(lib, width, height, bins, n, n_freq=0):
    o = PlanOut()
    lib.hsp_plan(width, height, bins, n_freq, n, C.byref(o))
    return o


def per(n_digits):
    return (n_digits + BLOCK - 1) // BLOCK


@pytest.mark.parametrize("n", [1, 4097, 1 << 22])
def test_every_supported_pixel_count(hsp, n):
    """every npix in [2, 2^22]: both digit counts fit the 2048 LDS counters and cover the film with no empty bucket, every
    region of the workspace (as the kernels and the memsets touch it) lies inside total_bytes before the next one, and the
    scan writes no more block sums than are reserved; one pixel more is not supported — and would need 2049 counters"""
    o = SweepOut()
    hsp.hsp_sweep(2, MAX_PIX, 2, n, C.byref(o))
    assert o.checked == MAX_PIX - 1
    assert (o.bad_supported, o.bad_digits, o.bad_bits, o.bad_layout, o.bad_scan) == (0, 0, 0, 0, 0)
    assert o.max_n_lo == 2048 and o.max_n_hi == 2048 and o.max_n_scan == 1025
    # 79 words lie between the last block sum and the end of the workspace, at every size
    assert (o.min_spare_words, o.max_spare_words) == (79, 79)
    beyond = plan(hsp, MAX_PIX + 1, 1, 2, n)
    assert not beyond.supported and beyond.n_hi == 2049 and beyond.n_lo == 2048


# npix, bits_pix, n_lo, n_hi, per_hi, per_lo
TABLE = [(65536, 16, 256, 256, 1, 1), (65538, 17, 256, 257, 2, 1), (262144, 18, 512, 512, 2, 2), (262656, 19, 512, 513, 3, 2),
         (1049600, 21, 1024, 1025, 5, 4), (1 << 22, 22, 2048, 2048, 8, 8)]


@pytest.mark.parametrize("row", TABLE, ids=[str(r[0]) for r in TABLE])
def test_digit_table(hsp, row):
    """the sizes at which tile_scan_claim gives a thread more than one digit counter, and a ragged last thread"""
    npix, bits_pix, n_lo, n_hi, per_hi, per_lo = row
    p = plan(hsp, npix, 1, 8, 1 << 20)
    assert p.supported
    assert (p.bits_pix, p.n_lo, p.n_hi, per(p.n_hi), per(p.n_lo)) == (bits_pix, n_lo, n_hi, per_hi, per_lo)
    assert p.bits_lo == bits_pix // 2 and p.n_scan == (npix + 1 + 4095) // 4096


# W, H of tests/splat_cases.py's table -> (n_lo, n_hi): what tests/test_gpu_splat_large_films.py says each case reaches
@pytest.mark.parametrize("W,H,n_lo,n_hi", [(256, 256, 256, 256), (331, 198, 256, 257), (512, 256, 256, 512), (512, 512, 512, 512),
                                           (513, 512, 512, 513), (1024, 1024, 1024, 1024), (1025, 1024, 1024, 1025),
                                           (2048, 1024, 1024, 2048), (2048, 2048, 2048, 2048)])
def test_width_times_height(hsp, W, H, n_lo, n_hi):
    p = plan(hsp, W, H, 8, 1 << 20)
    q = plan(hsp, W * H, 1, 8, 1 << 20)
    assert p.supported and (p.n_lo, p.n_hi) == (n_lo, n_hi)
    assert all(getattr(p, k) == getattr(q, k) for k, _ in PlanOut._fields_)


def bit_width(count):
    """bits that hold every index below count, at least one"""
    return max(1, (count - 1).bit_length())


def predicate(npix, bins, n, n_freq=0):
    """the support rule, written apart from the header: no phasor film; 0 < n < 2^32 - 1 (record offsets are u32, and the
    histogram's total must be one); 2 <= npix <= 2^22 (LDS counters); pixel and bin fields fit 32 bits together and the
    largest key is not the sentinel; a row of 3 f32 per bin fits 150 KiB of LDS"""
    if n_freq or n == 0 or n >= 0xffffffff or npix < 2 or npix > MAX_PIX:
        return False
    bp, bb = bit_width(npix), bit_width(bins)
    if bp + bb > 32:
        return False
    if ((npix - 1) | ((bins - 1) << bp)) == 0xffffffff:
        return False
    return bins * 12 <= 150 * 1024


def grid(limit):
    out = {1, limit + 1}
    k = 1
    while (1 << k) - 1 <= limit:
        out.update(v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 1 <= v <= limit)
        k += 1
    return sorted(out)


def test_support_rule_and_record_key(hsp):
    """bins in {1, 2^k - 1, 2^k, 2^k + 1 up to 12800, 12801} x npix in {2^k - 1, 2^k, 2^k + 1}: `supported` is the rule, and
    the largest key of every supported shape, (npix - 1) | (bins - 1) << bits_pix, fits 32 bits and is not 0xffffffff"""
    all_bins = sorted(set(grid(12800)) | {12800})            # 12800 bins: the longest row that fits LDS
    all_pix = [v for v in grid(MAX_PIX) if v >= 2]
    assert {1, 8191, 8192, 8193, 12800, 12801} <= set(all_bins) and {3, 4, 5, MAX_PIX - 1, MAX_PIX, MAX_PIX + 1} <= set(all_pix)
    n_supported = n_refused = 0
    refused_for_sentinel = []
    for npix in all_pix:
        for bins in all_bins:
            p = plan(hsp, npix, 1, bins, 1000)
            want = predicate(npix, bins, 1000)
            assert bool(p.supported) == want, (npix, bins)
            if p.supported:
                n_supported += 1
                key = (npix - 1) | ((bins - 1) << p.bits_pix)
                assert key < 0xffffffff, (npix, bins, hex(key))
                assert (npix - 1) >> p.bits_pix == 0                     # the fields do not overlap
            else:
                n_refused += 1
                if npix <= MAX_PIX and bins <= 12800 and bit_width(npix) + bit_width(bins) == 32:
                    refused_for_sentinel.append((npix, bins))
    assert n_supported > 1000 and n_refused > 100
    # the shapes of the grid whose last pixel's last bin would be the sentinel: both counts powers of two, 32 bits in all
    assert refused_for_sentinel == [(1 << 19, 8192), (1 << 20, 4096), (1 << 21, 2048), (1 << 22, 1024)]
    assert plan(hsp, 1 << 22, 1, 1023, 1000).supported and plan(hsp, (1 << 22) - 1, 1, 1024, 1000).supported
    assert plan(hsp, 1 << 22, 1, 1025, 1000).supported == 0           # 11 bin bits: 33 in all
    assert plan(hsp, 1 << 21, 1, 2048, 1000).supported == 0 and plan(hsp, 1 << 21, 1, 2047, 1000).supported


def test_unsupported_calls(hsp):
    ok = plan(hsp, 512, 512, 1024, 1 << 20)
    assert ok.supported
    assert not plan(hsp, 512, 512, 1024, 0).supported
    assert plan(hsp, 512, 512, 1024, 0xfffffffe).supported
    assert not plan(hsp, 512, 512, 1024, 0xffffffff).supported
    assert not plan(hsp, 512, 512, 1024, 1 << 32).supported
    assert not plan(hsp, 1, 1, 8, 1000).supported and not plan(hsp, 0, 7, 8, 1000).supported
    assert plan(hsp, 2, 1, 8, 1000).supported
    assert plan(hsp, 2048, 2048, 2, 1000).supported
    assert not plan(hsp, 2049, 2048, 2, 1000).supported and not plan(hsp, 65536, 65536, 2, 1000).supported
    assert not plan(hsp, 512, 512, 1, 1000, n_freq=3).supported            # a phasor film


def test_workspace_size_is_the_published_32_bytes_per_contribution(hsp):
    """the workspace: two 16-byte records per contribution plus tables of a few words per pixel"""
    for W, H, n in [(512, 512, 1 << 22), (2048, 2048, 1 << 21), (331, 198, 12345)]:
        p = plan(hsp, W, H, 8, n)
        npix = W * H
        assert p.total_bytes == 32 * n + 4 * (4096 + 2 * npix + npix // 4096 + 128)
        assert p.rec_b - p.rec_a == 16 * n and p.hist_hi == 32 * n
