"""The numerics contract on the device, function by function: every MTR_HD family of mtr_core.h that tests/kat_cases.py lists — the
special functions, the trigonometric restatements and phasor_term, the warps and frames, the Fresnel terms and the angular falloff,
every BSDF's eval / pdf / sample, the generator, the film's bin mapping and the pair helpers — evaluated by the library's device
harness (mitransient_amd/csrc/mtr_kat.hip) under BOTH of the Makefile's flag sets (suffix "": as the wavefront, gradient, tint,
samples and reconstruction files see the header; "_k": as k_fused sees it) and compared with the host build of the same header
(tests/host_harness.cpp) word for word: equal bits, NaNs of any payload equal.  tests/test_kat_cases.py holds that host build to the
oracle and to f64, and shows that the inputs reach every branch.  Each family runs in ONE child process under its own time limit
(tests/kat_gpu_cases.py): full size, n = 1 and n = 63, both flag sets."""
import functools
import json
import os
import subprocess
import sys

import pytest

import kat_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

# the one function whose device form differs from the host's ON PURPOSE (mtr_core.h safe_rcp: the hardware reciprocal, for culling)
BY_DESIGN = "safe_rcp"


@functools.lru_cache(maxsize=None)
def run_family(family, timeout=120):
    r = subprocess.run([sys.executable, os.path.join(HERE, "kat_gpu_cases.py"), family], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("suffix", K.SUFFIXES, ids=["others", "kflags"])
@pytest.mark.parametrize("family", K.FAMILIES)
def test_device_equals_host_bit_for_bit(family, suffix):
    out = run_family(family)
    n_cases = len(K.cases(family))
    assert out["runs"] == n_cases * len(K.SUFFIXES) * (1 + len(K.SMALL_N)) and out["words"] > 0, out["runs"]
    bad = {k: v for k, v in out["failures"].items() if k.endswith("|" + suffix) and k.split("|")[0] != BY_DESIGN}
    assert not bad, f"{family}, flag set '{suffix}': {len(bad)} case(s) differ from the host build\n" + "\n".join(bad.values())
    print(f"[kat] {family} '{suffix}': {n_cases} cases, {out['words'] // len(K.SUFFIXES)} words equal")


@pytest.mark.xfail(strict=True, reason="safe_rcp is v_rcp_f32 on the device and a correctly rounded 1 / x on the host, as mtr_core.h says: on the "
                   "MI355X 20779 of 200003 inputs differ under either flag set, by one ulp (3.0: host 3eaaaaab, device 3eaaaaaa) and, where the "
                   "result is a denormal, by a flush to zero (FLT_MAX: host 00200000, device 00000000).  Taking the host's form on the device "
                   "would put a ~10-instruction division into every slab test of k_fused (HISTORY.md)")
@pytest.mark.parametrize("suffix", K.SUFFIXES, ids=["others", "kflags"])
def test_safe_rcp_equals_host_bit_for_bit(suffix):
    out = run_family("warps")
    key = f"{BY_DESIGN}|{suffix}"
    assert key not in out["failures"], out["failures"][key]


@pytest.mark.parametrize("suffix", K.SUFFIXES, ids=["others", "kflags"])
def test_safe_rcp_is_within_what_the_header_states(suffix):
    """what mtr_core.h does promise of safe_rcp on the device: the hardware reciprocal, 1 ulp.  Every result the host has as a normal
    float is within one ulp of it; a result below FLT_MIN (|x| > 8.5e37: no direction has such a component) may be flushed to a zero of
    the same sign; zeros, denormals, infinities, NaN and the clamp at 1e28 come out as on the host — no other kind of difference"""
    d = run_family("warps")["extra"][f"{BY_DESIGN}|{suffix}"]
    print(f"[kat] safe_rcp '{suffix}': {d}")
    assert d["max_ulp"] <= 1 and d["other"] == 0, d
