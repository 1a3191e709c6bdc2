"""The word-to-segment rule of k_grad_reduce (mitransient_amd/csrc/mtr_grad_reduce.h: grad_reduce_segment) on the CPU, through
tests/host_grad_reduce.cpp: word i of a workgroup's row goes to exactly the output and offset that the three reduce kernels it
replaces wrote — k_grad_reduce (materials, emitters), k_grad_reduce_tex and k_grad_reduce_tint (a third segment behind them) —
and an empty segment, whose pointer may be NULL, is never chosen."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 3, 7)


def build_host_grad_reduce():
    """tests/host_grad_reduce.cpp into tests/_build/, as tests/test_splat_plan.py builds its host library"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_grad_reduce.so")
    deps = [os.path.join(ROOT, "tests", "host_grad_reduce.cpp"), os.path.join(ROOT, "mitransient_amd", "csrc", "mtr_grad_reduce.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", tmp, deps[0]], check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hgr():
    lib = C.CDLL(build_host_grad_reduce())
    lib.hgr_segment.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.hgr_segment.restype = C.c_uint32
    return lib


def old_kernels(n_m, n_e, n_x, i):
    """(segment, offset) as the removed kernels routed word i: `if (i < n_m) mats[i]; else if (i < n_m + n_e) ems[i - n_m];
    else third[i - n_m - n_e]` — k_grad_reduce itself had no third branch, its rows no third segment"""
    if i < n_m:
        return 0, i
    if n_x == 0 or i < n_m + n_e:
        return 1, i - n_m
    return 2, i - n_m - n_e


@pytest.mark.parametrize("n_m,n_e,n_x", list(itertools.product(LENGTHS, repeat=3)), ids=lambda v: str(v))
def test_every_word_goes_where_the_old_kernels_put_it(hgr, n_m, n_e, n_x):
    lengths = (n_m, n_e, n_x)
    hits = [[0] * n for n in lengths]
    for i in range(n_m + n_e + n_x):
        off = C.c_uint32(0xffffffff)
        seg = hgr.hgr_segment(n_m, n_e, n_x, i, C.byref(off))
        assert (seg, off.value) == old_kernels(n_m, n_e, n_x, i), (lengths, i)
        assert lengths[seg] > 0 and off.value < lengths[seg], (lengths, i)      # an empty segment is never chosen
        hits[seg][off.value] += 1
    assert all(h == 1 for seg in hits for h in seg)                             # every output word written exactly once
