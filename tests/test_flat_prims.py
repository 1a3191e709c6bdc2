"""The child-ordered primitive table of k_fused's lean flat-walk kernels (mitransient_amd/csrc/mtr_flat_prims.h: which entry a
root child and a box face take, where record and first-slot word lie, how many bytes the table needs) on the CPU, through
tests/host_flat_prims.cpp: EVERY top level a FlatTop can describe — 0..8 rectangles, 0..4 boxes.  A table that overran its bytes
would write into the staged tree behind it; the kernel carves and fused_plan reserves by the same function of this header."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitransient_amd", "csrc")
DEPS = [os.path.join(ROOT, "tests", "host_flat_prims.cpp"), os.path.join(CSRC, "mtr_flat_prims.h")]


class Out(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("entries", "bytes", "live", "collisions", "out_of_bounds", "misaligned", "unstaged", "slack")]


def _build(name, flags):
    """tests/host_flat_prims.cpp into tests/_build/, as tests/test_splat_plan.py builds its host library"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name)
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall"] + flags + ["-o", tmp, DEPS[0]], check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hfp():
    lib = C.CDLL(_build("libhost_flat_prims.so", ["-fPIC", "-shared"]))
    lib.hfp_check.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(Out)]
    lib.hfp_check.restype = None
    return lib


@pytest.mark.parametrize("n_boxes", range(5))
def test_every_top_level(hfp, n_boxes):
    """n_quads in 0..8 with this many boxes: no two entries share a byte, no two live primitives share an entry, records are
    16-byte aligned (ds_read_b128) and words 4-byte aligned, everything lies inside the planned bytes, and those are
    (8 + 6 n_boxes) entries of 84 bytes rounded to 16 — 1 680 for the Cornell box's two cubes"""
    for n_quads in range(9):
        o = Out()
        hfp.hfp_check(n_quads, n_boxes, C.byref(o))
        assert o.entries == 8 + 6 * n_boxes and o.live == n_quads + 6 * n_boxes
        assert (o.collisions, o.out_of_bounds, o.misaligned, o.unstaged) == (0, 0, 0, 0), (n_quads, n_boxes)
        assert o.bytes == (84 * o.entries + 15) // 16 * 16 and o.bytes % 16 == 0
        assert o.slack < 16                       # the last word ends in the table's last 16 bytes: nothing reserved for nobody
    if n_boxes == 2:
        assert o.bytes == 1680
    if n_boxes == 4:
        assert o.entries == 32 and o.bytes == 2688       # the table's end: face entry 8 + 23


def test_plan_and_kernel_size_the_table_by_one_function():
    """fused_plan's bytes are the kernel's: both call flat_prim_bytes on the scene's box count, under one predicate
    (flat_prim_table_on for the instantiation, fused_lean_flat_quads for the launch that picks it)"""
    src = open(os.path.join(CSRC, "mtr_kernels.hip")).read()
    assert len(re.findall(r"\bflat_prim_bytes\(", src)) == 2
    assert "off += flat_prim_bytes(nb)" in src and "const uint32_t nb = a.sc.flat.n_boxes" in src           # the kernel's carve-up
    assert "flat_prim_bytes(sc.flat.n_boxes)" in src                                                       # fused_plan's reservation
    assert src.count("fused_lean_flat_quads(") == 3          # its definition, fused_plan's use (fused_prim_table_bytes), launch_fused_s's
    assert src.count("flat_prim_table_on(") == 2             # the kernel's instantiations, the plan
    core = open(os.path.join(CSRC, "mtr_core.h")).read()
    assert "root - flat_prim_bytes(n_boxes)" in core         # flat_prim_fetch: the table ends where the tree begins


def test_stand_alone_sweep_under_sanitizers():
    """the same sweep as a program of its own, built with AddressSanitizer and UBSan (host code only; nothing is loaded into Python;
    the runtimes are linked statically, so the program needs nothing of its environment)"""
    exe = _build("host_flat_prims_san", ["-DHFP_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                         "-static-libasan", "-static-libubsan"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
