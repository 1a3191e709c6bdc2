"""The path-start table of k_fused's lean flat-walk kernels (mitransient_amd/csrc/mtr_start_blocks.h: how a ticket of n_lanes samples
is cut into blocks of 64, how many entries the last block holds, how many bytes a launch's table takes and where the record of
(workgroup, wave, entry) lies) on the CPU, as the library compiled it (mtr_test_start_blocks, mtr_test_start_blocks_sweep) and as a
stand-alone program under sanitizers.  The context allocates and the kernel indexes by the same functions of this header."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitransient_amd", "csrc")
DEPS = [os.path.join(ROOT, "tests", "host_start_blocks.cpp"), os.path.join(CSRC, "mtr_start_blocks.h")]


@pytest.fixture(scope="module")
def lib():
    from mitransient_amd import _cabi
    lib = _cabi.load_library()
    lib.mtr_test_start_blocks.argtypes = [C.c_uint32] * 6 + [C.POINTER(C.c_uint32)]
    lib.mtr_test_start_blocks.restype = None
    lib.mtr_test_start_blocks_sweep.argtypes = [C.c_uint32] * 4
    lib.mtr_test_start_blocks_sweep.restype = C.c_int
    return lib


def _one(lib, n_lanes, grid, wg, wave, entry, base):
    out = (C.c_uint32 * 7)()
    lib.mtr_test_start_blocks(n_lanes, grid, wg, wave, entry, base, out)
    return dict(blocks=out[0], last=out[1], bytes=out[2] | out[3] << 32, off=out[4] | out[5] << 32, entries=out[6])


def test_every_ticket_length_and_every_grid(lib):
    """every n_lanes in [1, 2^16 + 1]: ceil(n / 64) blocks, 1..64 entries in the last, the blocks' entries add up to n, none beyond the
    end; every grid in 1..1024: the records of all its waves tile the table in ascending order — none out of range, no two overlap,
    no byte left over — and the context's sixteen tables, whose stride comes from the allocation and not from a launch: a table of
    any smaller grid in slot s ends before slot s + 1 begins, so launches of different grids in flight never share a record"""
    assert lib.mtr_test_start_blocks_sweep(1, (1 << 16) + 1, 1, 1024) == 0


def test_spot_values(lib):
    """config 2's launch: 1024 workgroups of four waves, 48-byte records: 12 MiB a table; a ticket of 32 pixels x 1024 spp is 512 blocks"""
    r = _one(lib, 32 * 1024, 1024, 1023, 3, 63, 0)
    assert r["blocks"] == 512 and r["last"] == 64 and r["entries"] == 64
    assert r["bytes"] == 1024 * 4 * 64 * 48 == 12 << 20 and r["off"] == r["bytes"] - 48
    r = _one(lib, 48, 1, 0, 1, 0, 64)              # 3 x 2 pixels x 8 spp: one ragged block, wave 1's block is beyond the end
    assert (r["blocks"], r["last"], r["entries"], r["off"]) == (1, 48, 0, 64 * 48)
    assert _one(lib, 1311, 1, 0, 0, 0, 1280)["entries"] == 31 and _one(lib, 1311, 1, 0, 0, 0, 0)["blocks"] == 21
    assert _one(lib, 0xffff0000, 1, 0, 0, 0, 0xfffeffc0)["entries"] == 64          # the largest ticket fused_plan accepts


def test_stand_alone_sweep_under_sanitizers():
    """the header alone in a program of its own, built with AddressSanitizer and UBSan (host code only; nothing is loaded into
    Python; the runtimes are linked statically): every record of seven grids written into a table of exactly the planned bytes"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "host_start_blocks_san")
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS)):
        tmp = exe + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", tmp, DEPS[0]], check=True)
        os.replace(tmp, exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
