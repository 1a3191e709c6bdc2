"""SHADOW HULL on the CPU (mitransient_amd/csrc/mtr_shadow_hull.h; mtr_core.h flat_walk_device): a shadow ray that shade_hit aims at
the scene's one rectangular emitter E is spared the rectangle tests it provably cannot pass.  tests/host_shadow_hull.cpp runs the host
builds of what the kernel runs — offset_point, rect_emitter_point, shadow_ray_to, trav_quad_test, hull_side — and of what the host
decides (classify_scene -> shadow_hull_classify):

  * which scenes are such rooms (shadow_hull_cases.py): the Cornell box and its copies times 100 and 0.01, the light on a side wall,
    a seventh rectangle across the open side; not with a second emitter, the light in the ceiling's plane or touching a wall, a partition, a cube through the floor;
  * the claim itself, over 10^7 (origin, endpoint) pairs — uniform on walls, box faces and E, and adversarial: 0 .. 64 ulps from the
    walls' edges and corners and from E's, the strips of the walls around E's plane down to 1/4096 of delta_E — each pair asserted:
    hull-safe => no wall's plane reports a hit, E-safe => E reports none (both with the rectangle's bounds and with the plane alone);
  * that the sweep is not vacuous: of the uniform wall origins that cast a shadow ray at least 0.999 are hull-safe and 0.98 E-safe,
    the adversarial origins hold risky cases of both kinds, and in the turned room — no zero in any row, every rounding live — the
    tests DO report hits on the walls' planes and on E for risky origins;
  * that with the margin at 128 every origin on a wall of the unit room is hull-risky (the GPU tests' "stage unchanged" tier)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import shadow_hull_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitransient_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "host_shadow_hull.cpp"), os.path.join(CSRC, "mtr_scene_host.cpp"), os.path.join(CSRC, "mtr_bvh.cpp")]
DEPS = SRCS + [os.path.join(CSRC, h) for h in ("mtr_shadow_hull.h", "mtr_core.h", "mtr_scene_host.h", "mtr_bvh.h", "mtr_flat_prims.h")]
FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fno-fast-math", "-mfma"]      # (the host harness's numerics)


class Hull(C.Structure):
    _fields_ = [("count", C.c_uint32), ("e_child", C.c_uint32), ("e_delta", C.c_float), ("pad", C.c_float), ("e_row", C.c_float * 4),
                ("delta", C.c_float * 8), ("row", (C.c_float * 4) * 8)]


def _build(name, flags):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name)
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++"] + FLAGS + flags + ["-o", tmp] + SRCS + ["-lpthread"], check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hsh():
    lib = C.CDLL(_build("libhost_shadow_hull.so", ["-O2", "-fPIC", "-shared"]))
    lib.hsh_classify.argtypes = [C.c_void_p, C.POINTER(Hull)]
    return lib


def _classify(hsh, d):
    import mitransient_amd.mi as mi
    assert C.sizeof(Hull) == 192
    scene = mi.load_dict(d)
    desc = scene.data().desc()
    h = Hull()
    assert hsh.hsh_classify(C.byref(desc), C.byref(h)) == 0
    return h


@pytest.mark.parametrize("name", list(cases.ON))
def test_rooms_that_are_on(hsh, name):
    h = _classify(hsh, cases.ON[name]())
    assert h.count == cases.HULL_RECTANGLES[name]
    assert 0.0 < h.e_delta and all(h.delta[k] > 0.0 for k in range(h.count)) and all(h.delta[k] == 0.0 for k in range(h.count, 8))
    for k in range(h.count, 8):
        assert list(h.row[k]) == [0.0, 0.0, 0.0, 1.0]          # an unused row is safe for every origin


def test_the_guard_distances_scale_with_the_room(hsh):
    """delta_E is millimetres in the unit Cornell box (a few 1e-6 (M + D) / kShadowEps) and scales with the room"""
    h1, h100, h001 = (_classify(hsh, cases.ON[k]()) for k in ("cornell", "scaled-100", "scaled-0.01"))
    assert 1e-3 < h1.e_delta < 9e-3
    assert 50.0 < h100.e_delta / h1.e_delta < 200.0 and 0.005 < h001.e_delta / h1.e_delta < 0.02
    assert max(h1.delta) < 1e-5


@pytest.mark.parametrize("name", list(cases.OFF))
def test_rooms_that_are_off(hsh, name):
    assert _classify(hsh, cases.OFF[name]()).count == 0


def _run(exe, pairs):
    r = subprocess.run([exe, str(pairs)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    return r


def test_the_sweep():
    """the stand-alone program over 10^7 pairs: its own classification of the rooms of host_shadow_hull.cpp, every pair asserted, the
    shares that keep the sweep from being vacuous, the margin of 128 (module docstring); it prints one line per room"""
    r = _run(_build("host_shadow_hull", ["-O2", "-DHSH_MAIN"]), 10 ** 7)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
    rooms = re.findall(r"room \(([^)]*)\): (\d+) pairs, violations hull (\d+) E (\d+).*?hits reported: walls' planes (\d+) E (\d+)", r.stdout)
    assert len(rooms) == 7 and sum(int(x[1]) for x in rooms) >= 10 ** 7
    assert all(int(x[2]) == 0 and int(x[3]) == 0 for x in rooms)
    turned = [x for x in rooms if x[0].endswith(", 7")]
    assert turned and all(int(x[4]) > 0 and int(x[5]) > 0 for x in turned)          # the tests do report hits for risky origins


def test_stand_alone_sweep_under_sanitizers():
    """the same program built with AddressSanitizer and UBSan (host code only; nothing is loaded into Python; the runtimes are linked
    statically), over 10^6 pairs"""
    exe = _build("host_shadow_hull_san", ["-O1", "-g", "-DHSH_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                          "-static-libasan", "-static-libubsan"])
    r = _run(exe, 10 ** 6)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
