"""The white-furnace identity on the MI355X: mtr_render in both organisations and with deterministic rows, scenes staged in LDS
and walked in HBM, the extended shading code, the polarized bounce kernel, mtr_render_grad / mtr_render_grad_tex / mtr_render_fwd
— against the closed forms of tests/furnace_cases.py (no oracle), 64 x 64 pixels at 256 spp — and the camera configurations of
tests/test_furnace.py against the oracle at the suite's 1e-5.  Every test names the kernel organisation, tier or instantiation
it reached.  Every GPU step runs in a child process under its own time limit (tests/furnace_cases.py)."""
import json
import os
import subprocess
import sys

import pytest

import furnace_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


def run_case(*case, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(HERE, "furnace_cases.py"), *case], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check(vs, label):
    for k, v in vs.items():
        FC.assert_verdict(v, f"{label} {k}")
    print(f"[furnace] {label}: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs.values()))


def steady(out):
    return {k: out[k] for k in ("steady", "time_sum") if k in out}


ORGANISATION = {"fused": "fused", "deterministic": "fused", "wavefront": "wavefront"}


@pytest.mark.parametrize("org", ["fused", "wavefront", "deterministic"])
def test_gpu_orders(org):
    """max_depth 1 exactly, 2, 3, 4, 6, each order's own term, roulette at max_depth 6 and L_inf — the steady image and the
    transient film summed over time; the flat-top, several-emitter k_fused, the wavefront kernels, deterministic rows"""
    out = run_case("orders", org)
    info = out["info"]
    assert info["organisation"] == ORGANISATION[org] and info["tables"] == "lds", info
    assert info["flat_top"] and info["diffuse"] and not info["one_rect_emitter"], info
    spp = FC.GPU_SIZE[1]
    assert out["d1_max_rel"] <= spp * 2.0 ** -24 and out["d1_time_sum_max_rel"] <= spp * 2.0 ** -24, out
    # four orders and max_depth 6 under roulette, each as the steady image and as the time sum; three differences; L_inf
    assert sorted(out["cases"]) == sorted([f"D{d}{t}" for d in ("2", "3", "4", "6", "6_rr2") for t in ("", "_time_sum")] +
                                          ["D2-D1", "D3-D2", "D4-D3", "inf_rr3"]), sorted(out["cases"])
    check(out["cases"], f"gpu orders {org}")


@pytest.mark.parametrize("org", ["fused", "wavefront"])
def test_gpu_lossless_inclusions(org):
    """a glass cube, a thin-dielectric pane, both, a two-sided wall, two walls built outward with flip_normals: L_inf stays"""
    outs = run_case("inclusions", org)
    assert sorted(outs) == sorted(FC.INCLUSIONS)
    for name, out in outs.items():
        assert out["info"]["organisation"] == org and out["info"]["tables"] == "lds" and out["info"]["flat_top"], out["info"]
        assert out["info"]["diffuse"] == (name == "flip_normals"), out["info"]       # (the kTrDiffuse kernels: one-sided diffuse alone)
        check(steady(out), f"gpu inclusion {name} {org}")


@pytest.mark.parametrize("which,org,tables", [("small", "fused", "lds"), ("small", "wavefront", "lds"), ("large", "wavefront", "hbm"),
                                              ("large", "fused", "hbm"), ("mixed", "wavefront", "lds"), ("mixed", "fused", "lds")])
def test_gpu_mesh_emitter_room(which, org, tables):
    """the mesh emitter staged in LDS and walked in HBM (8-wide nodes, shadow lists, deferred commit); AUTO sends the large
    room, whose tables leave LDS, to the wavefront organisation"""
    out = run_case("mesh", which, org)
    assert out["info"]["organisation"] == org and out["info"]["tables"] == tables, out["info"]
    assert not out["info"]["flat_top"] and not out["info"]["no_lobes"], out["info"]          # a tree to walk, the plain shading code
    if which == "large":
        assert out["auto"] == "wavefront" and out["info"]["n_tris"] > 852, out
    check(steady(out), f"gpu mesh {which} {org}")


@pytest.mark.parametrize("org", ["fused", "wavefront"])
@pytest.mark.parametrize("which", ["bitmap", "lobes"])
def test_gpu_extended_shading(which, org):
    """rho as a bitmap: the extended shading code without lobes (kTrNoLobes); with a rough conductor in the scene, with them"""
    out = run_case("extended", which, org)
    assert out["info"]["organisation"] == org and out["needs_ext"], out
    assert out["info"]["no_lobes"] == (which == "bitmap") and not out["info"]["diffuse"], out["info"]
    check(steady(out), f"gpu extended {which} {org}")


@pytest.mark.parametrize("glass", ["empty", "glass"])
def test_gpu_polarized_room_stays_unpolarized(glass):
    out = run_case("polarized", glass)
    assert out["info"]["organisation"] == "wavefront" and out["info"]["scatter_launches"] > 0, out["info"]
    check({k: out[k] for k in ("S0", "S123", "steady")}, f"gpu polarized {glass}")


@pytest.mark.parametrize("which,instantiation", [("lds_D4", "lds,plain"), ("lds_inf", "lds,plain"), ("hbm_inf", "hbm,plain")])
def test_gpu_reverse_mode_sums(which, instantiation):
    out = run_case("grad", which)
    assert out["instantiation"] == instantiation, out
    check({k: out[k] for k in ("d_rho", "d_le")}, f"gpu reverse {which}")


def test_gpu_reverse_mode_texel_sums():
    out = run_case("grad_tex")
    assert out["instantiation"] == "lds,ext" and out["tier"] == "slab" and out["n_textures"] >= 1, out
    check({k: out[k] for k in ("d_rho", "d_le")}, "gpu reverse texels")


@pytest.mark.parametrize("which,instantiation", [("lds_D4", "lds,plain"), ("lds_inf", "lds,plain"), ("hbm_inf", "hbm,plain")])
def test_gpu_forward_mode_tangent_images(which, instantiation):
    out = run_case("fwd", which)
    assert out["instantiation"] == instantiation and out["tier"] == "rows", out
    check({k: out[k] for k in ("d_rho", "d_le")}, f"gpu forward {which}")


@pytest.mark.parametrize("org", ["fused", "wavefront"])
def test_gpu_camera_configurations(org):
    """every fov_axis, wide and tall films, crop windows: the D = 2 room against the oracle at the same seed"""
    outs = run_case("cameras", org)
    assert sorted(outs) == sorted(FC.CAMERAS)
    for name, out in outs.items():
        assert out["info"]["organisation"] == org and out["scale"] > 0, (name, out)
        assert out["rel_t"] <= 1e-5 and out["rel_s"] <= 1e-5, (name, out)
