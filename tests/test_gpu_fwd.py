"""mtr_render_fwd on the GPU: k_fwd_paths against the host build of the same arithmetic (tests/host_fwd.cpp) at the same seed in its
four <SCENE_LDS, EXT> forms and both tiers — each case naming the instantiation and the tier it ran —, the shapes at which the row
scheme can go wrong, pixel ranges, the device-side duality with mtr_render_grad_tex, the kernel against the CPU oracle directly
(linearity, the degree identity with roulette active), forward-mode AD through mi.render, and the sample sub-range refusal.  Every
GPU step runs in a child process under its own time limit (tests/fwd_gpu_cases.py).

Bound against the host build: rel-L2 1e-5 on both tensors — only the f32 summation order differs (the host sums the same f32 terms
in f64), as in the primal's GPU <-> oracle bound."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


def run_case(case, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(HERE, "fwd_gpu_cases.py"), case], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, out)
    return out


def _matches_host(out):
    assert out["scale"] > 0 and out["finite"], out
    assert out["rel_s"] <= 1e-5 and out["rel_t"] <= 1e-5, out


@pytest.mark.parametrize("form", ["lds,plain", "lds,ext", "hbm,plain", "hbm,ext"])
def test_gpu_tangent_film_matches_host_build_in_every_instantiation(form):
    out = run_case(form)
    assert out["instantiation"] == out["expected"] == form and out["tier"] == "rows", out
    _matches_host(out)


@pytest.mark.parametrize("spp", [16, 24, 300])
def test_gpu_row_scheme_at_the_sample_counts_that_change_it(spp):
    """12 x 10 pixels: 16 spp — 16 pixels per run, the last run has 8; 24 spp — 10 pixels per run, 240 of 256 lanes; 300 spp —
    one pixel per run in two trips"""
    out = run_case(f"rows_{spp}")
    assert out["instantiation"] == "lds,plain" and out["tier"] == "rows", out
    _matches_host(out)


def test_gpu_more_runs_than_workgroups():
    out = run_case("many_runs")
    assert out["n_runs"] > out["grid_cap"] and out["tier"] == "rows", out
    _matches_host(out)


def test_gpu_pixel_ranges_compose_bit_for_bit_and_leave_the_rest_untouched():
    out = run_case("ranges")
    assert out["nonzero"] and out["no_sentinel_in_full"], out
    assert out["untouched"], out
    assert out["composed_equal"], out


def test_gpu_global_tier():
    out = run_case("global")
    assert out["tier"] == "global" and out["small_film_tier"] == "rows" and out["instantiation"] == "lds,plain", out
    _matches_host(out)


def test_gpu_forward_and_reverse_kernels_are_transposes():
    out = run_case("duality")
    assert out["instantiation"] == "lds,ext", out
    assert out["err"] <= 1e-5 and out["share"] > 0.1 and out["control"] > 1e-5, out


def test_gpu_radiance_tangent_gives_the_oracles_primal_film():
    out = run_case("oracle_linear")
    assert out["instantiation"] == "lds,ext" and out["scale"] > 0, out
    assert out["rel_s"] <= 1e-5 and out["rel_t"] <= 1e-5, out


def test_gpu_parameter_tangent_counts_the_oracles_vertices():
    out = run_case("oracle_degree")
    assert out["instantiation"] == "lds,plain" and out["n_terms"] > 1000 and out["depths"][1] >= 8, out
    assert out["rel_s"] <= 1e-5 and out["rel_t"] <= 1e-5, out
    assert out["control"] > 0.1, out


def test_gpu_forward_ad_through_mi_render_is_render_forward():
    """within 1e-5, not bit-equal: LDS float atomics are unordered"""
    out = run_case("forward_ad")
    assert out["has_tangents"] and out["seed_seen"] and out["shape_s"] == [10, 12, 3] and out["shape_t"] == [10, 12, 32, 3], out
    assert out["rel_s"] <= 1e-5 and out["rel_t"] <= 1e-5 and out["auto"] <= 1e-5, out
    assert out["scalar_scale"] > 0 and out["scalar"] <= 1e-5, out


def test_gpu_sample_sub_range_is_unsupported():
    out = run_case("sub_range")
    assert out["status"] == -5 and out["untouched"], out


def test_gpu_render_forward_maps_texel_tangents_of_two_bitmaps():
    """the Python layer's texel offsets (two bitmaps of different sizes): render_forward against mtr_render_fwd within 1e-5 —
    two renders agree to rounding only, LDS float atomics are unordered"""
    out = run_case("texel_keys")
    assert out["instantiation"] == "lds,ext" and out["scale"] > 0, out
    assert out["rel_s"] <= 1e-5 and out["rel_t"] <= 1e-5, out
    assert out["control"] > 1e-3, out


def test_gpu_crop_window():
    out = run_case("crop")
    assert out["instantiation"] == "lds,plain" and out["tier"] == "rows", out
    _matches_host(out)
    assert out["outside_untouched"] and out["shape_s"] == [5, 7, 3], out
    assert out["py_s"] <= 1e-5 and out["py_t"] <= 1e-5, out
