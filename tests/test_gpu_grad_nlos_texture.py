"""mtr_render_grad_tex on a NLOS scene on the GPU: k_grad_paths_nlos_tex, both tiers, against the host build of the same arithmetic
(tests/host_grad_nlos_tex.cpp) at the same seed on every CPU case of tests/test_grad_nlos_texture.py — each naming the tier and the
instantiation it ran —, its grid-stride loop, ranges and passes, the unchanged mtr_render_grad, the degree identity against the CPU
oracle directly, loss.backward() against render_backward and an Adam fit of a hidden albedo map through mi.render.  Every GPU step
runs in a child process under its own time limit (tests/grad_nlos_tex_gpu_cases.py).
The bounds come from the host build, the number formats and the CPU rehearsal; figures measured on an MI355X are not recorded yet."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_grad_nlos_texture as NT  # noqa: E402

pytestmark = pytest.mark.gpu


def run_case(case, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(HERE, "grad_nlos_tex_gpu_cases.py"), case], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_host(out, tier):
    assert out["tier"] == tier and out["instantiation"] == f"nlos,lds,ext,{tier}", out
    assert out["finite"] and out["device_ok"] and out["same_support"] and out["n_textures"] == 1 and out["texel_scale"] > 0, out
    assert out["rel_texels"] <= 1e-5 and out["rel_other"] <= 1e-5, out


# 4 x 3 and 8 x 4: the slab tier; 20 x 18 = 360 texels (above 8 KiB / 24 B = 341): the global tier
@pytest.mark.parametrize("size,tier,cases", [("4x3", "slab", list(NT.TEX_CASES)), ("8x4", "slab", ["confocal_ls_hg", "single_hg_wall"]),
                                             ("20x18", "global", list(NT.TEX_CASES))], ids=["4x3", "8x4", "20x18"])
def test_gpu_texel_gradients_match_host_build(size, tier, cases):
    """every CPU case: texels within 1e-5 of the largest texel gradient, materials and the laser within 1e-5 of themselves"""
    out = run_case(f"host:{size}:{','.join(cases)}")
    for c in cases:
        print(c, out[c])
    for c in cases:
        check_host(out[c], tier)


@pytest.mark.parametrize("size,tier", [("4x3", "slab"), ("20x18", "global")])
def test_gpu_grid_stride_loop(size, tier):
    out = run_case(f"grid_stride:{size}", timeout=600)
    print(out)
    assert out["n_lanes"] > 2 * out["grid_cap_lanes"] and out["n_lanes"] % 256 != 0, out
    assert out["tier"] == tier and out["instantiation"] == f"nlos,lds,ext,{tier}", out
    assert out["rel_texels"] <= 1e-5 and out["rel_other"] <= 1e-5, out


def test_gpu_ranges_and_passes_sum():
    out = run_case("passes")
    print(out)
    assert out["n_passes"] > 1 and out["nonzero"] and out["tier"] == "slab"
    assert out["split_rel"] <= 1e-5 and out["multi_rel"] <= 1e-5, out


def test_gpu_render_grad_is_unchanged_on_a_textured_scene():
    out = run_case("unchanged")
    print(out)
    assert out["same_as_tex"] and out["null_is_plain"] and out["textured_zero"] and out["n_textured"] == 1 and out["texels_written"], out
    assert out["rel_host"] <= 1e-5, out


@pytest.mark.parametrize("max_depth", [12, -1])
@pytest.mark.parametrize("case", list(NT.DEGREE_CASES))
def test_gpu_texel_gradients_have_the_degree_of_the_detached_estimator(case, max_depth):
    out = run_case(f"oracle_degree:{case}:{max_depth}")
    print(out)
    assert out["instantiation"] == "nlos,lds,ext,slab" and out["n_terms"] > 300 and out["deepest"] >= 3 and out["share"] > 0.05
    assert out["err"] <= 1.0, out
    assert out["control"] > 0.1, out


@pytest.mark.parametrize("tier", ["slab", "global"])
def test_gpu_autograd_is_render_backward(tier):
    out = run_case("autograd_" + tier)
    print(out)
    assert out["tier"] == tier and out["shape_ok"] and out["grad_fn"] and out["constant_equal"] and out["seed_seen"] and out["nonzero"] > 0.5, out
    if tier == "slab":
        assert out["equal"], out
    else:
        assert out["rel"] <= 1e-6, out


def test_gpu_adam_fits_a_hidden_albedo_map():
    """an 8 x 8 checker on the hidden quad from uniform grey: Confocal, laser and hidden-geometry sampling, 8 x 8 x 256 bins x 64 spp,
    60 steps.  The CPU rehearsal (test_grad_nlos_texture.test_adam_rehearsal_on_the_cpu: oracle primal, host-build gradients) has the
    loss at the target's seed fall by 7.4 and the mean texel error — over all texels: each receives gradient — from 0.283 to 0.174;
    asserted here: half that factor and half that fall"""
    out = run_case("adam", timeout=600)
    print(out)
    assert out["tier"] == "slab"
    assert out["factor"] >= NT.ADAM_FACTOR / 2, out
    assert out["texel_err_last"] <= NT.ADAM_ERR_FIRST - (NT.ADAM_ERR_FIRST - NT.ADAM_ERR_LAST) / 2, out
