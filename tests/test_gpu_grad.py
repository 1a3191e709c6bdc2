"""mtr_render_grad on the GPU: the kernel's gradients against the host build of the same arithmetic (tests/host_grad.cpp) at the
same seed on every CPU case of tests/test_grad.py and tests/test_grad_general.py — the four instantiations of k_grad_paths, each
case naming the one it ran —, its grid-stride loop, the kernel against the CPU oracle directly (emitter coefficients, the degree
identity with roulette active), renders split into ranges and passes, loss.backward() against render_backward, and an Adam
optimisation through mi.render and torch autograd.  Every GPU step runs in a child process under its own time limit
(tests/grad_gpu_cases.py)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


def run_case(case, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(HERE, "grad_gpu_cases.py"), case], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", ["random", "one_bin", "steady", "zero_albedo", "camera_unwarp", "discard_direct_light",
                                  "hide_emitters", "beyond_last_bin", "crop", "several", "angular", "hbm"])
def test_gpu_gradients_match_host_build(case):
    """every gradient element within 1e-5 of itself (a floor of 1e-9 of the largest one)"""
    out = run_case(case)
    assert out["scale"] > 0 and out["finite"]
    assert out["rel"] <= 1e-5, out


@pytest.mark.parametrize("case,instantiation", [
    ("ext_ggx", "lds,ext"), ("ext_beckmann", "lds,ext"), ("ext_aniso", "lds,ext"), ("ext_glass", "lds,ext"), ("ext_plastic", "lds,ext"),
    ("ext_textured", "lds,ext"), ("ext_smooth", "lds,ext"), ("hbm_ext", "hbm,ext"), ("rr_12", "lds,plain"), ("rr_inf", "lds,plain"),
    ("hbm_rr", "hbm,plain")])
def test_gpu_gradients_match_host_build_in_every_instantiation(case, instantiation):
    """k_grad_paths<SCENE_LDS, EXT> in its four forms, microfacet / textured / smooth-shaded scenes and Russian roulette: within
    1e-5 of the host build as above, and the case did run the instantiation it names"""
    out = run_case(case)
    print(out)
    assert out["instantiation"] == out["expected"] == instantiation, out
    assert out["scale"] > 0 and out["finite"]
    assert out["rel"] <= 1e-5, out


def test_gpu_grid_stride_loop():
    """more than two trips of k_grad_paths' grid-stride loop, ragged pixel and sample ranges, against the host build"""
    out = run_case("grid_stride", timeout=600)
    print(out)
    assert out["n_lanes"] > 2 * out["grid_cap_lanes"] and out["n_lanes"] % 256 != 0, out
    assert out["instantiation"] == "lds,plain" and out["scale"] > 0
    assert out["rel"] <= 1e-5, out


def test_gpu_emitter_gradients_are_the_oracles_linear_coefficients():
    out = run_case("oracle_emitters")
    print(out)
    assert out["n_emitters"] == 2 and out["nonzero"] and out["instantiation"] == "lds,ext"
    assert out["err"] <= 1.0, out


@pytest.mark.parametrize("case", ["oracle_degree_12", "oracle_degree_inf"])
def test_gpu_albedo_gradients_have_the_degree_of_the_detached_estimator(case):
    out = run_case(case)
    print(out)
    assert out["instantiation"] == "lds,plain"
    assert out["err"] <= 1.0, out
    assert out["control"] > 0.1, out


def test_gpu_autograd_is_render_backward():
    out = run_case("autograd")
    assert out["nonzero"] and out["seed_seen"], out
    assert out["vector_equal"] and out["scalar_equal"], out


def test_gpu_max_depth_one():
    out = run_case("max_depth_1")
    assert out["all_zero_materials"] and out["rel"] <= 1e-5, out


def test_gpu_ranges_and_passes_sum():
    out = run_case("passes")
    assert out["n_passes"] > 1
    assert out["split_rel"] <= 1e-5 and out["multi_rel"] <= 1e-5, out
    assert out["handle_kept"] and out["update_rel"] <= 1e-5, out


def test_gpu_adam_recovers_red_wall():
    out = run_case("adam", timeout=600)
    assert abs(out["final"][0] - 0.570068) <= 0.03, out
