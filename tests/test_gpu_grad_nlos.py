"""mtr_render_grad on a NLOS scene on the GPU: k_grad_paths_nlos against the host build of the same arithmetic
(tests/host_grad_nlos.cpp) at the same seed on every CPU case of tests/test_grad_nlos.py — each case naming the instantiation it
ran —, its grid-stride loop, ranges and passes, loss.backward() against render_backward, the kernel against the CPU oracle directly
(laser coefficients, the degree identity with roulette active) and an Adam fit of the hidden Z's albedo through mi.render.  Every
GPU step runs in a child process under its own time limit (tests/grad_nlos_gpu_cases.py)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_grad_nlos as N  # noqa: E402

pytestmark = pytest.mark.gpu


def run_case(case, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(HERE, "grad_nlos_gpu_cases.py"), case], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", list(N.FD_CASES))
def test_gpu_gradients_match_host_build(case):
    """every gradient element — materials and the laser — within 1e-5 of itself (a floor of 1e-9 of the largest one)"""
    out = run_case("host:" + case)
    print(out)
    assert out["instantiation"] == ("nlos,lds,ext" if case == "rough_side" else "nlos,lds,plain"), out
    assert out["scale"] > 0 and out["finite"] and out["laser"]
    assert out["rel"] <= 1e-5, out


def test_gpu_zero_albedo_channel():
    out = run_case("zero_albedo")
    assert out["finite"] and out["rel"] <= 1e-5, out


def test_gpu_grid_stride_loop():
    out = run_case("grid_stride", timeout=600)
    print(out)
    assert out["n_lanes"] > 2 * out["grid_cap_lanes"] and out["n_lanes"] % 256 != 0, out
    assert out["instantiation"] == "nlos,lds,plain" and out["scale"] > 0
    assert out["rel"] <= 1e-5, out


def test_gpu_ranges_and_passes_sum():
    out = run_case("passes")
    assert out["n_passes"] > 1
    assert out["split_rel"] <= 1e-5 and out["multi_rel"] <= 1e-5, out


def test_gpu_autograd_is_render_backward():
    out = run_case("autograd")
    assert out["nonzero"] and out["seed_seen"] and out["vector_equal"], out


@pytest.mark.parametrize("case", ["confocal_ls_hg", "single_hg_wall", "confocal_wall_coin", "rough_side", "camera"])
def test_gpu_laser_gradient_is_the_oracles_linear_coefficient(case):
    out = run_case("oracle_laser:" + case)
    print(out)
    assert out["nonzero"] and out["err"] <= 1.0, out


@pytest.mark.parametrize("max_depth", [12, -1])
@pytest.mark.parametrize("case", list(N.DEGREE_CASES))
def test_gpu_albedo_gradients_have_the_degree_of_the_detached_estimator(case, max_depth):
    out = run_case(f"oracle_degree:{case}:{max_depth}")
    print(out)
    assert out["instantiation"] == "nlos,lds,plain" and out["n_terms"] > 300 and out["deepest"] >= 3
    assert out["err"] <= 1.0, out
    assert out["control"] > 0.1, out


def test_gpu_adam_recovers_the_hidden_albedo():
    """the band is test_grad_nlos.ADAM_BAND, set from the CPU rehearsal (test_adam_rehearsal_on_the_cpu)"""
    out = run_case("adam", timeout=600)
    print(out["final"], out["true"])
    assert all(abs(a - b) <= N.ADAM_BAND for a, b in zip(out["final"], out["true"])), out
