"""mtr_render_grad on the GPU: the kernel's gradients against the host build of the same arithmetic (tests/host_grad.cpp) at the
same seed on every CPU case of tests/test_grad.py, a scene walked in HBM, renders split into ranges and passes, and an Adam
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
