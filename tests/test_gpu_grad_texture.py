"""mtr_render_grad_tex on the GPU: both tiers of the texel gradients against the host build of the same arithmetic
(tests/host_grad_tex.cpp) at the same seed — each case naming the instantiation of k_grad_paths and the tier it ran —, the
grid-stride loop with texels on, mtr_render_grad unchanged on a textured scene, loss.backward() on a ``.data`` tensor against
render_backward, and an Adam fit of a pattern on a wall.  Every GPU step runs in a child process under its own time limit
(tests/grad_tex_gpu_cases.py)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


def run_case(case, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(HERE, "grad_tex_gpu_cases.py"), case], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,instantiation,tier", [
    ("slab_lds", "lds,ext", "slab"), ("slab_hbm", "hbm,ext", "slab"),
    ("global_wall", "lds,ext", "global"), ("global_staircase", "hbm,ext", "global")])
def test_gpu_texel_gradients_match_host_build(case, instantiation, tier):
    """every texel gradient within 1e-5 of the texture's largest element (test_gpu_grad.py's bound), every other gradient within
    1e-5 of itself as there; the case ran the kernel form and the tier it names.  slab: the 8 x 4 bitmap; global_wall: 256 x 256
    texels on two Cornell walls; global_staircase: 64 x 64 on the staircase stand-in's diffuse BSDF"""
    out = run_case(case)
    print(out)
    assert out["expected"] == [instantiation, tier] and out["instantiation"] == instantiation and out["tier"] == tier, out
    # (2048 lanes of at most 3 textured vertices and 4 taps cannot reach most of 65 536 texels: the texels the host build leaves at
    # 0 must be exactly those the kernel leaves at 0)
    assert out["finite"] and out["device_ok"] and out["texel_scale"] > 0 and out["texels_nonzero"] > 0 and out["same_support"], out
    assert out["rel_texels"] <= 1e-5, out
    assert out["rel_other"] <= 1e-5, out


def test_gpu_grid_stride_loop_with_texels():
    """more than two trips of k_grad_paths' grid-stride loop, ragged pixel and sample ranges, in both tiers"""
    out = run_case("grid_stride", timeout=900)
    print(out)
    for tier in ("slab", "global"):
        o = out[tier]
        assert o["tier"] == tier and o["n_lanes"] > 2 * o["grid_cap_lanes"] and o["n_lanes"] % 256 != 0, out
        assert o["rel_texels"] <= 1e-5 and o["rel_other"] <= 1e-5, out


def test_gpu_render_grad_is_unchanged_on_a_textured_scene():
    out = run_case("unchanged")
    print(out)
    assert out["n_textured"] == 2 and out["textured_zero"] and out["texels_written"], out
    assert out["same_as_tex"] and out["null_is_plain"], out
    assert out["rel_host"] <= 1e-5, out


def test_gpu_autograd_on_texels_is_render_backward_slab_tier():
    out = run_case("autograd_slab")
    print(out)
    assert out["tier"] == "slab" and out["shape_ok"] and out["seed_seen"] and out["nonzero"] > 0, out
    assert out["equal"] and out["constant_equal"], out                 # bit for bit


def test_gpu_autograd_on_texels_is_render_backward_global_tier():
    out = run_case("autograd_global")
    print(out)
    assert out["tier"] == "global" and out["shape_ok"] and out["seed_seen"] and out["nonzero"] > 0, out
    assert out["rel"] <= 1e-6 and out["constant_equal"], out           # arrival order of the atomics


# measured once at grad_tex_gpu_cases.ADAM's settings on the MI355X: the loss fell from 1.312e-6 to 7.95e-9, a factor of 165.08
# (mean absolute texel error 0.283 -> 0.089); the assertion is set at half of that
ADAM_FACTOR_MEASURED = 165.08


def test_gpu_adam_recovers_a_pattern_on_a_wall():
    out = run_case("adam", timeout=900)
    print(out)
    assert out["factor"] >= ADAM_FACTOR_MEASURED / 2, out
    assert out["texel_err_last"] < out["texel_err_first"], out
