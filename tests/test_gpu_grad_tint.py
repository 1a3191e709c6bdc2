"""mtr_render_grad_tint / mtr_render_fwd_tint on the GPU: the kernels of mtr_tint.hip against the host build of the same arithmetic
(tests/host_tint.cpp) at the same seed in every instantiation, the ragged grid-stride launch, the forward tiers, the device-side
duality, autograd through mi.render and params.update().  Every step runs in a child process of its own with a time limit
(tests/tint_gpu_cases.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(*args, limit=120):
    out = subprocess.run([sys.executable, os.path.join(HERE, "tint_gpu_cases.py"), *args], capture_output=True, text=True, timeout=limit)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"\n[tint gpu] {' '.join(args)}: {r}")
    return r


@pytest.mark.parametrize("name,inst", [("smooth", "lds,plain"), ("ggx", "lds,ext"), ("beckmann", "lds,ext"), ("pane", "lds,ext"),
                                       ("hbm_plain", "hbm,plain"), ("hbm_ext", "hbm,ext")])
def test_kernels_against_the_host_build(name, inst):
    r = run_case("kernels", name)
    assert r["instantiation"] == inst
    assert r["tint_scale"] > 0 and r["fwd_scale"] > 0
    assert r["rev"] <= 1e-5, r
    assert r["fwd_s"] <= 1e-5 and r["fwd_t"] <= 1e-5, r
    assert r["dual"] <= 1e-5, r
    assert r["null_pointer_same"], r


def test_ragged_grid_stride_launch():
    r = run_case("grid_stride")
    assert r["n_lanes"] > r["grid_cap_lanes"] and r["n_runs"] > r["run_cap"], r          # both grids take more than one trip
    assert r["parts"] <= 1e-5 and r["host"] <= 1e-5 and r["fwd_host"] <= 1e-5, r
    assert r["range_rows"] <= 1e-5 and r["others_at_sentinel"] and r["whole_written"], r


@pytest.mark.parametrize("which,tier", [("rows_8", "rows"), ("rows_300", "rows"), ("global", "global")])
def test_forward_tiers(which, tier):
    r = run_case("fwd_tier", which)
    assert r["tier"] == tier and r["scale"] > 0
    assert r["fwd_s"] <= 1e-5 and r["fwd_t"] <= 1e-5, r


def test_autograd_through_mi_render():
    r = run_case("autograd")
    assert r["backward_equal"] and r["forward_equal"], r


def test_params_update_of_a_tint_on_the_device():
    r = run_case("update")
    assert r["equal"] and r["changed"], r


def test_adam_fits_a_mirrors_tint_from_a_transient_target():
    """the band is test_grad_tint.py's CPU rehearsal (oracle primal, host-build gradients: worst channel 0.0073 after 60 steps, mean
    loss per 20 steps 0.49, 0.053, 0.0043) with a factor of two"""
    from test_grad_tint import ADAM_BAND
    r = run_case("adam", limit=180)
    err = [abs(a - b) for a, b in zip(r["final"], r["true"])]
    assert r["losses_thirds"][0] > r["losses_thirds"][1] > r["losses_thirds"][2], r
    assert max(err) <= ADAM_BAND, (r, err)
