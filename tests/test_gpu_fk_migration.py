"""nlos.fk_migration on the GPU: each kernel of csrc/mtr_fk.hip against the host build of the same text (tests/host_fk.cpp) bit
for bit at the shapes where it takes another path, the whole call against the f64 reference of tests/fk_cases.py on the CPU
tests' cases, determinism, and a render migrated where it lies.  Every GPU step runs in a child process under its own time limit
(tests/fk_gpu_cases.py); the steps several tests read run once."""
import functools
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fk_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run_case(case, timeout=180):
    r = subprocess.run([sys.executable, os.path.join(HERE, "fk_gpu_cases.py"), case], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("shape", ["ragged", "long", "unstaged", "q3", "range"])
def test_gpu_kernels_match_the_host_build_bit_for_bit(shape):
    """6 x 10 x 50 with ragged shifts of both signs; T' = 1200 (more than four trips of a workgroup along a row); T' = 9000 on a
    2 x 2 scan (a row longer than what k_fk_stolt stages in LDS); q = 3 with a ragged last group; kept depth rows that start
    and end mid-tile on a scan wider than one tile"""
    out = run_case("kernels:" + shape)
    print(out)
    assert out["staged"] == (shape != "unstaged") and (shape != "long" or out["trips"] > 4)
    assert out["finite"] and out["stolt_nonzero"] > 0
    assert out["prepare"] and out["stolt"] and out["finish"], out


@pytest.mark.parametrize("name", ["points", "quad", "z"])
def test_gpu_call_against_the_f64_reference(name):
    """The bar on V is the project's 1e-5 while the device FFT itself, measured against np.fft in f64 on the same padded input,
    is within 2.5e-6; four times that measurement otherwise.  Measured: DESIGN.md section 2, f-k migration."""
    out = run_case("e2e:" + name)
    print(out)
    bar = 1e-5 if out["fft_rel"] <= 2.5e-6 else 4.0 * out["fft_rel"]
    assert out["device"] and out["shape"][0] == out["depths"] and out["shape"][1:] == ([32, 32] if name == "points" else [16, 16])
    assert out["rel"] <= bar, (out["rel"], bar)
    assert out["range_rows"]


@pytest.mark.parametrize("name", ["points", "quad"])
def test_gpu_two_calls_give_equal_bits(name):
    assert run_case("e2e:" + name)["same_bits"]


def test_gpu_point_scatterers_are_where_they_were_put():
    assert run_case("e2e:points")["peaks"] == [[100, 12, 20], [60, 24, 9]]


def test_gpu_render_migrated_where_it_lies_focuses_at_its_depth():
    """mi.render of the 16 x 16 quad scene, the tensor handed to fk_migration as it is: the brightest depth within a sample of z = 1"""
    out = run_case("e2e:quad")
    assert abs(out["brightest"] - K.Z1_SAMPLE) <= 1.0 and out["share"] >= 0.85, out
