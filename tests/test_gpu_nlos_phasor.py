"""phasor_hdr_film on the NLOS tier, on the GPU: k_fused<NLOS, PHASOR> ((Re, Im) rows in LDS) and k_wf_nlos_bounce's (opl, value)
records -> k_wf_phasor_scatter, through mi.render / integrator.render and the C-ABI, against the CPU oracle.  Every GPU step runs
in a child process under its own time limit (tests/nlos_phasor_gpu_cases.py); each case reports the organisation that ran.

Bound: the project's bound for phasor and NLOS renders, rel-L2 <= 1e-5 on the phasors, the raw film and the steady image, and equal
counters — only the f32 summation order differs from the oracle; these inputs sum at most 32 samples and a handful of terms per pixel,
fewer than tests/test_gpu_phasor.py sums at the same bound.

Shapes: 6 x 5 pixels (30 pixels: a ragged last wave) at 32 spp; F = 15 from f = 0, and F = 151 — 302 floats per row, more than one
pass of 256 threads over a row in the clear and more than four passes of a wave in the flush, an odd 303-float pixel stride."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu
TOL = 1e-5


def run_case(case, timeout=240):
    r = subprocess.run([sys.executable, os.path.join(HERE, "nlos_phasor_gpu_cases.py"), case], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, out)
    return out


def _matches_oracle(o):
    assert o["shapes_ok"] and o["weight_zero"] and o["scale"] > 0 and o["lit"] >= 10, o
    assert o["rel_phasors"] <= TOL and o["rel_raw"] <= TOL and o["rel_steady"] <= TOL, o
    assert o["counters_equal"], o


@pytest.mark.parametrize("F", [15, 151])
@pytest.mark.parametrize("scene", ["confocal_z", "single_quad"])
def test_matches_oracle_in_every_organisation(scene, F):
    """AUTO (through mi.render), fused on request, wavefront on request.  Plain shading, rows that fit LDS: AUTO is the fused kernel
    up to 16 frequencies and the wavefront organisation beyond (mtr_api.hip: resolve_mode, measured)"""
    out = run_case(f"parity:{scene}:{F}")
    auto = "fused" if F <= 16 else "wavefront"
    assert (out["auto"]["ran"], out["fused"]["ran"], out["wavefront"]["ran"]) == (auto, "fused", "wavefront"), out
    for m in ("auto", "fused", "wavefront"):
        _matches_oracle(out[m])


@pytest.mark.parametrize("scene", ["meter_first_last", "camera"])
def test_capture_meter_with_first_and_last_bounces_and_perspective_camera(scene):
    out = run_case(f"parity:{scene}:151:fused,wavefront")
    assert (out["fused"]["ran"], out["wavefront"]["ran"]) == ("fused", "wavefront"), out
    for m in ("fused", "wavefront"):
        _matches_oracle(out[m])


@pytest.mark.parametrize("scene", ["rough_hidden", "textured_hidden"])
def test_extended_shading_is_the_wavefront_organisation(scene):
    """a roughconductor (ggx, alpha 0.3) / a bitmap-textured hidden quad: wavefront under AUTO, refused in the fused mode"""
    out = run_case(f"parity:{scene}:15:auto,fused")
    assert out["auto"]["ran"] == "wavefront", out
    _matches_oracle(out["auto"])
    assert "wavefront" in out["fused"].get("refused", "") and "status -5" in out["fused"]["refused"], out


def test_rows_are_flushed_and_reused():
    """128 x 96 pixels at 2 spp, F = 151 (1208-byte rows).  Fused plan: 48 workgroups (256-pixel shares of 12288 pixels), tickets of
    128 consecutive pixels — at least two per workgroup — over a ring of at most 40 row slots (48 KB / 1208 B): every slot is
    flushed and handed on three times per ticket.  Wavefront plan: 12 segments of 1024 pixels; k_wf_phasor_scatter's grid is at
    most 8 workgroups per compute unit, so each folds several pixels' record lists through its LDS staging buffer."""
    out = run_case("parity:row_reuse:151:fused,wavefront")
    assert (out["fused"]["ran"], out["wavefront"]["ran"]) == ("fused", "wavefront"), out
    for m in ("fused", "wavefront"):
        _matches_oracle(out[m])
        assert out[m]["lit"] > 6000, out


def test_zero_frequency_is_the_steady_image():
    out = run_case("zero_frequency")
    for m in ("fused", "wavefront"):
        assert out[m]["ran"] == m and out[m]["lit"] >= 20, out
        assert out[m]["im_zero"], out
        assert out[m]["rel_re_steady"] <= TOL, out


def test_transient_renders_around_a_phasor_render_are_equal():
    """no LDS plan or frequency table of the phasor render survives into the next render of the context.  The transient renders ask
    for deterministic rows: the fused kernel's fixed-point rows and steady sums are bit-reproducible; the wavefront organisation sums
    its steady image (and any overflowing record) with f32 atomics whatever the flag — summation order, 1e-6"""
    out = run_case("film_types")
    for m in ("fused", "wavefront"):
        assert out[m]["nonzero"] > 0 and out[m]["phasor_nonzero"] > 0, out
    assert out["fused"]["equal_t"] and out["fused"]["equal_s"], out
    assert out["wavefront"]["rel_t"] <= 1e-6 and out["wavefront"]["rel_s"] <= 1e-6, out


def test_c_abi_refusals_leave_the_film_untouched():
    out = run_case("abi_refusals")
    for k in ("exhaustive", "polarized_transient", "polarized_phasor"):
        assert out[k]["status"] == -5 and out[k]["untouched"], out
    assert "Exhaustive" in out["exhaustive"]["message"] and "phasor_hdr_film" in out["exhaustive"]["message"], out
    assert "polarized" in out["polarized_transient"]["message"] and "NLOS" in out["polarized_transient"]["message"], out
    assert "phasor_hdr_film" in out["distributed"], out                   # (DistributedRenderer: single-GPU only, as before)
