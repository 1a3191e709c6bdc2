"""The *_mono_polarized variants on the MI355X: k_wf_polar_bounce + k_wf_polar_scatter against the CPU oracle's f64 polarized
path (oracle/mtr_oracle.c) and the host build of the same arithmetic (tests/host_polarized.cpp over mtr_polar.h) at identical
(seed, lane) — per polarized lobe and at the wavefront path's edges: crop windows and ragged films, the depth / roulette
matrix, camera_unwarp and discard_direct_light, the three seedings, sample chunks, one sample per pixel, record-list overflow,
rows too long for LDS, a workspace reallocated between renders, a scene in HBM, sample and pixel shards; the mode rules;
values outside the fixed-point range through the Stokes scatter; the reference notebook's cells
(cornell-box/cbox_polarized.xml, `Au` substituted as in tests/test_polarized.py)."""
import math

import numpy as np
import pytest

from conftest import rel_l2
from test_polarized import (BSDF_KINDS, GOLD_ETA, GOLD_K, assert_matches_oracle, bsdf_scene, build_host_polarized, figure,
                            hp_render, load_cbox_polarized, oracle_render, sign_agreement)

pytestmark = pytest.mark.gpu
TOL = 1e-5          # the bar of every GPU / CPU parity test here: the GPU adds a pixel's samples in another order
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
FIG_SIGNS, FIG_NCC, FIG_NCC_4 = 0.98, 0.93, 0.96       # the reference figures at the notebook's 4096 spp; measured 0.990 / 0.997,
                                                        # NCC 0.9445 per pixel, 0.9727 over 4 x 4 blocks


@pytest.fixture(scope="module")
def hp():
    import ctypes as C
    return C.CDLL(build_host_polarized())


def _gpu(scene, spp, seed=0, mode="wavefront"):
    import torch
    integ = scene.integrator()
    integ.amd_mode = mode
    integ.collect_stats = True
    s, t = integ.render(scene, seed=seed, spp=spp)
    torch.cuda.synchronize()
    return np.array(s), np.array(t), dict(integ.last_counters)


def _host(hp, scene, spp, seed=0):
    t4, s4, cnt = hp_render(hp, scene, seed=seed, spp=spp)
    with np.errstate(invalid="ignore", divide="ignore"):
        steady = np.where(s4[..., 3:] > 0, s4[..., :1] / s4[..., 3:], 0.0).astype(np.float32)
    return steady, t4, cnt


@pytest.mark.parametrize("res,spp,seed", [(16, 16, 0), (24, 8, 3)])
def test_gpu_matches_the_host_build(hp, res, spp, seed):
    scene = load_cbox_polarized(res=res)
    s, t, c = _gpu(scene, spp, seed)
    hs, ht, hc = _host(hp, scene, spp, seed)
    assert t.shape == (res, res, 400, 4) and s.shape == (res, res, 1)
    assert rel_l2(t, ht) <= TOL and rel_l2(s, hs) <= TOL
    for k in range(4):                          # every Stokes channel on its own (S1..S3 are much smaller than S0)
        assert rel_l2(t[..., k], ht[..., k]) <= 1e-4, k
    assert np.abs(t[..., 1:]).max() > 0
    for k in COUNTERS:
        assert c[k] == hc[k], k
    assert_matches_oracle(t, s, c, oracle_render(scene, seed=seed, spp=spp))


def test_gpu_diffuse_box_is_the_unpolarized_render():
    import os
    import mitransient_amd.mi as mi
    from test_polarized import CBOX
    path = os.path.join(CBOX, "cbox_diffuse.xml")
    mi.set_variant("llvm_ad_mono")
    su, tu, cu = _gpu(mi.load_file(path, res=32, spp=16), 16, 2)
    mi.set_variant("llvm_ad_mono_polarized")
    sp, tp, cp = _gpu(mi.load_file(path, res=32, spp=16), 16, 2)
    assert rel_l2(tp[..., 0], tu[..., 0]) <= TOL and rel_l2(sp, su) <= TOL
    assert not np.any(tp[..., 1:])
    for k in COUNTERS:
        assert cp[k] == cu[k], k


def test_modes():
    scene = load_cbox_polarized(res=8)
    integ = scene.integrator()
    integ.amd_mode = "auto"
    s, t = integ.render(scene, spp=4)
    assert np.array(t).shape == (8, 8, 400, 4)
    assert integ.resolved_mode(scene, scene.sensors()[0], 4) == "wavefront"        # (mtr_render_plan, the film prepared)
    integ.amd_mode = "fused"
    with pytest.raises(Exception, match="wavefront"):
        integ.render(scene, spp=4)
    # deterministic rows do not exist for the Stokes film: refused, not ignored — by the integrator and by the C-ABI
    import ctypes as C
    import torch
    import mitransient_amd.mi as mi
    from mitransient_amd import _cabi
    integ.amd_mode = "wavefront"
    integ.deterministic = True
    with pytest.raises(ValueError, match="amd_deterministic"):
        mi.render(scene, spp=4)
    integ.deterministic = False
    p = integ.render_params(scene.sensors()[0].film(), 0, 4)
    p.flags |= _cabi.MTR_FLAG_DETERMINISTIC
    t4 = torch.zeros((8, 8, 400, 4), dtype=torch.float32, device="cuda")
    s4 = torch.zeros((8, 8, 4), dtype=torch.float32, device="cuda")
    lib = _cabi.load_library()
    ctx, sc = C.c_void_p(), C.c_void_p()
    assert lib.mtr_ctx_create(torch.cuda.current_device(), C.byref(ctx)) == 0
    try:
        d = scene.data().desc()
        assert lib.mtr_scene_create(ctx, C.byref(d), C.byref(sc)) == 0
        try:
            r = lib.mtr_render(sc, C.byref(p), C.c_void_p(t4.data_ptr()), C.c_void_p(s4.data_ptr()), None, None)
            assert r == -5, r                    # MTR_ERR_UNSUPPORTED
            assert b"MTR_FLAG_DETERMINISTIC" in lib.mtr_last_error(ctx)
        finally:
            lib.mtr_scene_destroy(sc)
    finally:
        torch.cuda.synchronize()
        lib.mtr_ctx_destroy(ctx)
    assert not t4.any()


def test_steady_is_the_sum_of_the_transient_s0():
    """a time window that covers every path: steady == transient.sum(2)[..., :1] (as tests/test_gpu_parity.py for rgb)"""
    import mitransient_amd.mi as mi
    from test_polarized import cbox_polarized_dict, CBOX
    mi.set_variant("llvm_ad_mono_polarized")
    d = cbox_polarized_dict(res=16)
    d["sensor"]["film"].update(start_opl=0.0, bin_width_opl=40.0, temporal_bins=400)     # 0 .. 16000: every path of max_depth 5
    scene = mi.load_dict(d, base_dir=CBOX)
    s, t, _ = _gpu(scene, 32, 1)
    assert rel_l2(s, t.sum(axis=2)[..., :1]) <= TOL


def _lit_floor(radiance):
    """a diffuse floor lit by a small rectangle light beside the camera's view (paths of 4 .. 7.5 in an 8-bin window)"""
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant("llvm_ad_mono_polarized")
    return mi.load_dict({
        "type": "scene",
        "integrator": {"type": "transient_path", "max_depth": 3},
        "sensor": {"type": "perspective", "fov": 40, "to_world": T().look_at([0, 0, 4], [0, 0, 0], [0, 1, 0]),
                   "film": {"type": "transient_hdr_film", "width": 8, "height": 8, "temporal_bins": 8, "start_opl": 0,
                            "bin_width_opl": 1, "rfilter": {"type": "box"}}},
        "floor": {"type": "rectangle", "bsdf": {"type": "diffuse", "reflectance": 0.5}},
        "light": {"type": "rectangle", "to_world": T().translate([1.5, 0, 2]).rotate([1, 0, 0], 180).scale(0.5),
                  "emitter": {"type": "area", "radiance": radiance}},
    })


@pytest.mark.parametrize("radiance", [1e7, math.inf, -math.inf, math.nan])
def test_values_outside_the_fixed_point_range_pass_through(hp, radiance):
    scene = _lit_floor(radiance)
    s, t, _ = _gpu(scene, 8, 0)
    hs, ht, _ = _host(hp, scene, 8, 0)
    for a, b in ((t, ht), (s, hs)):
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_array_equal(np.isposinf(a), np.isposinf(b))
        np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b))
        fin = np.isfinite(b)
        assert rel_l2(a[fin], b[fin]) <= TOL
    assert not np.all(np.isfinite(t)) or abs(radiance) == 1e7
    if radiance == 1e7:
        assert np.abs(ht).max() > 1e5


def test_notebook_cells():
    """render_cbox_polarized_and_visualization{,_steady}.ipynb as written apart from the `Au` substitution"""
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    scene = load_cbox_polarized()
    data_steady, data_transient = mi.render(scene, spp=4096)
    assert data_steady.shape == (256, 256, 1) and data_transient.shape == (256, 256, 400, 4)
    mi.util.convert_to_bitmap(data_steady)
    data_transient_np = np.array(data_transient)
    dop = mitr.vis.degree_of_polarization(data_transient_np)
    dop, aolp, aolp_scaled, top, chirality = mitr.vis.polarization_generate_false_color(data_transient_np)
    assert aolp.shape == (256, 256, 400, 3)
    data_steady_np = data_transient_np.sum(axis=2, keepdims=True)
    dop, aolp, aolp_scaled, top, chirality = mitr.vis.polarization_generate_false_color(data_steady_np)
    # the gold boxes polarize what they reflect; the diffuse walls do not
    assert np.all(np.isfinite(data_transient_np))
    assert np.abs(data_steady_np[..., 1:3]).max() > 1e-3 * data_steady_np[..., 0].max()
    st = np.array(data_steady)
    assert st.mean() > 0 and data_steady_np[..., 0].mean() > 0.5 * st.mean()
    # the reference's figures (tests/golden/polarized_figures.npz): the steady one pins the signs of S1 and S2 (the raw steady
    # accumulator holds S0, S1, S2 and the weight), the transient bin 120 is compared as displayed, by NCC
    acc = scene.sensors()[0].film().steady_accum().cpu().numpy().astype(np.float64)
    (a1, a2), (n1, n2) = sign_agreement(acc[..., :3] / np.maximum(acc[..., 3:], 1.0), figure("steady"))
    _, aolp120, *_ = mitr.vis.polarization_generate_false_color(data_transient_np[:, :, 120, :])
    shown = np.clip(aolp120, 0.0, 1.0)                       # matplotlib clips a float RGB image to [0, 1]
    fig = figure("transient_bin120") / 255.0
    n_px, n_4 = ncc(shown, fig), ncc(blocks(shown), blocks(fig))
    print(f"figures: steady sign agreement S1 {a1:.4f} S2 {a2:.4f} ({n1} / {n2} px), bin 120 NCC {n_px:.4f}, 4x4 blocks {n_4:.4f}")
    assert a1 >= FIG_SIGNS and a2 >= FIG_SIGNS
    assert n_px >= FIG_NCC and n_4 >= FIG_NCC_4


def ncc(a, b):
    a = a - a.mean(); b = b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def blocks(a, k=4):
    H, W, C = a.shape
    return a.reshape(H // k, k, W // k, k, C).mean(axis=(1, 3))


# ---------------------------------------------------------------- against the oracle's f64 polarized path
def _vs_oracle(scene, spp, seed=0, **kw):
    s, t, c = _gpu(scene, spp, seed)
    assert_matches_oracle(t, s, c, oracle_render(scene, seed=seed, spp=spp), **kw)
    return s, t, c


GOLD = {"type": "conductor", "eta": GOLD_ETA, "k": GOLD_K}


@pytest.mark.parametrize("kind", BSDF_KINDS)
def test_gpu_matches_the_oracle_per_bsdf(kind):
    _vs_oracle(bsdf_scene(kind), 32, 1)


def test_gpu_ragged_film_with_crop_window():
    """13 x 7 film, 5 spp, a crop window with offsets: pixel -> crop mapping in polar_begin, load_state and the steady write"""
    scene = bsdf_scene("glass", film={"width": 13, "height": 7, "crop_width": 9, "crop_height": 5, "crop_offset_x": 3,
                                      "crop_offset_y": 1, "temporal_bins": 37})
    s, t, _ = _vs_oracle(scene, 5, 4)
    assert t.shape == (7, 13, 37, 4) and s.shape == (5, 9, 1)
    assert np.all(t[5:] == 0) and np.all(t[:, 9:] == 0)          # only the crop_size corner is written


@pytest.mark.parametrize("max_depth,rr_depth", [(0, 5), (1, 5), (2, 5), (3, 1), (12, 2), (-1, 3)])
def test_gpu_depths_on_a_conductor_and_dielectric_scene(max_depth, rr_depth):
    """the first-bounce special case, roulette on a Mueller M00, the live-count polling loop of max_depth -1"""
    _vs_oracle(bsdf_scene("glass", max_depth=max_depth, rr_depth=rr_depth, back_bsdf=GOLD), 16, 2)


@pytest.mark.parametrize("flag", ["camera_unwarp", "discard_direct_light"])
def test_gpu_unwarp_and_discard_direct(flag):
    _vs_oracle(bsdf_scene("roughconductor_ggx", back_bsdf=GOLD, **{flag: True}), 16, 5)


@pytest.mark.parametrize("seeding", [{}, {"amd_pcg_initseq_plus_lane": True}, {"amd_pcg_tea64": True}],
                         ids=["tea", "tea+lane", "tea64"])
def test_gpu_seedings(seeding):
    """k_wf_polar_bounce recomputes the sampler's stream from rc.flags on every reloaded path"""
    _vs_oracle(bsdf_scene("glass", back_bsdf=GOLD, max_depth=10, **seeding), 16, 6)


def test_gpu_sample_chunks():
    """2 x 2 pixels at 4100 spp: two sample chunks (4096, then 4), two pixels per segment"""
    _vs_oracle(bsdf_scene("conductor", res=2), 4100, 7)


def test_gpu_one_sample_per_pixel():
    """128 x 96 at 1 spp: segments cut by pixel count (1024 per segment)"""
    _vs_oracle(bsdf_scene("roughconductor_beckmann_aniso", film={"width": 128, "height": 96}), 1, 8)


def test_gpu_record_overflow():
    """a closed box with a glass cube and a gold wall, paths of ~9 contributions: the per-pixel record lists (4 contributions per
    path) overflow into the film's atomics, S3 included"""
    scene = bsdf_scene("glass", res=8, closed=True, back_bsdf=GOLD, max_depth=-1, rr_depth=40,
                       film={"start_opl": 0.0, "bin_width_opl": 400.0 / 64})
    s, t, c = _vs_oracle(scene, 8, 9)
    assert c["splats_overflow"] > 0
    assert np.abs(t[..., 3]).max() > 0


@pytest.mark.parametrize("bins", [9600, 9601])
def test_gpu_rows_at_the_lds_limit(bins):
    """9600 bins: the last count whose Stokes rows fit LDS; 9601: no record lists, every contribution a film atomic"""
    _vs_oracle(bsdf_scene("glass", res=6, back_bsdf=GOLD, film={"temporal_bins": bins, "bin_width_opl": 16.0 / bins}), 8, 10)


def test_gpu_workspace_follows_the_bin_count():
    """one scene rendered with 400 -> 9601 -> 400 bins: the workspace is reallocated when the record capacity changes"""
    import mitransient_amd.mi as mi
    scene = bsdf_scene("glass", res=8, back_bsdf=GOLD, film={"temporal_bins": 400, "bin_width_opl": 0.04})
    for bins in (400, 9601, 400):
        params = mi.traverse(scene)
        params["sensor.film.temporal_bins"] = bins
        params["sensor.film.bin_width_opl"] = 16.0 / bins
        params.update()
        s, t, _ = _vs_oracle(scene, 8, 11)
        assert t.shape == (8, 8, bins, 4)


def test_gpu_staircase_in_hbm():
    """staircase_like(tiles=6) polarized: k_wf_polar_bounce with the scene in HBM, cubes, a thin glass pane, twosided brass"""
    import mitransient_amd.mi as mi
    from mitransient_amd.scenes import staircase_like
    mi.set_variant("llvm_ad_mono_polarized")
    scene = mi.load_dict(staircase_like(n_steps=12, balusters=2, tiles=6, width=24, height=24, temporal_bins=64, spp=8))
    _vs_oracle(scene, 8, 12)


def test_gpu_sample_and_pixel_shards():
    """sample shards and pixel shards accumulated through integ.accumulate sum to the whole render; each shard is the oracle's"""
    import torch
    scene = bsdf_scene("glass", res=16, back_bsdf=GOLD)
    spp = 12
    s_full, t_full, _ = _gpu(scene, spp, 13)
    integ = scene.integrator()
    sens = scene.sensors()[0]
    film = sens.film()
    for kw in ({"spp_range": (0, 5)}, {"spp_range": (5, 12)}, {"pixel_range": (0, 100)}, {"pixel_range": (100, 256)}):
        passes = integ.prepare(scene, sens, 13, spp, [])
        integ.accumulate(scene, sens, passes, spp, **kw)
        torch.cuda.synchronize()
        t1 = np.array(film.develop()[1])
        p = {"spp_begin": kw["spp_range"][0], "spp_end": kw["spp_range"][1]} if "spp_range" in kw else \
            {"pixel_begin": kw["pixel_range"][0], "pixel_end": kw["pixel_range"][1]}
        ot = oracle_render(scene, seed=13, spp=spp, **p)[0]
        assert rel_l2(t1, ot) <= TOL, kw
    passes = integ.prepare(scene, sens, 13, spp, [])
    for rng in ((0, 5), (5, 12)):
        integ.accumulate(scene, sens, passes, spp, spp_range=rng)
    s_a, t_a = film.develop()
    passes = integ.prepare(scene, sens, 13, spp, [])
    for rng in ((0, 100), (100, 256)):
        integ.accumulate(scene, sens, passes, spp, pixel_range=rng)
    s_b, t_b = film.develop()
    for s_, t_ in ((s_a, t_a), (s_b, t_b)):
        assert rel_l2(np.array(t_), t_full) <= 1e-6 and rel_l2(np.array(s_), s_full) <= 1e-6
