"""k_fused's shadow walk skips the rectangle tests a shadow ray provably cannot pass (mtr_core.h flat_walk_device: SHADOW HULL;
mtr_shadow_hull.h holds the proof, test_shadow_hull.py sweeps it on the CPU).  Per wave one of three tiers runs: the rectangle stage
as it always was (some lane's origin is within the guard distance of a wall's plane), the light's slab pair and test alone for the
lanes within the guard distance of the light's plane, or no rectangle stage.  Each must return what the full stage returns, bit for
bit.  Scenes: shadow_hull_cases.py; amd_mode="fused", against the CPU oracle — relative L2 <= 1e-5 on film and steady image, the five
counters exact — and, with order-independent rows (amd_deterministic: the fixed-point instantiation, which reads the same block),
films compared bit for bit between renders that take different tiers:

  * amd_shadow_hull_margin 128: every origin on a wall is hull-risky (test_shadow_hull.py asserts it), so every wave with a live lane
    on a wall runs the unchanged stage; 1: the light's tier in about half the waves, no stage in the others; 0: the block is empty;
  * a twin scene whose only difference is a rectangle no ray can reach, behind the back wall: that scene is no hull room.

Whether a scene is one is asserted through scene.gpu_shadow_hull() (mtr_scene_shadow_hull), not through a trait bit: the trait word
selects kernels and is pinned, value for value, by test_scene_class.py and test_gpu_scene_class.py."""
import ctypes as C

import numpy as np
import pytest

import shadow_hull_cases as cases
from conftest import rel_l2
from test_gpu_parity import gpu_render, oracle_render

pytestmark = pytest.mark.gpu

TOL = 1e-5   # relative L2 (BASELINE.json north_star)
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")


def _load(d):
    import mitransient_amd.mi as mi
    return mi.load_dict(d)


def _check_against_oracle(oracle, scene, spp, seed):
    s_gpu, t_gpu = gpu_render(scene, spp, seed=seed)
    got = dict(scene.integrator().last_counters)
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, spp, seed=seed)
    print("rel L2 film %.3e steady %.3e" % (rel_l2(t_gpu, t_ref), rel_l2(s_gpu, s_ref)), got)
    assert rel_l2(t_gpu, t_ref) <= TOL and rel_l2(s_gpu, s_ref) <= TOL
    for k in COUNTERS:
        assert got[k] == cnt[k], k
    assert got["rays_shadow"] > 0
    return s_gpu, t_gpu


def test_splat_log_and_counters_match_the_oracle(oracle):
    """the Cornell box, 32 x 24 pixels, 64 bins, 64 spp: the same (lane, depth, kind, pixel, bin) multiset as the oracle's, the same
    values bit for bit — an occluded contribution let through, or a visible one dropped, is a record too many or too few —, the five
    counters, the film to 1e-5"""
    import torch
    from mitransient_amd.runtime import get_context
    scene = _load(cases.cornell())
    assert scene.gpu_shadow_hull() == 5
    integ, sens = scene.integrator(), scene.sensors()[0]
    integ.collect_stats = True
    film = sens.film()
    passes = integ.prepare(scene, sens, 3, 64, [])
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    cap = 1 << 19
    log = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.check(ctx.lib.mtr_debug_set_splat_log(h, C.c_void_p(log.data_ptr()), cap, C.c_void_p(n.data_ptr())))
    integ.accumulate(scene, sens, passes, 64)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.mtr_debug_set_splat_log(h, None, 0, None))
    got = dict(integ.last_counters)
    s, t = (np.array(x) for x in film.develop())
    n_gpu = int(n.item())
    rec = log[:n_gpu].cpu().numpy().view(np.uint32)
    params = integ.render_params(film, 3, 64, 0, 64, 0, None)
    _, _, cnt, olog = oracle.render(scene.data(), params, use_bvh=False, log_capacity=cap)
    assert 0 < n_gpu == len(olog) == cnt["splats_issued"] < cap
    for k in COUNTERS:
        assert got[k] == cnt[k], k
    g = np.zeros(n_gpu, dtype=olog.dtype)
    g["lane"], g["depth_kind"], g["pixel"], g["bin"] = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    g["r"], g["g"], g["b"], g["opl"] = (rec[:, 4].view(np.float32), rec[:, 5].view(np.float32),
                                       rec[:, 6].view(np.float32), rec[:, 7].view(np.float32))
    order = ["lane", "depth_kind"]
    g.sort(order=order)
    olog.sort(order=order)
    for k in olog.dtype.names:
        assert np.array_equal(g[k].view(np.uint32), olog[k].view(np.uint32)), k
    s_ref, t_ref, s4, t4, cnt2 = oracle_render(oracle, scene, 64, seed=3)
    assert rel_l2(t, t_ref) <= TOL and rel_l2(s, s_ref) <= TOL


def _deterministic(d, spp=64, seed=7):
    scene = _load(d)
    s, t = gpu_render(scene, spp, seed=seed)
    return scene, s, t, dict(scene.integrator().last_counters)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_twin_scene_with_an_unreachable_rectangle(oracle):
    """40 x 40 pixels, 128 bins, 64 spp, deterministic rows.  The Cornell box without its small box (seven children under the root) and
    the same with a rectangle behind the back wall (eight: still a flat top level, the fourth slab pair in use).  No ray reaches that
    rectangle, but it lies behind the back wall's plane: the twin is no hull room and runs the full stage in every wave.  Films and
    counters are equal bit for bit — the device of test_flat_top_level_returns_the_bits_of_the_tree_walk"""
    from mitransient_amd import _cabi
    from mitransient_amd.transform import ScalarTransform4f as T
    film = dict(width=40, height=40, temporal_bins=128, start_opl=3.5, bin_width_opl=6.0 / 128)
    out = []
    for twin in (False, True):
        d = cases.cornell(film=film, amd_deterministic=True)
        d.pop("small-box")
        if twin:
            d["far-rectangle"] = {"type": "rectangle", "to_world": T().translate([0.0, 0.0, -30.0]).scale([0.1, 0.1, 0.1]), "bsdf": {"type": "ref", "id": "white"}}
        scene, s, t, cnt = _deterministic(d)
        assert scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP
        assert scene.gpu_shadow_hull() == (0 if twin else 5)
        out.append((s, t, cnt))
    assert _same_bits(out[0][1], out[1][1]) and _same_bits(out[0][0], out[1][0])
    for k in COUNTERS:
        assert out[0][2][k] == out[1][2][k], k
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, 64, seed=7)
    assert rel_l2(out[0][1], t_ref) <= TOL and out[0][2]["rays_shadow"] == cnt["rays_shadow"]


def test_margins_give_the_same_bits():
    """the Cornell box, 40 x 40 pixels, 128 bins, 64 spp, deterministic rows, with amd_shadow_hull_margin 1, 128 and 0: the three tiers
    in their usual shares, the unchanged stage in every wave, the parent's path — three films equal bit for bit"""
    film = dict(width=40, height=40, temporal_bins=128, start_opl=3.5, bin_width_opl=6.0 / 128)
    out = [_deterministic(cases.cornell(film=film, amd_deterministic=True, amd_shadow_hull_margin=m)) for m in (1, 128, 0)]
    assert all(o[0].gpu_shadow_hull() == 5 for o in out)          # (the scene's property: the margin is the render's)
    for o in out[1:]:
        assert _same_bits(out[0][2], o[2]) and _same_bits(out[0][1], o[1])
        for k in COUNTERS:
            assert out[0][3][k] == o[3][k], k


def test_margins_give_the_same_bits_in_the_lean_kernel():
    """the same three margins through the f32-row kernel (config 2's): its rows are summed in arrival order, so the films agree to
    1e-5 only — but the counters, which hold every shadow ray's verdict (a contribution more or fewer), are equal"""
    film = dict(width=40, height=40, temporal_bins=128, start_opl=3.5, bin_width_opl=6.0 / 128)
    out = [_deterministic(cases.cornell(film=film, amd_shadow_hull_margin=m)) for m in (1, 128, 0)]
    for o in out[1:]:
        assert rel_l2(o[2], out[0][2]) <= TOL
        for k in COUNTERS:
            assert out[0][3][k] == o[3][k], k


@pytest.mark.parametrize("name", list(cases.OFF))
def test_rooms_that_are_off(oracle, name):
    scene = _load(cases.OFF[name]())
    assert scene.gpu_shadow_hull() == 0
    _check_against_oracle(oracle, scene, 32, seed=5)


@pytest.mark.parametrize("name", [k for k in cases.ON if k != "cornell"])
def test_rooms_that_are_on(oracle, name):
    """times 100 and 0.01: the guard distances scale with the room; the light on the red wall: another row, another slab pair for the
    light's tier; seven rectangles and a cube: the fourth slab pair; a film cropped to the light: origins on E itself, never E-safe"""
    scene = _load(cases.ON[name]())
    assert scene.gpu_shadow_hull() == cases.HULL_RECTANGLES[name]
    _check_against_oracle(oracle, scene, 64 if name == "looking-at-the-light" else 32, seed=5)
