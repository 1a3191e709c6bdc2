"""k_fused's lean kernels request what a section reads as ONE group (mtr_core.h: BATCHED REQUESTS): film and render constants after
either walk, the six plane pairs of a slab step.  (Round 10 also tried the path start's arguments in front of the s_owner read and the
flat top level's header with box 0's rows: HISTORY.md.)  These are the smallest shapes at which a batched request can go wrong: a
header whose box rows are unused (no box) or partly used, slab pairs with a masked half, a start section that runs with nobody
waiting, film and flag words that matter (crop offset, camera_unwarp, discard_direct_light), LoopArgs that matter (spp_begin != 0, a
ragged last ticket).

Every case: about 24 x 20 pixels, 32 bins, 96 spp, amd_mode="fused", against the CPU oracle — relative L2 <= 1e-5 on film and steady
image, the five counters exact.  The flat top levels are also compared bit for bit with the tree walk under amd_deterministic, in the
manner of test_gpu_parity.py::test_flat_top_level_returns_the_bits_of_the_tree_walk (fixed-point kernels: not the lean ones)."""
import os

import numpy as np
import pytest

from conftest import rel_l2
from test_gpu_parity import gpu_render, oracle_render

pytestmark = pytest.mark.gpu

TOL = 1e-5   # relative L2 (BASELINE.json north_star)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
W, H, BINS, SPP = 24, 20, 32, 96


def _cornell(width=W, height=H, film=None, **integrator):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=width, height=height, temporal_bins=BINS, start_opl=0.0, bin_width_opl=12.0 / BINS)
    d["sensor"]["film"].update(film or {})
    d["integrator"].update(amd_mode="fused", max_depth=6)
    d["integrator"].update(integrator)
    return d


def _check_against_oracle(oracle, scene, spp, seed):
    s_gpu, t_gpu = gpu_render(scene, spp, seed=seed)
    got = dict(scene.integrator().last_counters)
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, spp, seed=seed)
    assert rel_l2(t_gpu, t_ref) <= TOL and rel_l2(s_gpu, s_ref) <= TOL
    for k in COUNTERS:
        assert got[k] == cnt[k], k
    return s_gpu, t_gpu, got


def _flat_scene(case, d):
    from mitransient_amd.transform import ScalarTransform4f as T
    white = {"type": "ref", "id": "white"}

    def cube(at, deg, scale):
        return {"type": "cube", "to_world": T().translate(at).rotate([0, 1, 0], deg).scale(scale), "bsdf": white}
    if case == "no-box":                      # rectangles only: the box loop does not run, the slab stage is the whole walk
        d.pop("small-box"); d.pop("large-box")
    elif case == "one-box":
        d.pop("small-box")
    elif case == "four-boxes":                # the most boxes a flat top level takes (under 4 rectangles: the root holds 8 children)
        d.pop("green-wall"); d.pop("red-wall")
        d["third-box"] = cube([0.5, 0.3, -0.5], 31.0, [0.15, 0.2, 0.1])
        d["fourth-box"] = cube([-0.6, -0.8, 0.5], -40.0, 0.18)
    elif case == "one-rectangle":             # the light alone: the second half of slab pair 0 and pairs 1, 2 are masked
        for k in ("floor", "ceiling", "back", "green-wall", "red-wall", "small-box", "large-box"):
            d.pop(k)
    elif case == "seven-rects-one-cube":      # the fourth slab pair, its second half masked
        d.pop("large-box")
        d["shelf"] = {"type": "rectangle", "to_world": T().translate([0.0, 0.1, -0.6]).rotate([1, 0, 0], -70.0).scale([0.5, 0.2, 1.0]),
                      "bsdf": {"type": "ref", "id": "green"}}
    else:
        raise ValueError(case)
    return d


@pytest.mark.parametrize("case", ["no-box", "one-box", "four-boxes", "one-rectangle", "seven-rects-one-cube"])
def test_flat_top_levels(oracle, case):
    """flat_walk_device with its slab reads six at a time: every count of boxes and rectangles at which a part of a group is unused
    or masked.  The comparison with the oracle (f32 rows, exact counters) is what covers the changed code: it runs the lean kernel.
    The second half — bit for bit against the tree walk, which the same scene takes with five unreachable boxes more (one box too
    many for a flat top level) — needs order-independent rows, and amd_deterministic selects the fixed-point kernels, which are not
    lean and read their slabs as before: it pins the flat walk those kernels share with the lean ones, not the batched reads."""
    import mitransient_amd.mi as mi
    from mitransient_amd import _cabi
    scene = mi.load_dict(_flat_scene(case, _cornell()))
    assert scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP
    _check_against_oracle(oracle, scene, SPP, seed=11)
    from mitransient_amd.transform import ScalarTransform4f as T
    outs, cnts, flat = [], [], []
    for extra in (False, True):
        d = _flat_scene(case, _cornell(amd_deterministic=True))
        if extra:          # five more boxes than a flat top level takes, high above the ceiling and the downward-facing light, outside the camera's frustum
            for i in range(5):
                d[f"far-box-{i}"] = {"type": "cube", "to_world": T().translate([-2.0 + i, 30.0, 0.0]).scale(0.05), "bsdf": {"type": "ref", "id": "white"}}
        sc = mi.load_dict(d)
        s, t = gpu_render(sc, SPP, seed=11)
        outs.append((s, t)); cnts.append(dict(sc.integrator().last_counters))
        flat.append(bool(sc.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP))
    assert flat == [True, False]
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    for k in COUNTERS:
        assert cnts[0][k] == cnts[1][k], k


def test_top_level_triangle_leaves(oracle):
    """triangle leaves beside rectangles and a box node at the top level (kTrFlatLeaves, general shading): the slab pairs are masked
    by FlatHdr::prim_mask, and a leaf of triangle pairs is tested where a rectangle would be"""
    import mitransient_amd.mi as mi
    from mitransient_amd import _cabi
    d = _cornell()
    d.pop("small-box")
    tri = os.path.join(ROOT, "tests", "_build", "kite.obj")
    os.makedirs(os.path.dirname(tri), exist_ok=True)
    with open(tri, "w") as fh:
        fh.write("v 0.2 -0.9 0.6\nv 0.7 -0.9 0.2\nv 0.5 -0.2 0.4\nv 0.1 -0.3 0.1\nf 1 2 3\nf 1 3 4\n")
    d["kite"] = {"type": "obj", "filename": tri, "face_normals": True,
                 "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.4, 0.5, 0.6]}}}}
    scene = mi.load_dict(d)
    assert scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP and scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_LEAVES
    _check_against_oracle(oracle, scene, SPP, seed=11)


def test_start_section_with_nobody_waiting(oracle):
    """fewer lanes than a workgroup (6 x 5 pixels x 8 spp = 240 < 256): some lanes never wait, the start section runs with
    nobody waiting and the wave drains from its first iteration"""
    import mitransient_amd.mi as mi
    scene = mi.load_dict(_cornell(width=6, height=5))
    _check_against_oracle(oracle, scene, 8, seed=3)


@pytest.mark.parametrize("flag", ["camera_unwarp", "discard_direct_light"])
def test_crop_window_with_offset(oracle, flag):
    """a crop window with a non-zero offset: crop_w, crop_x, crop_y place the path at its start; width, height and the flag words of
    the group `refresh` fetches after either walk decide what reaches the film"""
    import mitransient_amd.mi as mi
    crop = dict(width=40, height=24, crop_width=17, crop_height=9, crop_offset_x=5, crop_offset_y=3)
    scene = mi.load_dict(_cornell(film=crop, **{flag: True}))
    s_gpu, t_gpu, _ = _check_against_oracle(oracle, scene, SPP, seed=5)
    assert t_gpu.shape == (24, 40, BINS, 3)
    assert np.all(t_gpu[9:] == 0) and np.all(t_gpu[:, 17:] == 0)


def test_passes_and_a_ragged_last_ticket(oracle):
    """a render split into passes (spp_begin != 0: the start section's LoopArgs) over 23 x 19 = 437 pixels, a count no ticket size
    but 19 and 23 divides: the passes add up to the oracle's whole render, film and counters"""
    import torch
    import mitransient_amd.mi as mi
    scene = mi.load_dict(_cornell(width=23, height=19))
    integ, sens = scene.integrator(), scene.sensors()[0]
    integ.collect_stats = True
    passes = integ.prepare(scene, sens, 9, SPP, [])
    total = {k: 0 for k in COUNTERS}
    for rng in [(0, 31), (31, 32), (32, SPP)]:
        integ.accumulate(scene, sens, passes, SPP, spp_range=rng)
        for k in COUNTERS:
            total[k] += integ.last_counters[k]
    s, t = sens.film().develop()
    torch.cuda.synchronize()
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, SPP, seed=9)
    assert rel_l2(np.array(t), t_ref) <= TOL and rel_l2(np.array(s), s_ref) <= TOL
    for k in COUNTERS:
        assert total[k] == cnt[k], k
