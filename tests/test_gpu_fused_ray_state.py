"""k_fused's flat walk keeps its ray in registers from the first box to the last rectangle (mtr_core.h flat_walk_device takes o, d
and tmax by value; trav_leaf_test / trav_quad_test read them from a RayByValue).  Every place where the ray used to be read back from private memory — in front of
the box loop, behind it, in front of the rectangles' slab tests and in front of the rectangle tests — is crossed here with one, three
and four boxes, with a fourth slab pair, with a triangle leaf at the top level, under the general shading code and by a workgroup
that enters the walks again for a second ticket.  Each render against the CPU oracle: relative L2 <= 1e-5 on film and steady image,
the five counters exact.  The sizes are the smallest that still hold waves whose shadow rays all end on a box (the rectangle stage is
skipped), waves with none that do, and camera rays that leave through the open front."""
import os

import numpy as np
import pytest

from conftest import rel_l2

TOL = 1e-5      # the project's bar (BASELINE.json north_star)
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
W, H, BINS, SPP = 24, 20, 32, 96          # pixels x spp = 46080: no multiple of 256
SEED = 5


def _dict(width=W, height=H, bins=BINS, **film):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=width, height=height, temporal_bins=bins, start_opl=3.5, bin_width_opl=6.0 / bins, **film)
    d["integrator"].update(amd_mode="fused")
    return d


def _cube(at, deg, scale):
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "cube", "to_world": T().translate(at).rotate([0, 1, 0], deg).scale(scale), "bsdf": {"type": "ref", "id": "white"}}


def _load(d):
    import mitransient_amd.mi as mi
    return mi.load_dict(d)


def _gpu(scene, spp, seed):
    import torch
    integ = scene.integrator()
    integ.collect_stats = True
    s, t = integ.render(scene, seed=seed, spp=spp)
    torch.cuda.synchronize()
    return np.array(s), np.array(t)


def _oracle(oracle, scene, spp, seed):
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)
    t4, s4, cnt = oracle.render(sd, p, use_bvh=True)
    t3, s3 = oracle.develop(sd.film, t4, s4)
    return s3, t3, cnt


def _check(oracle, scene, spp=SPP, seed=SEED, flat_leaves=False):
    from mitransient_amd import _cabi
    traits = scene.gpu_traits()
    assert traits & _cabi.MTR_TRAIT_FLAT_TOP, "the scene must take the flat walk"
    assert bool(traits & _cabi.MTR_TRAIT_FLAT_LEAVES) == flat_leaves
    s_gpu, t_gpu = _gpu(scene, spp, seed)
    s_ref, t_ref, cnt = _oracle(oracle, scene, spp, seed)
    assert t_gpu.shape == t_ref.shape and s_gpu.shape == s_ref.shape
    assert np.linalg.norm(t_ref) > 0 and np.linalg.norm(s_ref) > 0
    rt, rs = rel_l2(t_gpu, t_ref), rel_l2(s_gpu, s_ref)
    c = scene.integrator().last_counters
    print(f"film rel-L2 {rt:.3e}, steady rel-L2 {rs:.3e}, counters {[c[k] for k in COUNTERS]} vs oracle {[cnt[k] for k in COUNTERS]}")
    assert rt <= TOL
    assert rs <= TOL
    for k in COUNTERS:
        assert c[k] == cnt[k], (k, c[k], cnt[k])
    return cnt


@pytest.mark.gpu
def test_cornell_box(oracle):
    """two boxes, six rectangles: shadow rays that end on a box and shadow rays that reach the light share waves (fewer
    contributions than shadow rays: some are occluded); rays leave through the open front without a hit"""
    cnt = _check(oracle, _load(_dict()))
    assert 0 < cnt["splats_issued"] < cnt["rays_shadow"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_boxes", [1, 3, 4])
def test_number_of_boxes(oracle, n_boxes):
    """one box: a single trip of the box loop; three; four = kFlatMaxBoxes (the root holds eight children: four rectangles beside
    them, and three boxes leave room for five)"""
    d = _dict()
    if n_boxes == 1:
        d.pop("large-box")
    else:
        d.pop("red-wall")
        d["third-box"] = _cube([0.5, 0.3, -0.5], 31.0, [0.15, 0.2, 0.1])
    if n_boxes == 4:
        d.pop("green-wall")
        d["fourth-box"] = _cube([-0.6, -0.8, 0.5], -40.0, 0.18)
    scene = _load(d)
    assert sum(1 for v in d.values() if isinstance(v, dict) and v.get("type") == "cube") == n_boxes
    _check(oracle, scene)


@pytest.mark.gpu
def test_more_than_six_rectangles(oracle):
    """seven rectangles and one box: the fourth slab pair, whose second half is absent"""
    from mitransient_amd.transform import ScalarTransform4f as T
    d = _dict()
    d.pop("large-box")
    d["shelf"] = {"type": "rectangle", "to_world": T().translate([0.0, 0.1, -0.6]).rotate([1, 0, 0], -70.0).scale([0.5, 0.2, 1.0]),
                  "bsdf": {"type": "ref", "id": "green"}}
    _check(oracle, _load(d))


@pytest.mark.gpu
def test_triangle_leaf_at_the_top_level(oracle, tmp_path):
    """a two-triangle mesh beside rectangles and a box (kTrFlatLeaves): the rectangle stage tests rectangles and a pair leaf"""
    d = _dict()
    d.pop("small-box")
    kite = os.path.join(str(tmp_path), "kite.obj")
    with open(kite, "w") as fh:
        fh.write("v 0.2 -0.9 0.6\nv 0.7 -0.9 0.2\nv 0.5 -0.2 0.4\nv 0.1 -0.3 0.1\nf 1 2 3\nf 1 3 4\n")
    d["kite"] = {"type": "obj", "filename": kite, "face_normals": True,
                 "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.4, 0.5, 0.6]}}}}
    _check(oracle, _load(d), flat_leaves=True)


@pytest.mark.gpu
def test_conductor_box(oracle):
    """the small box a conductor: the flat walk under the general shading code"""
    d = _dict()
    d["mirror"] = {"type": "conductor", "eta": {"type": "rgb", "value": [1.65, 0.88, 0.52]}, "k": {"type": "rgb", "value": [9.2, 6.3, 4.8]}}
    d["small-box"]["bsdf"] = {"type": "ref", "id": "mirror"}
    _check(oracle, _load(d))


@pytest.mark.gpu
def test_second_ticket_with_a_crop_window(oracle):
    """a crop window of 45 x 37 = 1665 pixels off the film's origin at one pixel per ticket: more tickets than the largest grid has
    workgroups (4 on each of 256 CUs), so a workgroup's chunk loop enters both walks again with a fresh ray"""
    from mitransient_amd import _cabi
    lib = _cabi.load_library()
    n_px, spp = 45 * 37, 48
    chunk = lib.mtr_test_fused_chunk(n_px, spp, 1024)
    assert (n_px + chunk - 1) // chunk > 1024
    d = _dict(width=48, height=40, crop_width=45, crop_height=37, crop_offset_x=2, crop_offset_y=1)
    _check(oracle, _load(d), spp=spp)


@pytest.mark.gpu
def test_fixed_point_rows_flat_walk_returns_the_bits_of_the_tree_walk(tmp_path):
    """the fixed-point instantiation shares the walk: with order-independent film rows (amd_deterministic) the Cornell box, which
    takes the flat walk, and the same box with an unreachable triangle behind its back wall, which is walked through its tree, give
    films and steady images that are equal bit for bit, and the same counters"""
    from mitransient_amd import _cabi
    outs, cnts, flat = [], [], []
    for extra in (False, True):
        d = _dict()
        d["integrator"].update(amd_deterministic=True)
        if extra:
            tri = os.path.join(str(tmp_path), "far_triangle.obj")
            with open(tri, "w") as fh:
                fh.write("v -0.1 -0.1 -30\nv 0.1 -0.1 -30\nv 0 0.1 -30\nf 1 2 3\n")
            d["far-triangle"] = {"type": "obj", "filename": tri, "face_normals": True, "bsdf": {"type": "ref", "id": "white"}}
        scene = _load(d)
        outs.append(_gpu(scene, SPP, SEED)); cnts.append(dict(scene.integrator().last_counters))
        flat.append(bool(scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP))
    assert flat == [True, False]
    assert np.linalg.norm(outs[0][1]) > 0
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    for k in COUNTERS:
        assert cnts[0][k] == cnts[1][k], k
