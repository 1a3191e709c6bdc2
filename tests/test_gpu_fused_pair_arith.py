"""k_fused's pair arithmetic: two triangles of a leaf, or two children of a node, are evaluated side by side with the f2 helpers of
mtr_core.h, which a translation unit lowers either to packed instructions on register pairs or to two plain f32 instructions each
(MTR_PAIR_SCALAR).  Either form must give each half what a single evaluation gives, whatever sits in the other half.  One case per
family of sites: the flat walk's slab pairs with an absent child beside a present one and with its fourth pair, the pair leaf test
with a pad half and with rays on the diagonal that both halves share, the node test of the LDS tree walk, the NLOS instantiation.
Each render against the CPU oracle: relative L2 <= 1e-5 on film and steady image, the five counters exact; and the contributions of
a flat-walk and of a tree-walk scene bit for bit.  These tests guard arithmetic, not speed: they hold for either form."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import make_nlos, rel_l2

TOL = 1e-5      # the project's bar (BASELINE.json north_star)
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
W, H, BINS, SPP = 24, 20, 32, 96          # pixels x spp = 46080: no multiple of 256
SEED = 7


def _dict(width=W, height=H, bins=BINS):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=width, height=height, temporal_bins=bins, start_opl=3.5, bin_width_opl=6.0 / bins)
    d["integrator"].update(amd_mode="fused")
    return d


def _load(d):
    import mitransient_amd.mi as mi
    return mi.load_dict(d)


def _rect(at, axis, deg, scale, material):
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "rectangle", "to_world": T().translate(at).rotate(axis, deg).scale(scale), "bsdf": {"type": "ref", "id": material}}


def _cube(at, deg, scale):
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "cube", "to_world": T().translate(at).rotate([0, 1, 0], deg).scale(scale), "bsdf": {"type": "ref", "id": "white"}}


def _obj(tmp_path, name, text, rgb=(0.4, 0.5, 0.6)):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as fh:
        fh.write(text)
    return {"type": "obj", "filename": path, "face_normals": True,
            "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": list(rgb)}}}}


# eight triangles around (0.3, -0.45, 0.3): a mesh that is no cube and has more than two triangles, so its subtree is neither a box
# node nor one leaf and no scene that holds it has a flat top level
OCTAHEDRON = ("v 0.55 -0.45 0.3\nv 0.05 -0.45 0.3\nv 0.3 -0.15 0.3\nv 0.3 -0.75 0.3\nv 0.3 -0.45 0.55\nv 0.3 -0.45 0.05\n"
              "f 1 3 5\nf 3 2 5\nf 2 4 5\nf 4 1 5\nf 3 1 6\nf 2 3 6\nf 4 2 6\nf 1 4 6\n")


def _tree_walk_dict(tmp_path):
    d = _dict()
    d.pop("small-box")
    d["octahedron"] = _obj(tmp_path, "octahedron.obj", OCTAHEDRON)
    return d


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


def _check(oracle, scene, spp=SPP, seed=SEED, flat=True, flat_leaves=False):
    from mitransient_amd import _cabi
    traits = scene.gpu_traits()
    assert bool(traits & _cabi.MTR_TRAIT_FLAT_TOP) == flat
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
@pytest.mark.parametrize("n_rect", [5, 7])
def test_flat_slab_pair_with_one_present_child(oracle, n_rect):
    """five rectangles (the red wall taken out) and seven (a shelf put in, one box taken out to leave room at the top level): the
    last slab pair holds one rectangle and, in its other half, an absent child with an inverted box — whose entry distances are
    computed all the same and must neither report a hit nor disturb the half beside it"""
    d = _dict()
    if n_rect == 5:
        d.pop("red-wall")
    else:
        d.pop("large-box")
        d["shelf"] = _rect([0.0, 0.1, -0.6], [1, 0, 0], -70.0, [0.5, 0.2, 1.0], "green")
    assert sum(1 for v in d.values() if isinstance(v, dict) and v.get("type") == "rectangle") == n_rect
    _check(oracle, _load(d))


@pytest.mark.gpu
def test_flat_slab_pairs_fourth_pair(oracle):
    """eight children at the top level, all of them rectangles: the fourth slab pair runs with both of its halves present"""
    d = _dict()
    d.pop("large-box"); d.pop("small-box")
    d["shelf"] = _rect([0.0, 0.1, -0.6], [1, 0, 0], -70.0, [0.5, 0.2, 1.0], "green")
    d["ramp"] = _rect([-0.4, -0.5, 0.3], [1, 0, 0], -60.0, [0.3, 0.25, 1.0], "red")
    assert sum(1 for v in d.values() if isinstance(v, dict) and v.get("type") == "rectangle") == 8
    _check(oracle, _load(d))


@pytest.mark.gpu
def test_pair_leaf_with_a_pad_half(oracle, tmp_path):
    """a one-triangle mesh at the top level (kTrFlatLeaves): the second half of its pair is a pad, which repeats the triangle and
    must never report a hit — a hit there would count twice or win the tie with another original index"""
    d = _dict()
    d.pop("small-box")
    d["sail"] = _obj(tmp_path, "sail.obj", "v 0.1 -0.9 0.6\nv 0.75 -0.85 0.2\nv 0.45 -0.1 0.35\nf 1 2 3\n")
    _check(oracle, _load(d), flat_leaves=True)


@pytest.mark.gpu
def test_pair_leaf_on_face_diagonals(oracle):
    """both boxes square to the camera: their front faces are seen face-on, the pixel grid is symmetric about the optical axis and
    rays cross the diagonal that the two triangles of a face share — both halves of the pair evaluate that edge, and the tie
    between them goes to the original index as in the oracle"""
    d = _dict()
    d["small-box"] = _cube([0.0, -0.7, 0.4], 0.0, 0.3)
    d["large-box"] = _cube([0.0, 0.3, -0.4], 0.0, [0.45, 0.25, 0.3])
    _check(oracle, _load(d))


@pytest.mark.gpu
def test_node_pairs_under_the_lds_tree_walk(oracle, tmp_path):
    """an octahedron in place of the small box: the scene takes no flat walk and the fused mode walks its wide tree from LDS —
    wide_node_test's pairs of children at two levels, the octahedron's pair leaves under them"""
    _check(oracle, _load(_tree_walk_dict(tmp_path)), flat=False)


@pytest.mark.gpu
def test_nlos_confocal(oracle):
    """k_fused<NLOS>: a confocal capture of the 'Z' of three flat boxes (pair leaves under a tree) behind an 8 x 6 relay wall"""
    scene = make_nlos(sx=8, sy=6, capture="confocal", hidden="z", bins=BINS, bin_width=0.06)
    scene.integrator().mode = 1            # MTR_MODE_FUSED
    s_gpu, t_gpu = _gpu(scene, 64, 0)
    s_ref, t_ref, cnt = _oracle(oracle, scene, 64, 0)
    assert np.linalg.norm(t_ref) > 0 and np.linalg.norm(s_ref) > 0
    rt, rs = rel_l2(t_gpu, t_ref), rel_l2(s_gpu, s_ref)
    c = scene.integrator().last_counters
    print(f"film rel-L2 {rt:.3e}, steady rel-L2 {rs:.3e}, counters {[c[k] for k in COUNTERS]} vs oracle {[cnt[k] for k in COUNTERS]}")
    assert rt <= TOL
    assert rs <= TOL
    for k in COUNTERS:
        assert c[k] == cnt[k], (k, c[k], cnt[k])


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["flat", "tree"])
def test_contributions_bit_for_bit(oracle, tmp_path, walk):
    """the splat log of the flat Cornell box and of the tree-walk scene against the oracle's: the same (lane, depth, kind, pixel,
    bin) multiset and the same values bit for bit — what tests/test_gpu_parity.py::test_splat_log_matches_oracle asks of the default
    scene, here of both walks under the fused mode"""
    import torch
    from mitransient_amd import _cabi
    from mitransient_amd.runtime import get_context
    spp = 4
    d = _dict(width=16, height=16, bins=64) if walk == "flat" else None
    if d is None:
        d = _tree_walk_dict(tmp_path)
        d["sensor"]["film"].update(width=16, height=16, temporal_bins=64, bin_width_opl=6.0 / 64)
    scene = _load(d)
    assert bool(scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP) == (walk == "flat")
    integ, sensor = scene.integrator(), scene.sensors()[0]
    passes = integ.prepare(scene, sensor, 0, spp, [])
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    cap = 1 << 16
    log = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.check(ctx.lib.mtr_debug_set_splat_log(h, C.c_void_p(log.data_ptr()), cap, C.c_void_p(n.data_ptr())))
    integ.accumulate(scene, sensor, passes, spp)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.mtr_debug_set_splat_log(h, None, 0, None))
    n_gpu = int(n.item())
    rec = log[:n_gpu].cpu().numpy().view(np.uint32)
    _, _, cnt, olog = oracle.render(scene.data(), integ.render_params(sensor.film(), 0, spp), use_bvh=False, log_capacity=cap)
    assert 0 < n_gpu <= cap
    assert n_gpu == len(olog) == cnt["splats_issued"]
    g = np.zeros(n_gpu, dtype=olog.dtype)
    g["lane"], g["depth_kind"], g["pixel"], g["bin"] = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    g["r"], g["g"], g["b"], g["opl"] = (rec[:, 4].view(np.float32), rec[:, 5].view(np.float32),
                                       rec[:, 6].view(np.float32), rec[:, 7].view(np.float32))
    g.sort(order=["lane", "depth_kind"])
    olog.sort(order=["lane", "depth_kind"])
    for k in olog.dtype.names:
        assert np.array_equal(g[k].view(np.uint32), olog[k].view(np.uint32)), k
