"""k_fused's lean flat-walk kernels fetch a primitive in ONE LDS trip (mtr_core.h: CHILD-ORDERED PRIMITIVE TABLE — the records of the
root's rectangles and of the boxes' faces copied in child order, addressed by the child index / face bit the walk holds in a
register) and hand the surface interaction from shade_hit to shade_finish.  These are the smallest shapes at which a table entry
can be wrong or unused, or the handed-over context read where it was never written: no box (the face region is empty), one and
four boxes (face entries up to 8 + 23, the table's end), one rectangle (misses), child indices 6 and 7, a shadow ray that ends on
a rectangle (the any-hit rectangle pass), a child order that is not the declaration order, a top-level triangle leaf (the kernel
that keeps its loaded references), max_depth = 2 (no shadow ray, no BSDF sample after the first hit), an emitter reached from a
box top.

Every case: about 24 x 20 pixels, 32 bins, 96 spp, max_depth = 6, amd_mode="fused", against the CPU oracle — relative L2 <= 1e-5 on
film and steady image (BASELINE.json north_star), the five counters exact."""
import os

import pytest

from conftest import rel_l2
from test_gpu_parity import gpu_render, oracle_render

pytestmark = pytest.mark.gpu

TOL = 1e-5   # relative L2 (BASELINE.json north_star)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
W, H, BINS, SPP = 24, 20, 32, 96
SHAPES = ("light", "floor", "ceiling", "back", "green-wall", "red-wall", "small-box", "large-box")


def _cornell(**integrator):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=W, height=H, temporal_bins=BINS, start_opl=0.0, bin_width_opl=12.0 / BINS)
    d["integrator"].update(amd_mode="fused", max_depth=6)
    d["integrator"].update(integrator)
    return d


def _rect(at, deg, scale, material):
    """a horizontal rectangle (normal +y before the tilt `deg` about x is added to the floor's -90)"""
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "rectangle", "to_world": T().translate(at).rotate([1, 0, 0], -90.0 + deg).scale(scale), "bsdf": {"type": "ref", "id": material}}


def _cube(at, deg, scale):
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "cube", "to_world": T().translate(at).rotate([0, 1, 0], deg).scale(scale), "bsdf": {"type": "ref", "id": "white"}}


def _scene(case):
    d = _cornell(max_depth=2) if case == "max-depth-2" else _cornell()
    if case == "no-box":                      # rectangle entries only: the face region of the table is empty
        d.pop("small-box"); d.pop("large-box")
    elif case == "one-box":                   # face entries 8 .. 13
        d.pop("small-box")
    elif case == "four-boxes":                # face entries up to 8 + 23, the table's end (4 rectangles + 4 boxes: the root's 8 children)
        d.pop("green-wall"); d.pop("red-wall")
        d["third-box"] = _cube([0.5, 0.3, -0.5], 31.0, [0.15, 0.2, 0.1])
        d["fourth-box"] = _cube([-0.6, -0.8, 0.5], -40.0, 0.18)
    elif case == "one-rectangle":             # the light alone: nearly every ray misses, and a miss hands no context over
        for k in SHAPES[1:]:
            d.pop(k)
    elif case == "seven-rects-one-cube":      # child index 6; the shelf under the light ends shadow rays on a RECTANGLE (the any-hit rectangle pass)
        d.pop("large-box")
        d["shelf"] = _rect([0.0, 0.55, 0.0], 0.0, [0.45, 0.4, 1.0], "green")
    elif case == "eight-rects-no-box":        # child index 7
        d.pop("small-box"); d.pop("large-box")
        d["shelf"] = _rect([0.0, 0.55, 0.0], 0.0, [0.45, 0.4, 1.0], "green")
        d["ramp"] = _rect([-0.4, -0.7, 0.2], 25.0, [0.4, 0.3, 1.0], "red")
    elif case == "shuffled":                  # shapes declared in reverse order, cubes turned: child order (by centroid) is not declaration order
        shapes = {k: d.pop(k) for k in SHAPES}
        shapes["small-box"] = _cube([0.335, -0.7, 0.38], 52.0, 0.3)
        shapes["large-box"] = _cube([-0.33, -0.4, -0.28], -63.0, [0.3, 0.61, 0.3])
        for k in reversed(SHAPES):
            d[k] = shapes[k]
    elif case == "box-top-under-light":       # a tall box right under the light: paths leave its top and hit the emitter (em_plus1 with a handed-over context)
        d["large-box"] = _cube([0.0, -0.25, 0.0], 18.25, [0.3, 0.75, 0.3])
    elif case not in ("cornell", "max-depth-2"):
        raise ValueError(case)
    return d


def _check_against_oracle(oracle, scene, spp, seed):
    s_gpu, t_gpu = gpu_render(scene, spp, seed=seed)
    got = dict(scene.integrator().last_counters)
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, spp, seed=seed)
    print(f"rel-L2 transient {rel_l2(t_gpu, t_ref):.3e} steady {rel_l2(s_gpu, s_ref):.3e} counters {got}")
    assert rel_l2(t_gpu, t_ref) <= TOL and rel_l2(s_gpu, s_ref) <= TOL
    for k in COUNTERS:
        assert got[k] == cnt[k], k
    return got


@pytest.mark.parametrize("case", ["no-box", "one-box", "four-boxes", "one-rectangle", "seven-rects-one-cube", "eight-rects-no-box",
                                  "shuffled", "max-depth-2", "box-top-under-light"])
def test_table_entries(oracle, case):
    """the lean kernels without top-level leaves: every record comes from the table, the surface interaction from shade_hit"""
    import mitransient_amd.mi as mi
    from mitransient_amd import _cabi
    scene = mi.load_dict(_scene(case))
    traits = scene.gpu_traits()
    assert traits & _cabi.MTR_TRAIT_FLAT_TOP and not traits & _cabi.MTR_TRAIT_FLAT_LEAVES
    got = _check_against_oracle(oracle, scene, SPP, seed=13)
    if case == "max-depth-2":                 # no path goes on after its second vertex: shade_finish runs there without a BSDF sample
        assert got["bounces"] <= 2 * got["paths"]


def test_top_level_triangle_leaf(oracle):
    """triangle leaves beside rectangles and a box node at the top level (kTrFlatLeaves): that kernel stages no table and keeps its
    loaded references — a top-level leaf may hold more than one pair (as test_gpu_fused_round_trips.py::test_top_level_triangle_leaves)"""
    import mitransient_amd.mi as mi
    from mitransient_amd import _cabi
    d = _cornell()
    d.pop("small-box")
    tri = os.path.join(ROOT, "tests", "_build", "kite_prim_fetch.obj")
    os.makedirs(os.path.dirname(tri), exist_ok=True)
    with open(tri, "w") as fh:
        fh.write("v 0.2 -0.9 0.6\nv 0.7 -0.9 0.2\nv 0.5 -0.2 0.4\nv 0.1 -0.3 0.1\nf 1 2 3\nf 1 3 4\n")
    d["kite"] = {"type": "obj", "filename": tri, "face_normals": True,
                 "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.4, 0.5, 0.6]}}}}
    scene = mi.load_dict(d)
    assert scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP and scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_LEAVES
    _check_against_oracle(oracle, scene, SPP, seed=13)
