"""What classify_scene (mtr_scene_host.cpp) decides about a scene, on the CPU.  The specialised kernels LACK the shading code a
trait rules out, so a wrong bit is a wrong picture.  EXPECTED holds, per scene of scene_class_cases.py, the words the library
reported on an MI355X (mtr_scene_traits; the extended shading code and the polarized form through what mtr_render_plan
refuses) before the classification moved out of mtr_scene_create — the NLOS tier refuses polarized transport before it looks
at the materials, so the polarized form of the four NLOS scenes follows from reading that rule: diffuse materials, no bitmap,
no emitter.  test_gpu_scene_class.py checks that the library still reports these words."""
import pytest

import scene_class_cases as cases
from scene_class_cases import host_class

DIFFUSE, ONE_RECT_EMITTER, LEAF_PAIR, FLAT_TOP, FLAT_LEAVES, NO_LOBES, GREY = 1, 2, 4, 8, 16, 32, 64

# name: (trait word, needs the extended shading code, has a polarized form, the organisation MTR_MODE_AUTO picks)
EXPECTED = {
    "cornell-config1": (15, 0, 1, "fused"),              # kTrCornellFlat and nothing else
    "cornell-config2": (15, 0, 1, "fused"),
    "cornell-config3": (15, 0, 1, "fused"),
    "nlos-z-config4": (120, 1, 1, "fused"),              # (an `obj` with vertex normals: the extended code without lobes)
    "nlos-grey-quad": (77, 0, 1, "fused"),
    "nlos-coloured-laser": (13, 0, 1, "fused"),
    "nlos-coloured-hidden": (13, 0, 1, "fused"),
    "staircase-config5": (2, 0, 1, "wavefront"),
    "staircase-rough": (0, 1, 0, "wavefront"),
    "staircase-rough-normals": (0, 1, 0, "wavefront"),
    "staircase-rough-normals-textures": (0, 1, 0, "wavefront"),
    "mirror-box": (14, 0, 1, "fused"),
    "cornell-angulararea": (13, 0, 0, "fused"),
    "cornell-two-emitters": (5, 0, 1, "fused"),
    "cornell-mesh-boxes": (7, 0, 1, "wavefront"),
    "top-level-triangles": (30, 0, 1, "fused"),
    "far-triangle": (7, 0, 1, "fused"),
    "five-cubes": (7, 0, 1, "wavefront"),
    "rough-ggx": (8, 1, 0, "fused"),
    "rough-beckmann-by-default": (8, 1, 0, "fused"),
    "rough-anisotropic": (8, 1, 0, "fused"),
    "rough-roughdielectric": (8, 1, 0, "fused"),
    "rough-plastic-thindielectric": (8, 1, 0, "fused"),
    "textured-diffuse": (56, 1, 0, "fused"),
    "textured-roughplastic": (24, 1, 0, "fused"),
    "grey-cornell": (79, 0, 1, "fused"),
    "grey-cornell-one-wall-coloured": (15, 0, 1, "fused"),
}


def test_every_case_is_pinned():
    assert set(EXPECTED) == set(cases.CASES)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_scene_class_is_the_recorded_one(host_harness, tmp_path, name):
    traits, ext, polar, flat = host_class(host_harness, cases.CASES[name](tmp_path))
    assert (traits, ext, polar) == EXPECTED[name][:3]
    # kTrFlatTop never without a tree of at most two levels, and with it the top level's description (otherwise all zero)
    n_quads, n_boxes, node0, prim_mask, wide_levels = flat
    if traits & FLAT_TOP:
        assert wide_levels <= 2 and node0 == 1 and n_boxes <= 4 and prim_mask != 0
        assert prim_mask & ((1 << n_quads) - 1) == (1 << n_quads) - 1
        assert bool(traits & FLAT_LEAVES) == bool(prim_mask >> n_quads)
    else:
        assert flat[:4] == [0, 0, 0, 0] and not traits & FLAT_LEAVES


def test_flat_top_levels_of_the_cornell_box(host_harness, tmp_path):
    """six rectangles (the light among them) and two box nodes under one root; with its boxes as meshes a third level and no flat top"""
    assert host_class(host_harness, cases.CASES["cornell-config1"](tmp_path))[3] == [6, 2, 1, 0x3f, 2]
    flat = host_class(host_harness, cases.CASES["cornell-mesh-boxes"](tmp_path))[3]
    assert flat[:4] == [0, 0, 0, 0] and flat[4] > 2


def test_no_flat_knob_clears_the_flat_top_only(host_harness, tmp_path, monkeypatch):
    """MTR_NO_FLAT (live in the harness and the experiments build): the tree walk instead, every other trait as it was"""
    scene = cases.CASES["top-level-triangles"](tmp_path)
    monkeypatch.setenv("MTR_NO_FLAT", "1")
    traits, ext, polar, flat = host_class(host_harness, scene)
    assert traits == EXPECTED["top-level-triangles"][0] & ~(FLAT_TOP | FLAT_LEAVES) and flat[:4] == [0, 0, 0, 0]


# one unequal channel anywhere clears kTrGrey: material a, b, c, c2 — except the slots where an anisotropic lobe keeps its second
# roughness (roughdielectric: b[0]; roughconductor: c2[0]) — and an emitter's radiance
@pytest.mark.parametrize("field", ["a", "b", "c", "c2", "radiance"])
def test_grey_is_cleared_by_one_unequal_channel(host_harness, tmp_path, field):
    scene = cases.grey_cornell(tmp_path)
    sd = scene.data()
    assert host_class(host_harness, scene)[0] == EXPECTED["grey-cornell"][0]
    for channel in range(3):
        arr = sd.emitters[0].radiance if field == "radiance" else getattr(sd.materials[1], field)
        saved = arr[channel]
        arr[channel] = saved + 0.125
        assert host_class(host_harness, scene)[0] == EXPECTED["grey-cornell"][0] & ~GREY, (field, channel)
        arr[channel] = saved
    assert host_class(host_harness, scene)[0] & GREY


@pytest.mark.parametrize("bsdf,field", [("roughdielectric", "b"), ("roughconductor", "c2")])
def test_grey_anisotropic_exceptions(host_harness, tmp_path, bsdf, field):
    """the second roughness of an anisotropic lobe is no colour: grey stays; the same slot of the isotropic lobe clears it"""
    from mitransient_amd import _cabi
    import mitransient_amd.mi as mi
    for aniso in (True, False):
        d = cases.grey_cornell_dict()
        lobe = {"type": bsdf, "distribution": "ggx"}
        lobe.update({"alpha_u": 0.1, "alpha_v": 0.3} if aniso else {"alpha": 0.1})
        lobe.update({"int_ior": 1.5, "ext_ior": 1.0} if bsdf == "roughdielectric" else {"eta": 0.2, "k": 3.9})
        d["small-box"]["bsdf"] = lobe
        scene = mi.load_dict(d)
        sd = scene.data()
        m = next(sd.materials[i] for i in range(sd.n_materials) if sd.materials[i].type in (_cabi.MTR_BSDF_ROUGHDIELECTRIC, _cabi.MTR_BSDF_ROUGHCONDUCTOR))
        assert bool(m.flags & _cabi.MTR_MAT_ANISOTROPIC) == aniso
        assert host_class(host_harness, scene)[0] & GREY
        getattr(m, field)[0] += 0.125
        assert bool(host_class(host_harness, scene)[0] & GREY) == aniso
        if aniso:       # ... and the lobe's other colour slot still counts
            other = m.c2 if field == "b" else m.b
            other[1] += 0.125
            assert not host_class(host_harness, scene)[0] & GREY
