"""The scenes, ray families and forms of the walker tests: tests/test_walk_cases.py (CPU: the host build's walks against the oracle's
brute force and an f64 reference, and that every family reaches the edge it names) and tests/test_gpu_walk.py with its child
tests/walk_gpu_cases.py (MI355X: every device walker — mitransient_amd/csrc/mtr_walk_kat.hip — against the host twin hh_walk, ray by
ray).  Everything is seeded numpy; nothing is read from a file.

Every ray is finite: a unit direction, a finite origin, tmax 0, finite or +inf (check_finite).  A walker that did not terminate on
anything else would hang a GPU, and the renderer builds no such ray."""
import ctypes as C
import functools
import tempfile
import zlib

import numpy as np

# form -> the hook's number (mtr_walk_kat.hip: WalkForm)
FORMS = {"wide_lds": 0, "wide_lds_multi": 1, "q8_hbm": 2, "q4_hbm": 3, "flat_refs": 4, "flat_leaves": 5, "flat_table": 6,
         "flat_table_shadow": 7, "flat_table_hull": 8}
SHADOW_FORMS = ("flat_table_shadow", "flat_table_hull")
SUFFIXES = ("", "_k")                      # the Makefile's two flag sets: as the wavefront files see mtr_core.h, as k_fused sees it
# the host tree a device form is compared with (hh_set_node_pairs, hh_set_wide); test_walk_cases.py shows that all five agree
HOST_TREES = {"bvh2-selects": (0, 0), "bvh2-offsets": (1, 0), "wide": (1, 1), "quantised-4": (0, 2), "quantised-8": (0, 3)}
TWIN = {"wide_lds": "wide", "wide_lds_multi": "wide", "q8_hbm": "quantised-8", "q4_hbm": "quantised-4", "flat_refs": "wide",
        "flat_leaves": "wide", "flat_table": "wide", "flat_table_shadow": "wide", "flat_table_hull": "wide"}
# the hook's refusals (mtr_walk_kat.hip)
ERR_EMPTY, ERR_FORM, ERR_TRAITS, ERR_NOT_FLAT, ERR_LDS, ERR_HULL = -2, -3, -4, -5, -6, -7

K_EDGE_EPS = 2.0 ** -19                    # mtr_core.h kEdgeEps
BAND = 2.0 * K_EDGE_EPS                    # the f64 reference's edge band
MIN_COS = 0.05
# The oracle's f32 brute force against the f64 reference (tests/walk_reference.py) on the interior, non-grazing rays of every `random`
# family, as test_walk_cases.py measures it: the largest relative error of t and the largest absolute error of (u, v) seen, and the
# bounds the test asserts — twice the measurement, the margin tests/kat_cases.py uses
# (per scene: Moller-Trumbore's error grows with the triangles' aspect ratio — the sticks are 1 : 100 slivers).  scene: (largest relative
# error of t measured, its bound, largest absolute error of (u, v) measured, its bound)
TOLS = {
    "cornell": (9.65e-06, 1.93e-05, 6.7e-07, 1.34e-06),
    "cornell-panel": (5.98e-05, 0.00012, 5.28e-07, 1.06e-06),
    "top-level-triangles": (1.36e-05, 2.72e-05, 6.46e-07, 1.29e-06),
    "relay-room": (5.74e-06, 1.15e-05, 6.32e-07, 1.26e-06),
    "spheres": (1.66e-05, 3.32e-05, 0, 0),
    "mesh-boxes": (4.26e-06, 8.52e-06, 2.16e-06, 4.32e-06),
    "loose-triangle": (6.53e-05, 0.000131, 8.45e-07, 1.69e-06),
    "sticks": (0.00334, 0.00668, 1.32e-05, 2.64e-05),
    "sticks-small": (8.74e-05, 0.000175, 3.55e-05, 7.1e-05),
}
MAX_EXCLUDED = 0.02                        # share of `random` rays that may lie in the edge band or graze


class Rays:
    """one family on one scene.  o, d (n, 3) f32 and tmax (n) f32 — or, for `shadow`, sp, gn and (u1, u2) (n, 2);
    target: (n, k) f64 what each ray was aimed at, for the failure message; edges: {name: count} the edge cases counted from the inputs"""

    def __init__(self, family, o, d, tmax, target=None, edges=None, variants=None):
        self.family, self.o, self.d, self.tmax = family, np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(tmax, np.float32)
        self.target, self.edges, self.variants = target, edges or {}, variants
        self.n = len(self.o)
        assert self.o.shape == (self.n, 3) and self.d.shape == (self.n, 3)


def check_finite(r):
    assert np.all(np.isfinite(r.o)) and np.all(np.isfinite(r.d)), r.family
    ln = np.linalg.norm(r.d.astype(np.float64), axis=1)
    assert np.all(np.abs(ln - 1.0) < 1e-6), (r.family, float(np.abs(ln - 1.0).max()))
    if r.family == "shadow":
        assert r.tmax.shape == (r.n, 2) and np.all((r.tmax >= 0.0) & (r.tmax <= 1.0))
    else:
        assert r.tmax.shape == (r.n,) and not np.any(np.isnan(r.tmax)) and np.all(r.tmax >= 0.0)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)


def _f32_unit(v):
    return _unit(_unit(v).astype(np.float32).astype(np.float64)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- scenes
def _mi():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    return mi


def _cornell():
    import mitransient_amd as mitr
    _mi()
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=16, height=16, temporal_bins=16, start_opl=3.5, bin_width_opl=6.0 / 16)
    return d


_TMP = None


def _tmp():
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="walk_cases_")
    return _TMP.name


def _obj(name, tris):
    import os
    path = os.path.join(_tmp(), name)
    with open(path, "w") as fh:
        for i, t in enumerate(np.asarray(tris, np.float64).reshape(-1, 3, 3)):
            for p in t:
                fh.write("v %.9g %.9g %.9g\n" % tuple(p))
            fh.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    return path


ROTATED = lambda T: T().translate([0.3, -0.2, 0.1]).rotate([1, 2, 3], 37.0).scale([0.3, 0.6, 0.2])      # noqa: E731
SHEARED_FAR = np.array([[80.0, 25.0, 0.0, 350.0], [-10.0, 160.0, 30.0, 165.0], [5.0, -20.0, 90.0, 270.0], [0, 0, 0, 1.0]])
QUAD = np.array([[-1, -1, 0, 1, -1, 0, 1, 1, 0], [-1, -1, 0, 1, 1, 0, -1, 1, 0]], np.float64).reshape(2, 3, 3)


def _relay_copy():
    c, s_ = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    return rot


def _raw(tris):
    """triangles alone, no shape table: the degenerate scenes of test_bvh_degenerate_inputs"""
    from mitransient_amd.scene import SceneData
    base = scene("cornell")
    sd = SceneData()
    sd.tri_verts = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    n = sd.tri_verts.shape[0]
    sd.tri_material = np.zeros(n, np.uint32)
    sd.tri_emitter = np.full(n, -1, np.int32)
    sd.materials, sd.n_materials = base.materials, 1
    sd.camera, sd.film = base.camera, base.film
    return sd


def _build(name):
    mi = _mi()
    T = mi.ScalarTransform4f
    if name == "cornell":
        return mi.load_dict(_cornell()).data()
    if name in ("cornell-rotated", "cornell-sheared"):
        d = _cornell()
        d["small-box"]["to_world"] = ROTATED(T) if name == "cornell-rotated" else T(SHEARED_FAR)
        return mi.load_dict(d).data()
    if name == "cornell-twin-wall":            # two walls twice: coincident rectangles, the tie goes to the lower original index — the copy
        src = _cornell()                       # of the back wall comes after it in the description, the ceiling's copy before it, so that
        src.pop("small-box"), src.pop("large-box")      # whatever order the root's children take, one pair has the lower index second
        d = {}                                 # (eight rectangles, no box: the top level stays flat)
        for k, v in src.items():
            if k == "ceiling":
                d["ceiling-first"] = dict(v)
            d[k] = v
            if k == "back":
                d["back-again"] = dict(v)
        return mi.load_dict(d).data()
    if name == "cornell-panel":                # a tilted partition: a rectangle whose box is mostly empty (second_nearest)
        d = _cornell()
        d.pop("large-box")
        d["panel"] = {"type": "rectangle", "to_world": T().translate([-0.35, -0.3, -0.2]).rotate([0.2, 1, 0.1], 40.0).scale([0.45, 0.6, 1.0]),
                      "bsdf": {"type": "ref", "id": "white"}}
        return mi.load_dict(d).data()
    if name == "top-level-triangles":
        import scene_class_cases
        import pathlib
        return scene_class_cases.top_level_triangles(pathlib.Path(_tmp())).data()
    if name == "relay-room":                   # no cube: the room's rectangles, the relay quad of the NLOS example and its small copy
        d = _cornell()
        d.pop("small-box"), d.pop("large-box")
        bsdf = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.5]}}}
        d["relay"] = {"type": "obj", "filename": _obj("relay.obj", QUAD * 0.5 + np.array([0.1, 0.05, -0.3])), "face_normals": True, "bsdf": bsdf}
        d["relay-copy"] = {"type": "obj", "filename": _obj("relay_copy.obj", QUAD @ _relay_copy().T * 0.37 * 0.5 + np.array([-0.31, -0.22, 0.53])),
                           "face_normals": True, "bsdf": bsdf}
        return mi.load_dict(d).data()
    if name == "spheres":                      # a room that holds the ray origins, a ball in it, and a unit ball 10^3 away
        import delta_cases as DC
        light = {"type": "area", "radiance": {"type": "rgb", "value": [1.0, 1.0, 1.0]}}
        grey = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.5]}}
        return mi.load_dict({"type": "scene", "integrator": {"type": "transient_path", "max_depth": 2},
                             "sensor": DC._sensor({"width": 8, "height": 8}, 1, origin=(0.0, -3.0, 0.0), target=(0.0, 0.0, 0.0)),
                             "room": {"type": "sphere", "radius": 5.0, "center": [0.3, 0.2, -0.1], "flip_normals": True, "emitter": light, "bsdf": grey},
                             "ball": {"type": "sphere", "radius": 1.0, "center": [0.5, -0.4, 0.2], "bsdf": grey},
                             "far": {"type": "sphere", "radius": 1.0, "center": [1000.0, 30.0, -20.0], "bsdf": grey}}).data()
    if name == "loose-triangle":               # one loose triangle in the room: a leaf that is no pair, so no flat top level and no leaf-pair trait
        d = _cornell()
        d["loose"] = {"type": "obj", "filename": _obj("loose.obj", [[-0.3, 0.2, 0.5, 0.2, 0.25, 0.45, 0.0, 0.6, 0.3]]), "face_normals": True,
                      "bsdf": {"type": "ref", "id": "white"}}
        return mi.load_dict(d).data()
    if name == "mesh-boxes":
        import scene_class_cases
        import pathlib
        return scene_class_cases.mesh_boxes(pathlib.Path(_tmp())).data()
    if name in ("sticks", "sticks-small"):     # test_spatial_splits_equal_brute_force's 1500 long thin triangles: spatial splits, no LDS;
        rng = np.random.default_rng(11)        # 300 of them: leaves of more than one pair in a tree that fits LDS
        tris = []
        for i in range(1500 if name == "sticks" else 300):
            c = rng.uniform(-0.9, 0.9, 3)
            axis = _unit(rng.normal(size=3))
            side = _unit(np.cross(axis, rng.normal(size=3)))
            half = rng.uniform(0.05, 0.9) if i % 3 else rng.uniform(0.01, 0.05)
            tris.append([np.clip(p, -0.99, 0.99) for p in (c - half * axis, c + half * axis, c + 0.01 * side)])
        d = _cornell()
        d.pop("small-box"), d.pop("large-box")
        d["sticks"] = {"type": "obj", "filename": _obj(name + ".obj", tris), "face_normals": True,
                       "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.5]}}}
        return mi.load_dict(d).data()
    if name == "empty":
        return _raw(np.zeros((0, 9)))
    if name == "one-triangle":
        return _raw([[0, 0, 0, 1, 0, 0, 0, 1, 0]])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene(name):
    return _build(name)


# scene -> (forms, families).  The device child of a scene runs every form x flag set x family; the shadow forms run `shadow` alone.
SCENES = {
    "cornell": (("wide_lds", "wide_lds_multi", "q8_hbm", "q4_hbm", "flat_refs", "flat_table", "flat_table_shadow", "flat_table_hull"),
                ("random", "box_edges", "diagonals", "rect_borders", "tmax_ties", "wave_shapes", "shadow")),
    "cornell-rotated": (("wide_lds", "flat_refs", "flat_table"), ("box_edges",)),
    "cornell-sheared": (("wide_lds", "flat_refs", "flat_table"), ("box_edges",)),
    "cornell-twin-wall": (("wide_lds", "flat_refs", "flat_table"), ("random", "tmax_ties")),
    "cornell-panel": (("wide_lds", "flat_refs", "flat_table"), ("random", "second_nearest")),
    "top-level-triangles": (("wide_lds", "flat_leaves"), ("random", "diagonals")),
    "relay-room": (("wide_lds", "flat_leaves"), ("random", "diagonals")),
    "spheres": (("wide_lds", "q8_hbm", "q4_hbm"), ("random", "sphere_tangent")),
    "mesh-boxes": (("wide_lds", "wide_lds_multi", "q8_hbm", "q4_hbm"), ("random",)),
    "loose-triangle": (("wide_lds", "q8_hbm", "q4_hbm"), ("random",)),
    "sticks": (("q8_hbm", "q4_hbm"), ("random",)),
    "sticks-small": (("wide_lds", "q8_hbm", "q4_hbm"), ("random",)),
    "empty": (("wide_lds", "q8_hbm", "q4_hbm"), ("random",)),
    "one-triangle": (("wide_lds", "wide_lds_multi", "q8_hbm", "q4_hbm", "flat_leaves"), ("random",)),
}
# (scene, form) pairs the hook must REFUSE, with the code it answers: nothing is launched for them
REFUSALS = (("sticks", "wide_lds", ERR_LDS), ("mesh-boxes", "flat_refs", ERR_NOT_FLAT), ("cornell", "flat_leaves", ERR_TRAITS),
            ("top-level-triangles", "flat_refs", ERR_TRAITS), ("cornell-panel", "flat_table_hull", ERR_HULL), ("sticks", "flat_table", ERR_NOT_FLAT), ("empty", "flat_leaves", ERR_NOT_FLAT),
            ("spheres", "wide_lds_multi", ERR_TRAITS))
# the oracle has no analytic sphere (tests/test_sphere.py holds the host build to quadrature instead): on this scene the host walk is held
# to the f64 reference alone, and its five trees to each other
NO_ORACLE = {"spheres"}
# a tenth of this scene's rays end on two rectangles at once: which of them is hit is the tie rule's to say, not f64's — its `random`
# family is held to the oracle, and the plain Cornell box's to f64
COINCIDENT = {"cornell-twin-wall"}
# Two rays of a family that was tried and taken out again (rays from 3 000 to 30 000 room sizes away at the duplicated walls of
# cornell-twin-wall, 2 of 30 000): (origin, direction) as hex words, tmax = +inf.  Out there one ulp of t (1e-3) is fifty times the
# padding of a rectangle's box: the oracle's brute force hits the rim of a wall and every tree — host and device alike — culls its box.
# Outside what the renderer builds (a camera's far_clip is 100 and every other ray starts on the scene); test_walk_cases.py carries them
FAR_RAYS = (("c3f43b59 c5f2dc07 4619f019", "3d1f25e7 3f1e6e69 bf48d6f7"), ("c331add8 c5b285ea 464bcc48", "3c4c94a4 3ecd69c7 bf6a78d8"))
# families of all hits or all misses by construction: no hit-fraction rule
NO_FRACTION = {("empty", "random"), ("one-triangle", "random")}


def families_of(name, form):
    fams = SCENES[name][1]
    if form in SHADOW_FORMS:
        return ("shadow",)
    return tuple(f for f in fams if f != "shadow" and (f != "second_nearest" or form.startswith("flat")))


def expected_runs(name):
    """[(scene, form, suffix, family, n)] the device child of a scene must report, in its order"""
    out = []
    for form in SCENES[name][0]:
        for suffix in SUFFIXES:
            for fam in families_of(name, form):
                r = rays(name, fam)
                for var, idx in variants(r):
                    out.append([name, form, suffix, fam + var, int(len(idx))])
    return out


# ---------------------------------------------------------------------------------------------- scene geometry, from the description
def shapes_of(sd):
    """rectangles [(c, du, dv)], cubes [(3x4 to_world, first triangle)], spheres [(c, r)], loose two-triangle quads [(first, (2, 3, 3))]"""
    from mitransient_amd import _cabi
    rects, cubes, spheres, quads = [], [], [], []
    tv = np.asarray(sd.tri_verts, np.float64).reshape(-1, 3, 3)
    for s in range(sd.n_shapes):
        sh = sd.shapes[s]
        a, n = int(sh.first_tri), int(sh.n_tris)
        if (sh.kind & 0xff) == _cabi.MTR_SHAPE_SPHERE:
            spheres.append((np.array(list(sh.center), np.float64), float(sh.radius)))
        elif sh.is_rectangle & 1:
            rects.append((np.array(list(sh.center), np.float64), np.array(list(sh.du), np.float64), np.array(list(sh.dv), np.float64)))
        elif n == 12 and sh.has_to_world:
            cubes.append((np.array(list(sh.to_world), np.float64).reshape(3, 4), a))
        elif n == 2:
            quads.append((a, tv[a:a + 2]))
    return rects, cubes, spheres, quads


def scene_box(sd):
    rects, cubes, spheres, _ = shapes_of(sd)
    if spheres:                                      # the ball that holds the origins
        c, r = max(spheres, key=lambda s: s[1])
        return c - 0.55 * r, c + 0.55 * r
    tv = np.asarray(sd.tri_verts, np.float64).reshape(-1, 3)
    if not len(tv):
        return -np.ones(3), np.ones(3)
    lo, hi = tv.min(0), tv.max(0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return mid - 0.95 * np.maximum(half, 0.5), mid + 0.95 * np.maximum(half, 0.5)


# ---------------------------------------------------------------------------------------------- families
def _random(sd, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sd)
    o = rng.uniform(lo, hi, (n, 3))
    d = _unit(rng.normal(size=(n, 3)))
    d[:100, 0] = 0.0                                           # one, then two, components exactly zero (infinite reciprocals)
    d[100:200, 1] = 0.0
    d[200:250, :2] = 0.0
    d[250:300, 1:] = 0.0
    scale = float(np.max(hi - lo)) * 0.5
    tmax = np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.1, 2.0, n) * scale)
    zeros = {"one-zero": int(np.sum((d == 0.0).sum(1) == 1)), "two-zero": int(np.sum((d == 0.0).sum(1) == 2)), "finite-tmax": int(np.isfinite(tmax).sum()),
             "infinite-tmax": int(np.isinf(tmax).sum())}
    return Rays("random", o, _f32_unit(d), tmax, edges=zeros)


def _box_edges(sd, n, seed):
    """test_box_node_equals_brute_force's rays at the scene's first cube: faces, edges and corners in object space"""
    rng = np.random.default_rng(seed)
    _, cubes, _, _ = shapes_of(sd)
    M = cubes[0][0]
    A, b = M[:, :3], M[:, 3]
    to_w = lambda p: p @ A.T + b                                # noqa: E731
    tgt = rng.uniform(-1, 1, (n, 3))
    kind = rng.integers(0, 4, n)
    for i in range(3):
        snap = (kind >= 1) & (rng.random(n) < 0.75) | (kind == 3)
        tgt[snap, i] = np.sign(tgt[snap, i])
    tgt += rng.choice([0.0, 1e-7, 1e-5, 1e-3], (n, 1)) * rng.normal(size=(n, 3))
    org = rng.uniform(-3, 3, (n, 3))
    inside = rng.random(n) < 0.2
    org[inside] = rng.uniform(-0.999, 0.999, (int(inside.sum()), 3))
    on_face = rng.random(n) < 0.1
    ax = rng.integers(0, 3, n)
    org[on_face, ax[on_face]] = np.sign(org[on_face, ax[on_face]]) * (1.0 + rng.choice([0.0, 1e-6, 1e-4], int(on_face.sum())))
    tgt[on_face, ax[on_face]] = rng.uniform(-0.9, 0.9, int(on_face.sum()))          # (not IN the plane of that face: see the CPU test)
    dirs = to_w(tgt) - to_w(org)
    leaving = on_face & (rng.random(n) < 0.5)
    dirs[leaving] *= -1.0
    tmax = np.where(rng.random(n) < 0.7, np.inf, rng.uniform(0.1, 4.0, n) * np.abs(A).max())
    # the object-space entry point of a ray from outside, from the inputs alone: slabs of [-1, 1]^3 in f64
    dl = tgt - org
    dl[leaving] *= -1.0
    with np.errstate(all="ignore"):
        t0, t1 = (-1.0 - org) / dl, (1.0 - org) / dl
        tn = np.nanmax(np.minimum(t0, t1), axis=1)
        tf = np.nanmin(np.maximum(t0, t1), axis=1)
    entry = org + dl * tn[:, None]
    enters = (tn <= tf) & (tn > 0)
    near1 = (np.abs(np.abs(entry) - 1.0) < 1e-6).sum(1)
    edges = {"entry-on-a-face": int(np.sum(enters & (near1 == 1))), "entry-on-an-edge": int(np.sum(enters & (near1 == 2))),
             "entry-on-a-corner": int(np.sum(enters & (near1 == 3))), "origin-inside": int(inside.sum()), "origin-on-a-face": int(on_face.sum()),
             "leaving": int(leaving.sum())}
    return Rays("box_edges", to_w(org), _f32_unit(dirs), tmax, target=np.concatenate([org, tgt], 1), edges=edges)


def _some_short(rng, target, o, share=0.15):
    """tmax: +inf, and for a share of the rays a length that ends in front of the target (a family of hits alone would pass a walker
    that never misses)"""
    dist = np.linalg.norm(np.asarray(target, np.float64) - np.asarray(o, np.float64), axis=1)
    return np.where(rng.random(len(dist)) < share, dist * rng.uniform(0.3, 0.95, len(dist)), np.inf)


def _diagonals(sd, n, seed):
    """rays at the shared diagonal of every two-triangle quad — cube faces, loose quads, the carrier triangles' diagonal of an analytic
    rectangle: its centre (the laser spot behind kEdgeEps) for half of them, random points of it for the rest"""
    rng = np.random.default_rng(seed)
    rects, cubes, _, quads = shapes_of(sd)
    tv = np.asarray(sd.tri_verts, np.float64).reshape(-1, 3, 3)
    diags = [(c - du - dv, c + du + dv, np.cross(du, dv)) for c, du, dv in rects]
    pairs = [q for _, q in quads] + [tv[a + 2 * f:a + 2 * f + 2] for _, a in cubes for f in range(6)]
    for q in pairs:
        shared = [p for p in q[0] if any(np.array_equal(p, r) for r in q[1])]
        if len(shared) == 2:
            diags.append((shared[0], shared[1], np.cross(q[0][1] - q[0][0], q[0][2] - q[0][0])))
    assert diags
    which = rng.integers(0, len(diags), n)
    a = np.array([diags[k][0] for k in which]); b = np.array([diags[k][1] for k in which]); nrm = _unit(np.array([diags[k][2] for k in which]))
    lam = np.where(np.arange(n) < n // 2, 0.5, rng.uniform(0.02, 0.98, n))[:, None]
    target = a * (1 - lam) + b * lam
    dirs = _unit(rng.normal(size=(n, 3)))
    cosn = (dirs * nrm).sum(1)
    dirs = np.where((np.abs(cosn) > MIN_COS)[:, None], dirs, nrm)              # (not grazing)
    size = np.linalg.norm(b - a, axis=1, keepdims=True)
    o = (target + dirs * rng.uniform(0.05, 0.6, (n, 1)) * size).astype(np.float32)
    d = _f32_unit(target - o.astype(np.float64))
    edges = {"at-the-centre": int(n // 2), "along-the-diagonal": int(n - n // 2), "diagonals": len(diags)}
    return Rays("diagonals", o, d, _some_short(rng, target, o), target=target, edges=edges)


def _rect_borders(sd, n, seed):
    """rays at the border of every analytic rectangle, |lx| = 1 -+ {0, 1 ulp, 4 ulp, 1e-6}; in the Cornell box the walls' borders are the
    lines where two walls meet"""
    rng = np.random.default_rng(seed)
    rects, _, _, _ = shapes_of(sd)
    which = rng.integers(0, len(rects), n)
    c = np.array([rects[k][0] for k in which]); du = np.array([rects[k][1] for k in which]); dv = np.array([rects[k][2] for k in which])
    ulp = 2.0 ** -23
    off = rng.choice([0.0, ulp, 4 * ulp, 1e-6, -ulp, -4 * ulp, -1e-6], n)
    lx = np.sign(rng.uniform(-1, 1, n)) * (1.0 + off)
    ly = rng.uniform(-1, 1, n)
    swap = rng.random(n) < 0.5
    lx, ly = np.where(swap, ly, lx), np.where(swap, lx, ly)
    target = c + du * lx[:, None] + dv * ly[:, None]
    nrm = _unit(np.cross(du, dv))
    dirs = _unit(rng.normal(size=(n, 3)))
    cosn = (dirs * nrm).sum(1)
    dirs = np.where((np.abs(cosn) > MIN_COS)[:, None], dirs, nrm)
    size = np.linalg.norm(du, axis=1, keepdims=True)
    o = (target + dirs * rng.uniform(0.2, 1.5, (n, 1)) * size).astype(np.float32)
    d = _f32_unit(target - o.astype(np.float64))
    edges = {"on-the-border": int(np.sum(off == 0.0)), "outside-by-ulps": int(np.sum((off > 0) & (off < 1e-6))), "inside-by-ulps": int(np.sum((off < 0) & (off > -1e-6))),
             "by-1e-6": int(np.sum(np.abs(off) == 1e-6))}
    return Rays("rect_borders", o, d, _some_short(rng, target, o), target=np.stack([which, lx, ly], 1), edges=edges)


def _tmax_ties(sd, n, seed, hh):
    """tmax = the host walk's own t for the same ray, then t -+ 1 ulp: `t <= tmax` and the flat walk's tb = fminf(tmax, h.t) without slack.
    On a scene with a duplicated rectangle a third of the rays hit both copies at one t"""
    base = _random(sd, n, seed)
    hit4, _, _ = host_walk(hh, sd, base.o, base.d, np.full(n, np.inf, np.float32), "wide")
    tb = hit4[:, 0].copy()
    hit = hit4[:, 3] != 0xffffffff
    o, d, tb = base.o[hit], base.d[hit], tb[hit]
    assert np.all((tb > 0) & (tb < 0x7f800000))
    tm = np.concatenate([tb, tb - 1, tb + 1]).view(np.float32)
    edges = {"tmax-equals-t": int(hit.sum()), "tmax-one-ulp-below": int(hit.sum()), "tmax-one-ulp-above": int(hit.sum())}
    return Rays("tmax_ties", np.tile(o, (3, 1)), np.tile(d, (3, 1)), tm, edges=edges)


def _slab_entry(lo, hi, o, d):
    with np.errstate(all="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
        tn = np.maximum(np.nanmax(np.minimum(t0, t1), axis=1), 0.0)
        tf = np.nanmin(np.maximum(t0, t1), axis=1)
    return np.where(tn <= tf, tn, np.inf)


def rect_entry_order(sd, o, d):
    """per ray: the entry distances into the boxes of the scene's analytic rectangles (f64 slabs; inf: missed), for the second_nearest counts"""
    rects, _, _, _ = shapes_of(sd)
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    ent = []
    for c, du, dv in rects:
        corners = np.array([c + a * du + b * dv for a in (-1, 1) for b in (-1, 1)])
        ent.append(_slab_entry(corners.min(0), corners.max(0), o, d))
    return np.array(ent).T


def _second_nearest(sd, n, seed):
    """the flat walk's key-ordered rectangle loop: rays through the EMPTY part of a tilted rectangle's box, whose nearest-entry candidate
    the rectangle test itself refuses and whose hit is the second or third candidate; and rays that hit a wall within a few ulps of
    where the next wall's box begins (key2 & ~7)"""
    rng = np.random.default_rng(seed)
    rects, _, _, _ = shapes_of(sd)
    c, du, dv = rects[-1]                                    # the panel: the last rectangle of the description
    corners = np.array([c + a * du + b * dv for a in (-1, 1) for b in (-1, 1)])
    lo, hi = corners.min(0), corners.max(0)
    m = n // 2
    target = rng.uniform(lo, hi, (m, 3))
    blo, bhi = scene_box(sd)
    o1 = rng.uniform(blo, bhi, (m, 3)).astype(np.float32)
    d1 = _f32_unit(target - o1.astype(np.float64))
    # a hit on wall A at a point a few ulps from wall B's plane: targets on A = rects[k], pushed off its border towards the inside
    k = rng.integers(0, 5, n - m)
    ca = np.array([rects[1 + i][0] for i in k]); dua = np.array([rects[1 + i][1] for i in k]); dva = np.array([rects[1 + i][2] for i in k])
    inset = rng.choice([0.0, 2.0 ** -23, 2.0 ** -21, 2.0 ** -19, 1e-5], n - m)
    lx = np.sign(rng.uniform(-1, 1, n - m)) * (1.0 - inset)
    ly = rng.uniform(-0.95, 0.95, n - m)
    t2 = ca + dua * lx[:, None] + dva * ly[:, None]
    o2 = rng.uniform(blo * 0.6, bhi * 0.6, (n - m, 3)).astype(np.float32)
    d2 = _f32_unit(t2 - o2.astype(np.float64))
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    return Rays("second_nearest", o, d, _some_short(rng, np.concatenate([target, t2]), o), target=np.concatenate([target, t2]), edges={"through-the-panel-box": m, "at-a-wall-joint": n - m})


def _sphere_tangent(sd, n, seed):
    """grazing rays, the discriminant 0 -+ a few ulps, at every sphere (the far one from 10^3 away); origins inside; origins on the surface"""
    rng = np.random.default_rng(seed)
    _, _, spheres, _ = shapes_of(sd)
    which = rng.integers(0, len(spheres), n)
    c = np.array([spheres[k][0] for k in which]); r = np.array([spheres[k][1] for k in which])
    lo, hi = scene_box(sd)
    kind = rng.integers(0, 3, n)                              # 0 grazing from the origin box, 1 origin inside, 2 origin on the surface
    o = rng.uniform(lo, hi, (n, 3))
    # grazing: aim at a point of the silhouette circle seen from o, impact parameter r (1 + k ulp)
    to_c = c - o
    dist = np.linalg.norm(to_c, axis=1)
    axis = to_c / dist[:, None]
    side = _unit(np.cross(axis, rng.normal(size=(n, 3))))
    ulps = rng.choice([0.0, 1.0, -1.0, 2.0, -2.0, 8.0, -8.0, 64.0, -64.0], n) * 2.0 ** -23
    bpar = r * (1.0 + ulps)
    graze_ok = (kind == 0) & (dist > 1.01 * r)
    sin_a = np.clip(bpar / np.maximum(dist, 1e-30), 0.0, 1.0)
    d_graze = axis * np.sqrt(1.0 - sin_a ** 2)[:, None] + side * sin_a[:, None]
    d = _unit(rng.normal(size=(n, 3)))
    d = np.where(graze_ok[:, None], d_graze, d)
    ins = kind == 1
    o[ins] = (c + _unit(rng.normal(size=(n, 3))) * (r * rng.uniform(0.0, 0.999, n))[:, None])[ins]
    surf = kind == 2
    nrm = _unit(rng.normal(size=(n, 3)))
    o[surf] = (c + nrm * (r * (1.0 + rng.choice([0.0, 1e-6, -1e-6, 1e-4, -1e-4], n)))[:, None])[surf]
    tmax = np.where(rng.random(n) < 0.6, np.inf, rng.uniform(0.5, 12.0, n))
    edges = {"grazing": int(graze_ok.sum()), "grazing-the-far-ball": int(np.sum(graze_ok & (dist > 500.0))), "origin-inside": int(ins.sum()),
             "origin-on-the-surface": int(surf.sum()), "leaving-the-surface": int(np.sum(surf & ((d * nrm).sum(1) > 0)))}
    return Rays("sphere_tangent", o, _f32_unit(d), tmax, target=np.stack([which, ulps], 1), edges=edges)


# ---- shadow: (sp, gn, u1, u2); the ray is built on the device and by hh_walk_shadow, rect_emitter_point and shadow_ray_to
def hull_of(hh, sd):
    """the scene's ShadowHull (margin 1) from the host classifier: dict of count, e_child, e_delta, e_row, delta, row; its traits; tree sizes"""
    hull = (C.c_uint32 * 48)()
    tr = C.c_uint32(0)
    sizes = (C.c_uint32 * 5)()
    desc = sd.desc()
    assert hh.hh_walk_scene_info(C.byref(desc), hull, C.byref(tr), sizes) == 0
    w = np.frombuffer(hull, np.uint32).copy()
    f = w.view(np.float32)
    return ({"count": int(w[0]), "e_child": int(w[1]), "e_delta": float(f[2]), "e_row": f[4:8].astype(np.float64), "delta": f[8:16].astype(np.float64),
             "row": f[16:48].reshape(8, 4).astype(np.float64)}, int(tr.value), [int(x) for x in sizes])


def hull_tiers(hull, so):
    """mtr_core.h's guard re-stated: per computed origin, (risky_h, risky_e) — hull_side(row, o) >= delta fails for a hull row / for E"""
    so = np.asarray(so, np.float64)
    side = so @ hull["row"][:, :3].T + hull["row"][:, 3]
    risky_h = np.any(~(side[:, :hull["count"]] >= hull["delta"][:hull["count"]]), axis=1)
    risky_e = ~(so @ hull["e_row"][:3] + hull["e_row"][3] >= hull["e_delta"])
    return risky_h, risky_e


def _shadow(sd, n_waves, seed, hh):
    """surface points on every wall, on the boxes' faces, within e_delta of the emitter's plane and within delta_k of a wall's plane.
    Whole waves of 64: all lanes safe; exactly one lane risky_e; exactly one lane risky_h — so that all three tiers of SHADOW HULL run"""
    rng = np.random.default_rng(seed)
    hull, _, _ = hull_of(hh, sd)
    rects, cubes, _, _ = shapes_of(sd)
    n = 64 * n_waves
    E = rects[0]                                              # the light: the first rectangle of the Cornell box's description
    walls = rects[1:]
    en = _unit(np.cross(E[1], E[2]))
    en = en if (hull["e_row"][:3] @ en) > 0 else -en          # the side E shines on
    centre = np.mean([c for c, _, _ in walls], axis=0)

    def on_wall(m, lift, along=False):
        k = rng.integers(0, len(walls), m)
        c = np.array([walls[i][0] for i in k]); du = np.array([walls[i][1] for i in k]); dv = np.array([walls[i][2] for i in k])
        nrm = _unit(np.cross(du, dv))
        nrm = np.where(((centre - c) * nrm).sum(1)[:, None] > 0, nrm, -nrm)           # into the room
        p = c + du * rng.uniform(-0.97, 0.97, (m, 1)) + dv * rng.uniform(-0.97, 0.97, (m, 1)) + nrm * lift
        if along:          # the normal of a surface that STANDS on the wall (a box's side where it meets the floor): the offset stays in the plane
            ang = rng.uniform(0, 2 * np.pi, (m, 1))
            nrm = _unit(_unit(du) * np.cos(ang) + _unit(dv) * np.sin(ang))
        return p, nrm

    def on_box(m):
        M, _ = cubes[rng.integers(0, len(cubes))]
        A, b = M[:, :3], M[:, 3]
        pl = rng.uniform(-0.95, 0.95, (m, 3))
        ax = rng.integers(0, 3, m); sg = np.sign(rng.uniform(-1, 1, m))
        pl[np.arange(m), ax] = sg
        nl = np.zeros((m, 3)); nl[np.arange(m), ax] = sg
        return pl @ A.T + b, _unit(nl @ np.linalg.inv(A))     # (normals go with the inverse transpose)

    def safe(m):
        # well inside the room, on surfaces lifted off their planes far beyond any delta: floating boxes' faces and points in the air
        p1, n1 = on_box(m)
        p2, n2 = on_wall(m, 0.2)
        pick = (rng.random(m) < 0.5)[:, None]
        return np.where(pick, p1, p2), np.where(pick, n1, n2)

    u = rng.random((n, 2))
    sp, gn = safe(n)
    # (a box's bottom face lies in or under the floor: whatever the guard calls risky is moved into the air, 0.2 off a wall)
    ray7 = host_walk_shadow(hh, sd, sp, _f32_unit(gn), u)[0]
    rh, re = hull_tiers(hull, ray7[:, :3])
    p2, n2 = on_wall(n, 0.2)
    sp, gn = np.where((rh | re)[:, None], p2, sp), np.where((rh | re)[:, None], n2, gn)
    kind = np.zeros(n, np.int64)
    lane = rng.integers(0, 64, n_waves)
    for w in range(n_waves):
        i = 64 * w + lane[w]
        if w % 3 == 1:                                        # one lane within e_delta of E's plane, in front of it
            a, b = rng.uniform(-3, 3, 2)
            sp[i] = E[0] + E[1] * a + E[2] * b + en * hull["e_delta"] * rng.uniform(0.05, 0.3)
            gn[i] = en
            kind[i] = 1
        elif w % 3 == 2:                                      # one lane IN a wall's plane, and staying there (within delta_k)
            p, nn = on_wall(1, 0.0, along=True)
            sp[i], gn[i] = p[0], nn[0]
            kind[i] = 2
    # half of the all-safe waves' rays start on the walls proper — every wall, lanes that are risky_h by the dozen — as a bounce does
    for w in range(0, n_waves, 6):
        p, nn = on_wall(64, 0.0)
        pa, na = on_wall(64, 0.0, along=True)
        pick = (rng.random(64) < 0.3)[:, None]
        sp[64 * w:64 * w + 64], gn[64 * w:64 * w + 64] = np.where(pick, pa, p), np.where(pick, na, nn)
        kind[64 * w:64 * w + 64] = 3
    return Rays("shadow", sp, _f32_unit(gn), u.astype(np.float32), target=kind[:, None].astype(np.float64),
                edges={"aimed-at-e-delta": int(np.sum(kind == 1)), "on-a-wall-alone": int(np.sum(kind == 2)), "on-the-walls": int(np.sum(kind == 3))})


def _wave_shapes(sd, seed):
    base = _random(sd, 300, seed)
    rng = np.random.default_rng(seed + 1)
    var = [("", np.arange(300))] + [(f"/n={k}", np.arange(k)) for k in (1, 63, 64, 65, 257)] + [(f"/perm{j}", rng.permutation(300)) for j in range(3)]
    var.append(("/lane37", np.arange(300)))                    # one real ray in lane 37, tmax = 0 everywhere else (test_gpu_walk.py)
    base.family = "wave_shapes"
    base.variants = var
    return base


LANE37 = 37


def variants(r):
    """[(suffix of the family's name, indices into the family's rays)]: the device runs a family once per variant"""
    return r.variants if r.variants else [("", np.arange(r.n))]


def variant_rays(r, var, idx):
    o, d, tm = r.o[idx], r.d[idx], r.tmax[idx]
    if var == "/lane37":
        tm = np.zeros_like(tm)
        tm[LANE37::64] = r.tmax[idx][LANE37::64]
    return o, d, tm


SIZES = {"random": 20000, "box_edges": 60000, "diagonals": 30000, "rect_borders": 30000, "tmax_ties": 8000, "second_nearest": 30000,
         "sphere_tangent": 40000, "shadow": 384}
_HH = None


def host_harness():
    global _HH
    if _HH is None:
        import __graft_entry__ as g
        _HH = C.CDLL(g.build_host_harness())
    return _HH


@functools.lru_cache(maxsize=None)
def rays(name, family):
    sd = scene(name)
    seed = zlib.crc32(name.encode()) % 100000
    n = SIZES.get(family, 0)
    if name == "sticks":
        n = 12000
    if family == "random":
        r = _random(sd, n, seed)
    elif family == "box_edges":
        r = _box_edges(sd, n, seed + 1)
    elif family == "diagonals":
        r = _diagonals(sd, n, seed + 2)
    elif family == "rect_borders":
        r = _rect_borders(sd, n, seed + 3)
    elif family == "tmax_ties":
        r = _tmax_ties(sd, n, seed + 4, host_harness())
    elif family == "second_nearest":
        r = _second_nearest(sd, n, seed + 5)
    elif family == "sphere_tangent":
        r = _sphere_tangent(sd, n, seed + 6)
    elif family == "shadow":
        r = _shadow(sd, n, seed + 7, host_harness())
    elif family == "wave_shapes":
        r = _wave_shapes(sd, seed + 8)
    else:
        raise KeyError(family)
    check_finite(r)
    assert r.n <= 200000
    return r


# ---------------------------------------------------------------------------------------------- the host twin
def host_walk(hh, sd, o, d, tmax, tree="wide"):
    """hh_walk through one of HOST_TREES: (hit4 (n, 4) u32 = t, u, v bits and slot, original index (n) i32, occlusion (n) u8)"""
    n = len(o)
    o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
    hit4 = np.zeros((n, 4), np.uint32); orig = np.zeros(n, np.int32); occ = np.zeros(n, np.uint8)
    pairs, wide = HOST_TREES[tree]
    desc = sd.desc()
    hh.hh_set_node_pairs(pairs); hh.hh_set_wide(wide)
    try:
        if n:
            rc = hh.hh_walk(C.byref(desc), C.c_uint32(n), C.c_void_p(o.ctypes.data), C.c_void_p(d.ctypes.data), C.c_void_p(tmax.ctypes.data),
                            C.c_void_p(hit4.ctypes.data), C.c_void_p(orig.ctypes.data), C.c_void_p(occ.ctypes.data))
            assert rc == 0, rc
    finally:
        hh.hh_set_node_pairs(0); hh.hh_set_wide(0)
    return hit4, orig, occ


def host_walk_shadow(hh, sd, sp, gn, u2, tree="wide"):
    """hh_walk_shadow: (ray7 (n, 7) f32 = o, d, tmax as built, hit4, original index, occlusion)"""
    n = len(sp)
    sp = np.ascontiguousarray(sp, np.float32); gn = np.ascontiguousarray(gn, np.float32); u2 = np.ascontiguousarray(u2, np.float32)
    ray7 = np.zeros((n, 7), np.float32); hit4 = np.zeros((n, 4), np.uint32); orig = np.zeros(n, np.int32); occ = np.zeros(n, np.uint8)
    pairs, wide = HOST_TREES[tree]
    desc = sd.desc()
    hh.hh_set_node_pairs(pairs); hh.hh_set_wide(wide)
    try:
        rc = hh.hh_walk_shadow(C.byref(desc), C.c_uint32(n), C.c_void_p(sp.ctypes.data), C.c_void_p(gn.ctypes.data), C.c_void_p(u2.ctypes.data),
                               C.c_void_p(ray7.ctypes.data), C.c_void_p(hit4.ctypes.data), C.c_void_p(orig.ctypes.data), C.c_void_p(occ.ctypes.data))
        assert rc == 0, rc
    finally:
        hh.hh_set_node_pairs(0); hh.hh_set_wide(0)
    return ray7, hit4, orig, occ


def host_answer(hh, name, family, form, var="", idx=None):
    """what a device form must return for (a variant of) a family: hit4, occlusion"""
    r = rays(name, family)
    idx = np.arange(r.n) if idx is None else idx
    sd = scene(name)
    if family == "shadow":
        _, hit4, _, occ = host_walk_shadow(hh, sd, r.o[idx], r.d[idx], r.tmax[idx], TWIN[form])
    else:
        o, d, tm = variant_rays(r, var, idx)
        hit4, _, occ = host_walk(hh, sd, o, d, tm, TWIN[form])
    return hit4, occ


def describe(name, family, i):
    """the ray, replayable: origin, direction and tmax as hex words, and what it was aimed at"""
    r = rays(name, family)
    hexs = lambda a: " ".join(f"{int(w):08x}" for w in np.atleast_1d(a).view(np.uint32))       # noqa: E731
    tgt = "" if r.target is None else f" target {np.array2string(r.target[i], precision=17)}"
    return f"{name}/{family}[{i}] o {hexs(r.o[i])} d {hexs(r.d[i])} tmax {hexs(r.tmax[i])} (o {r.o[i]}, d {r.d[i]}, tmax {r.tmax[i]}){tgt}"
