"""The white-furnace identity (tests/test_furnace.py on the CPU, tests/test_gpu_furnace.py on the GPU): scene builders, the
statistic, and the GPU steps, each run in a child process of its own (the test gives each step a time limit):
``python tests/furnace_cases.py <case>`` prints one JSON line.

A closed room whose every wall is a `diffuse` reflector of albedo rho and an `area` emitter of radiance Le carries, along every
camera ray,  L_D = Le sum_{k<D} rho^k  at max_depth D and  L_inf = Le / (1 - rho)  without a depth limit (roulette on); a lossless
object inside leaves L_inf as it is and the field unpolarized.  Nothing here reads the oracle's arithmetic: the expectation is the
closed form."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

RHO, LE = (0.7, 0.5, 0.3), (1.0, 2.0, 0.5)
POL_RHO, POL_LE = 0.6, 1.5                  # the *_mono_polarized room
HALF = (1.0, 1.5, 2.0)                      # the room is 2 x 3 x 4
CPU_SIZE, GPU_SIZE = (32, 128), (64, 256)   # (film edge, samples per pixel)
GRAD_SEEDS, GRAD_SIZE = 16, (32, 32)        # reverse mode: one number per seed
# The derivative of L_inf in rho weights a path of k bounces by k: at rho = 0.7 its relative variance is 13 times that of L_inf
# itself (measured: se / expected 0.255 % over 16 x 32 x 32 x 32 samples, 0.55 % over 32 x 32 x 128), so at the sizes above
# 4 se is 1.02 % and 2.2 % — over the 1 % power cap with no bias in sight (z 0.15 and -0.31).  These cases take more samples;
# the bounds stay.
GRAD_SIZE_INF, FWD_SIZE_INF_CPU, FWD_SIZE_INF_GPU = (32, 128), (64, 512), (128, 256)


def grad_size(D):
    return GRAD_SIZE_INF if D < 0 else GRAD_SIZE


# -- the closed forms ------------------------------------------------------------------------------------------------------
def radiance(D, rho=RHO, le=LE):
    """L_D per channel; D = -1: L_inf"""
    r, le = np.atleast_1d(np.asarray(rho, np.float64)), np.atleast_1d(np.asarray(le, np.float64))
    return le / (1.0 - r) if D < 0 else le * sum(r ** k for k in range(D))


def d_radiance_d_rho(D, rho=RHO, le=LE):
    """the derivative of L_D in the common albedo: Le sum k rho^(k-1); D = -1: Le / (1 - rho)^2"""
    r, le = np.atleast_1d(np.asarray(rho, np.float64)), np.atleast_1d(np.asarray(le, np.float64))
    return le / (1.0 - r) ** 2 if D < 0 else le * sum(k * r ** (k - 1) for k in range(1, D))


def d_radiance_d_le(D, rho=RHO):
    """... in the common radiance: sum rho^k; D = -1: 1 / (1 - rho)"""
    return radiance(D, rho, np.ones(len(np.atleast_1d(rho))))


def neighbours(D, rho=RHO, le=LE):
    """the expectations a test must reject beside +-1 %: L_(D-1) and L_(D+1); L_inf has no order above it, and below it the series
    cut at order 8 (short by rho^8: 5.8 % in the red channel, 1.7 % in the polarized room; order 16 is short by 0.33 %, which no
    test with a 1 % power condition tells apart)"""
    return [radiance(CUT, rho, le)] if D < 0 else [radiance(D - 1, rho, le), radiance(D + 1, rho, le)]


CUT = 8


def wrong_orders(D):
    return (CUT,) if D < 0 else (D - 1, D + 1)


# -- the statistic ---------------------------------------------------------------------------------------------------------
def holds(samples, expected, scale=None):
    """samples (n, channels): independent values of one expectation per channel.  |mean - expected| <= 4 se AND the power
    condition 4 se <= 1 % of `scale` (the expectation itself unless given: the Stokes components are held to 0 on the scale
    of L_inf)"""
    x = np.asarray(samples, np.float64)
    x = x.reshape(x.shape[0], -1)
    e = np.broadcast_to(np.asarray(expected, np.float64), x.shape[1:])
    s = np.abs(e) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), e.shape)
    m, se = x.mean(0), x.std(0, ddof=1) / np.sqrt(x.shape[0])
    return bool(np.all(np.abs(m - e) <= 4.0 * se) and np.all(4.0 * se <= 0.01 * s))


def verdict(samples, expected, others=(), scale=None):
    """the figures of one comparison and whether it holds — and whether the same data fail against expected (1 +- 0.01)
    (an expectation of 0: against +- 1 % of the scale) and against each of `others`"""
    x = np.asarray(samples, np.float64)
    x = x.reshape(x.shape[0], -1)
    e = np.broadcast_to(np.asarray(expected, np.float64), x.shape[1:]).copy()
    s = np.abs(e) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), e.shape)
    m, se = x.mean(0), x.std(0, ddof=1) / np.sqrt(x.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(se > 0, (m - e) / se, 0.0)
    wrong = [e + 0.01 * s, e - 0.01 * s] + [np.asarray(o, np.float64) for o in others]
    return {"mean": m.tolist(), "se": se.tolist(), "expected": e.tolist(), "z": z.tolist(), "rel_se": (se / s).tolist(),
            "n": int(x.shape[0]), "holds": holds(x, e, s), "rejects": [not holds(x, w, s) for w in wrong]}


def assert_verdict(v, label=""):
    print(f"[furnace] {label}: z {np.round(v['z'], 2).tolist()} se/expected {['%.2e' % r for r in v['rel_se']]}")
    assert v["holds"], (label, v)
    assert all(v["rejects"]), (label, v)


def worst(vs):
    """(worst |z|, worst se / expected) of a family's verdicts"""
    return max(abs(z) for v in vs for z in v["z"]), max(r for v in vs for r in v["rel_se"])


def pixels(img):
    a = np.asarray(img, np.float64)
    return a.reshape(-1, a.shape[-1])


# -- scenes ----------------------------------------------------------------------------------------------------------------
def _mi(variant="llvm_ad_rgb"):
    import mitransient_amd.mi as mi
    mi.set_variant(variant)
    return mi


def wall_transforms(flipped=()):
    """the six rectangles ([-1, 1]^2, normal +z) of the room, facing inward; a wall named in `flipped` is built facing outward
    (its shape then takes flip_normals)"""
    from mitransient_amd.transform import ScalarTransform4f as T
    hx, hy, hz = HALF
    spec = {"back": ([0, 0, -hz], None, 0.0, [hx, hy, 1]), "front": ([0, 0, hz], [0, 1, 0], 180.0, [hx, hy, 1]),
            "left": ([-hx, 0, 0], [0, 1, 0], 90.0, [hz, hy, 1]), "right": ([hx, 0, 0], [0, 1, 0], -90.0, [hz, hy, 1]),
            "floor": ([0, -hy, 0], [1, 0, 0], -90.0, [hx, hz, 1]), "ceil": ([0, hy, 0], [1, 0, 0], 90.0, [hx, hz, 1])}
    out = {}
    for name, (at, axis, angle, scale) in spec.items():
        if name in flipped:
            axis, angle = (axis or [0, 1, 0]), angle + 180.0
        t = T().translate(at)
        out[name] = (t.rotate(axis, angle) if axis is not None else t).scale(scale)
    return out


WALLS = ("back", "front", "left", "right", "floor", "ceil")
CAMERA = dict(origin=[0.3, -0.2, 1.2], target=[-0.2, 0.1, -1.0], up=[0, 1, 0])     # off-centre and tilted


def _colour(v):
    return {"type": "rgb", "value": [float(x) for x in v]} if np.ndim(v) else float(v)


def room_dict(max_depth, rr_depth, size=CPU_SIZE, rho=RHO, le=LE, walls=WALLS, extra=None, twosided=(), flipped=(), reflectance=None,
              bins=64, bin_width=1.0, sensor=None, film=None, **integrator):
    """the furnace: every wall of `walls` a rectangle with a BSDF and an emitter of its own; `extra`: more shapes; `reflectance`:
    what the walls' BSDFs take instead of the constant rho (a bitmap); a 64-bin film window [0, 64) — every path of max_depth
    <= 6 ends inside it (6 segments of at most the room's diagonal, 5.39)"""
    from mitransient_amd.transform import ScalarTransform4f as T
    res, spp = size
    d = {"type": "scene",
         "integrator": dict({"type": "transient_path", "max_depth": max_depth, "rr_depth": rr_depth}, **integrator),
         "sensor": {"type": "perspective", "fov": 70.0, "near_clip": 0.01, "far_clip": 100.0, "to_world": T().look_at(**CAMERA),
                    "sampler": {"type": "independent", "sample_count": spp},
                    "film": {"type": "transient_hdr_film", "width": res, "height": res, "rfilter": {"type": "box"},
                             "temporal_bins": bins, "start_opl": 0.0, "bin_width_opl": bin_width}}}
    d["sensor"].update(sensor or {})
    d["sensor"]["film"].update(film or {})
    tw = wall_transforms(flipped)
    for name in walls:
        bsdf = {"type": "diffuse", "reflectance": _colour(rho) if reflectance is None else dict(reflectance)}
        if name in twosided:
            bsdf = {"type": "twosided", "bsdf": bsdf}
        d[name] = {"type": "rectangle", "to_world": tw[name], "bsdf": bsdf, "emitter": {"type": "area", "radiance": _colour(le)}}
        if name in flipped:
            d[name]["flip_normals"] = True
    d.update(extra or {})
    return d


def room(*a, variant="llvm_ad_rgb", **kw):
    return _mi(variant).load_dict(room_dict(*a, **kw))


def glass_cube():
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "cube", "to_world": T().translate([-0.2, 0, -0.5]).rotate([0, 1, 0], 30).scale(0.4),
            "bsdf": {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0}}


def thin_pane():
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "rectangle", "to_world": T().translate([0.3, 0.2, 0.4]).rotate([1, 0, 0], 20).scale(0.6),
            "bsdf": {"type": "thindielectric", "int_ior": 1.5, "ext_ior": 1.0}}


def far_rough_conductor():
    """an object outside the closed room: no path reaches it, the scene takes the lobe code all the same"""
    from mitransient_amd.transform import ScalarTransform4f as T
    return {"type": "cube", "to_world": T().translate([20.0, 20.0, 20.0]).scale(0.5),
            "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": 0.2, "eta": [0.2, 0.9, 1.1], "k": [3.9, 2.4, 2.2]}}


INCLUSIONS = {
    "glass": lambda: dict(extra={"inner": glass_cube()}), "thin": lambda: dict(extra={"pane": thin_pane()}),
    "glass_and_thin": lambda: dict(extra={"inner": glass_cube(), "pane": thin_pane()}),
    "twosided": lambda: dict(twosided=("left",)), "flip_normals": lambda: dict(flipped=("back", "floor")),
}


def write_room_obj(path, n, walls=WALLS):
    """the walls as one OBJ without vn (the shape takes face_normals: flat-shaded), inward-facing: each an n x n grid whose cuts lie at (i / n)^2 of the edge, so that
    its cells' areas differ by (2 n - 1)^2 (49 for n = 4) — picking triangles uniformly instead of by area would show.
    Returns (number of triangles, largest / smallest triangle area)"""
    cuts = -1.0 + 2.0 * (np.arange(n + 1) / n) ** 2
    tw = wall_transforms()
    lines, areas, nv = [], [], 0
    for name in walls:
        for i in range(n):
            for j in range(n):
                quad = np.array([[cuts[i], cuts[j], 0], [cuts[i + 1], cuts[j], 0], [cuts[i + 1], cuts[j + 1], 0], [cuts[i], cuts[j + 1], 0]])
                w = tw[name].transform_affine(quad)
                lines += [f"v {p[0]!r} {p[1]!r} {p[2]!r}" for p in w.tolist()]
                lines += [f"f {nv + 1} {nv + 2} {nv + 3}", f"f {nv + 1} {nv + 3} {nv + 4}"]
                areas += [0.5 * np.linalg.norm(np.cross(w[1] - w[0], w[2] - w[0]))] * 2
                nv += 4
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return len(areas), max(areas) / min(areas)


MESH_SMALL, MESH_LARGE = 4, 9              # 192 triangles: staged in LDS; 972: walked in HBM (the staircase stand-in has 852)


def mesh_room(tmp, n, max_depth=-1, rr_depth=3, size=CPU_SIZE, mixed=False, **kw):
    """the room as a mesh emitter (mixed: back, left and floor as the mesh, the other three walls rectangles)"""
    tmp = str(tmp)
    names = ("back", "left", "floor") if mixed else WALLS
    n_tris, ratio = write_room_obj(os.path.join(tmp, f"room_{n}_{int(mixed)}.obj"), n, names)
    assert ratio >= 10.0
    # (face_normals: an OBJ without vn gets vertex normals averaged over the vertices that share a position — across the room's edges)
    mesh = {"type": "obj", "filename": os.path.join(tmp, f"room_{n}_{int(mixed)}.obj"), "face_normals": True,
            "bsdf": {"type": "diffuse", "reflectance": _colour(RHO)}, "emitter": {"type": "area", "radiance": _colour(LE)}}
    scene = room(max_depth, rr_depth, size, walls=[w for w in WALLS if w not in names], extra={"mesh": mesh}, **kw)
    sd = scene.data()
    assert sd.tri_verts.shape[0] == n_tris + 2 * (6 - len(names))
    return scene


def bitmap_room(tmp, max_depth=-1, rr_depth=3, size=CPU_SIZE, extra=None, **kw):
    """rho as a constant 4 x 4 bitmap on every wall's `diffuse` (the texels are set in the flattened tables: linear values)"""
    from PIL import Image
    path = os.path.join(str(tmp), "rho.png")
    Image.fromarray(np.full((4, 4, 3), 128, np.uint8)).save(path)
    scene = room(max_depth, rr_depth, size, reflectance={"type": "bitmap", "filename": path}, extra=extra, **kw)
    sd = scene.data()
    assert len(sd.textures) >= 1
    for t in sd.textures:
        t[...] = np.asarray(RHO, np.float32)
    for m in range(sd.n_materials):
        if sd.materials[m].albedo_texture:
            for k in range(3):
                sd.materials[m].a[k] = RHO[k]
    return scene


def _tmp():
    import pathlib
    import tempfile
    return pathlib.Path(tempfile.mkdtemp(prefix="furnace_"))


# -- CPU renders -----------------------------------------------------------------------------------------------------------
def params_of(scene, seed=0):
    spp = scene.sensors()[0].sampler().sample_count()
    return scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)


def oracle_film(scene, seed=0):
    """the oracle's developed (steady (H, W, 3), transient (H, W, T, 3))"""
    from oracle import oracle
    sd = scene.data()
    t4, s4, _ = oracle.render(sd, params_of(scene, seed), use_bvh=True)
    t3, s3 = oracle.develop(sd.film, t4, s4)
    return s3, t3


def host_film(hh, scene, seed=0):
    """the host harness's (tests/host_harness.cpp over mtr_core.h), developed the same way"""
    from conftest import hh_render
    from oracle import oracle
    sd = scene.data()
    t4, s4, _ = hh_render(hh, sd, params_of(scene, seed))
    t3, s3 = oracle.develop(sd.film, t4, s4)
    return s3, t3


def wall_indices(scene):
    """(material indices, emitter indices) of the room's surfaces: every diffuse material and every emitter"""
    sd = scene.data()
    return [m for m in range(sd.n_materials) if sd.materials[m].type == 0], list(range(sd.n_emitters))


def mean_upstream(scene):
    """g_s = 1 / n_pixels, g_t = 0: the loss is the mean of the steady image per channel"""
    f = scene.data().film
    g_s = np.full((f.crop_height, f.crop_width, 3), 1.0 / (f.crop_height * f.crop_width), np.float32)
    return g_s, np.zeros((f.height, f.width, f.temporal_bins, 3), np.float32)


# -- the f64 pinhole camera ------------------------------------------------------------------------------------------------
CAMERAS = {      # (film width, height, fov_axis, crop window (w, h, x, y) or None)
    "x": (24, 16, "x", None), "y": (24, 16, "y", None), "diagonal": (24, 16, "diagonal", None), "smaller": (24, 16, "smaller", None),
    "larger": (24, 16, "larger", None), "tall_smaller": (16, 24, "smaller", None), "tall_larger": (16, 24, "larger", None),
    "tall_y": (16, 24, "y", None), "crop": (24, 16, "x", (7, 5, 11, 6)), "tall_crop": (16, 24, "diagonal", (5, 9, 2, 13)),
}
CAMERA_FOV, CAMERA_NEAR = 55.0, 0.25


def camera_room(name, size_spp=8, **kw):
    w, h, axis, crop = CAMERAS[name]
    film = {"width": w, "height": h}
    if crop is not None:
        film.update(crop_width=crop[0], crop_height=crop[1], crop_offset_x=crop[2], crop_offset_y=crop[3])
    return room(2, 3, (16, size_spp), sensor={"fov": CAMERA_FOV, "fov_axis": axis, "near_clip": CAMERA_NEAR}, film=film, **kw)


def pinhole_ray(name, px, py, jx, jy):
    """the ray through crop-window pixel (px, py) at jitter (jx, jy), from the definition of the field of view: the film is
    the rectangle |x| <= tan(fov_x / 2), |y| <= tan(fov_x / 2) / aspect of the plane z = 1 in front of the pinhole, the full
    angle `fov` spans the axis fov_axis names (the diagonal: the rectangle's diagonal), pixel (0, 0) is the top-left corner as
    seen along the viewing direction, and the ray starts where it crosses the near plane z = near_clip"""
    w, h, axis, crop = CAMERAS[name]
    ox, oy = (crop[2], crop[3]) if crop is not None else (0, 0)
    aspect = w / h
    t = np.tan(np.radians(CAMERA_FOV) / 2.0)
    if axis == "smaller":
        axis = "x" if w < h else "y"
    elif axis == "larger":
        axis = "x" if w > h else "y"
    tx = {"x": t, "y": t * aspect, "diagonal": t / np.sqrt(1.0 + 1.0 / aspect ** 2)}[axis]
    ty = tx / aspect
    u, v = (ox + px + jx) / w, (oy + py + jy) / h
    origin, target, up = (np.asarray(CAMERA[k], np.float64) for k in ("origin", "target", "up"))
    fwd = (target - origin) / np.linalg.norm(target - origin)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    d = fwd + (2.0 * u - 1.0) * tx * right + (1.0 - 2.0 * v) * ty * upv
    d /= np.linalg.norm(d)
    return origin + d * (CAMERA_NEAR / np.dot(d, fwd)), d


def camera_samples(name):
    """corner and centre pixels of the crop window, each at jitter 0 and 0.999"""
    w, h, _, crop = CAMERAS[name]
    cw, ch = (crop[0], crop[1]) if crop is not None else (w, h)
    return [(px, py, j, k) for px in (0, cw // 2, cw - 1) for py in (0, ch // 2, ch - 1) for j in (0.0, 0.999) for k in (0.0, 0.999)]


# -- GPU steps -------------------------------------------------------------------------------------------------------------
ORGANISATIONS = {"fused": dict(amd_mode="fused"), "wavefront": dict(amd_mode="wavefront"),
                 "deterministic": dict(amd_mode="fused", amd_deterministic=True)}


def gpu_film(scene, seed=0):
    """(steady, transient) of a render and what ran: the organisation mtr_render_plan names for these parameters, checked
    against the launches the render reports, the trait word, and where the scene's tables lie"""
    import torch
    from mitransient_amd import _cabi
    import grad_gpu_cases as GC
    integ = scene.integrator()
    integ.collect_stats = True
    spp = scene.sensors()[0].sampler().sample_count()
    s, t = integ.render(scene, seed=seed, spp=spp)
    torch.cuda.synchronize()
    planned = integ.resolved_mode(scene, scene.sensors()[0], spp)           # (mtr_render_plan, the film prepared)
    ran = "wavefront" if integ.total_times["scatter_launches"] else "fused"
    assert ran == planned, (ran, planned)
    tr = scene.gpu_traits()
    n_tris = scene.data().tri_verts.shape[0]
    info = {"organisation": ran, "flat_top": bool(tr & _cabi.MTR_TRAIT_FLAT_TOP), "one_rect_emitter": bool(tr & _cabi.MTR_TRAIT_ONE_RECT_EMITTER),
            "no_lobes": bool(tr & _cabi.MTR_TRAIT_NO_LOBES), "diffuse": bool(tr & _cabi.MTR_TRAIT_DIFFUSE),
            "tables": "hbm" if n_tris * GC.TSHADE_BYTES > 64 * 1024 else "lds", "n_tris": int(n_tris)}
    return np.array(s), np.array(t), info


def _steady_case(scene, D, rho=RHO, le=LE):
    s, t, info = gpu_film(scene)
    out = {"info": info, "steady": verdict(pixels(s), radiance(D, rho, le), neighbours(D, rho, le))}
    if D > 0:                # the film window holds every path: the transient film summed over time is the steady image
        out["time_sum"] = verdict(pixels(t.astype(np.float64).sum(2)), radiance(D, rho, le), neighbours(D, rho, le))
    return out


def gpu_orders(org):
    """family 1 in one organisation: D = 1 exactly, the orders and their pixelwise differences at one seed, roulette"""
    kw = ORGANISATIONS[org]
    out, prev = {"cases": {}}, None
    for D in (1, 2, 3, 4, 6):
        s, t, info = gpu_film(room(D, D + 1, GPU_SIZE, **kw))
        ts = t.astype(np.float64).sum(2)
        if D == 1:
            e = radiance(1)
            out["d1_max_rel"] = float(np.max(np.abs(s.astype(np.float64) - e) / e))
            out["d1_time_sum_max_rel"] = float(np.max(np.abs(ts - e) / e))
        else:
            out["cases"][f"D{D}"] = verdict(pixels(s), radiance(D), neighbours(D))
            out["cases"][f"D{D}_time_sum"] = verdict(pixels(ts), radiance(D), neighbours(D))
        if prev is not None and D == prev[0] + 1:
            term = np.asarray(LE) * np.asarray(RHO) ** (D - 1)
            out["cases"][f"D{D}-D{D - 1}"] = verdict(pixels(s.astype(np.float64) - prev[1]), term, [term * r for r in (np.asarray(RHO), 1.0 / np.asarray(RHO))])
        prev = (D, s.astype(np.float64))
        out["info"] = info
    for name, (D, rr) in {"D6_rr2": (6, 2), "inf_rr3": (-1, 3)}.items():
        c = _steady_case(room(D, rr, GPU_SIZE, **kw), D)
        assert c["info"] == out["info"]
        out["cases"][name] = c["steady"]
        if "time_sum" in c:
            out["cases"][name + "_time_sum"] = c["time_sum"]
    return out


def gpu_inclusions(org):
    return {name: _steady_case(room(-1, 3, GPU_SIZE, **INCLUSIONS[name](), **ORGANISATIONS[org]), -1) for name in INCLUSIONS}


def gpu_mesh(which, org):
    import scene_class_cases as SC
    n, mixed = {"small": (MESH_SMALL, False), "large": (MESH_LARGE, False), "mixed": (MESH_SMALL, True)}[which]
    scene = mesh_room(_tmp(), n, size=GPU_SIZE, mixed=mixed, **({} if org == "auto" else ORGANISATIONS[org]))
    out = _steady_case(scene, -1)
    out["auto"] = SC.planned_mode(scene, GPU_SIZE[1])
    return out


def gpu_extended(which, org):
    scene = bitmap_room(_tmp(), size=GPU_SIZE, extra={"far": far_rough_conductor()} if which == "lobes" else None, **ORGANISATIONS[org])
    out = _steady_case(scene, -1)
    import __graft_entry__ as g
    from scene_class_cases import host_class
    out["needs_ext"] = bool(host_class(C.CDLL(g.build_host_harness()), scene)[1])
    return out


def stokes_verdicts(t4, s4=None):
    """the time-summed Stokes film (H, W, T, 4) — every sample of a polarized render carries weight 1, so the sum divided by the
    weight is the sum itself, as the raw film has it (sample_scale = 1 / spp) —: S0 -> L_inf, S1..S3 -> 0 on the scale of L_inf"""
    linf = float(radiance(-1, POL_RHO, POL_LE)[0])
    S = np.asarray(t4, np.float64).sum(2).reshape(-1, 4)
    return {"S0": verdict(S[:, :1], [linf], neighbours(-1, POL_RHO, POL_LE)), "S123": verdict(S[:, 1:], np.zeros(3), scale=np.full(3, linf))}


def polarized_room(glass, size):
    # the film window [0, 64): what a path adds after 64 units of length is missing from the time sum.  No segment is longer than
    # the room's diagonal 5.39, so that is beyond the 11th bounce: under 0.6^11 = 0.4 % of L_inf even if every segment were a
    # diagonal, and 1e-7 of it at the room's mean chord 4 V / S = 1.85 (35 bounces)
    return room(-1, 3, size, rho=POL_RHO, le=POL_LE, variant="llvm_ad_mono_polarized",
                extra={"inner": glass_cube()} if glass else None)


def gpu_polarized(glass):
    import torch
    scene = polarized_room(glass, GPU_SIZE)
    integ = scene.integrator()
    integ.collect_stats = True
    spp = scene.sensors()[0].sampler().sample_count()
    s, t = integ.render(scene, seed=0, spp=spp)
    torch.cuda.synchronize()
    planned = integ.resolved_mode(scene, scene.sensors()[0], spp)           # (mtr_render_plan, the film prepared)
    out = stokes_verdicts(np.array(t))
    out["steady"] = verdict(pixels(np.array(s)), radiance(-1, POL_RHO, POL_LE), neighbours(-1, POL_RHO, POL_LE))
    out["info"] = {"organisation": planned, "scatter_launches": int(integ.total_times["scatter_launches"])}
    return out


def _sum_keys(scene, g):
    """(sum over the wall materials of d / d rho, sum over the emitters of d / d Le) of render_backward's dictionary"""
    keys = scene.grad_keys()
    gm = sum(g[k] for k, (kind, _) in keys.items() if kind == "material")
    ge = sum(g[k] for k, (kind, _) in keys.items() if kind == "emitter")
    return gm, ge


def grad_verdicts(gm, ge, D):
    """K seeds of (sum d / d rho, sum d / d Le), each (K, 3)"""
    drho, dle = d_radiance_d_rho(D), d_radiance_d_le(D)
    return {"d_rho": verdict(gm, drho, [d_radiance_d_rho(x) for x in wrong_orders(D)]),
            "d_le": verdict(ge, dle, [d_radiance_d_le(x) for x in wrong_orders(D)])}


def gpu_grad(which):
    """mtr_render_grad over K seeds: the rectangle room (lds) at D = 4 and at L_inf, the large mesh room (hbm) at L_inf"""
    import grad_gpu_cases as GC
    D, rr = (4, 5) if which == "lds_D4" else (-1, 3)
    scene = mesh_room(_tmp(), MESH_LARGE, D, rr, grad_size(D)) if which == "hbm_inf" else room(D, rr, grad_size(D))
    g_s, g_t = mean_upstream(scene)
    gm, ge = [], []
    for seed in range(GRAD_SEEDS):
        g, _ = GC.gpu_grads(scene, g_s, g_t, seed=seed, spp=grad_size(D)[1])
        a, b = _sum_keys(scene, g)
        gm.append(a)
        ge.append(b)
    out = grad_verdicts(np.array(gm), np.array(ge), D)
    out["instantiation"] = GC.instantiation(scene)
    return out


def gpu_grad_tex():
    """mtr_render_grad_tex on the constant bitmap: the texel gradients summed are the walls' d / d rho"""
    import grad_gpu_cases as GC
    import grad_tex_gpu_cases as XC
    import torch
    scene = bitmap_room(_tmp(), 4, 5, GRAD_SIZE)
    XC.upload(scene)
    p = XC.tex_params(scene)
    g_s, g_t = mean_upstream(scene)
    integ = scene.integrator()
    gm, ge = [], []
    for seed in range(GRAD_SEEDS):
        g = integ.render_backward(scene, p, grad_in=(torch.from_numpy(g_s).cuda(), torch.from_numpy(g_t).cuda()), seed=seed, spp=GRAD_SIZE[1])
        torch.cuda.synchronize()
        g = {k: v.double().cpu().numpy() for k, v in g.items()}
        tex = {i: k for k, i in scene.texture_keys().items() if k in g}
        gm.append(sum(g[k].sum(axis=(0, 1)) for k in tex.values()))
        ge.append(_sum_keys(scene, g)[1])
    out = grad_verdicts(np.array(gm), np.array(ge), 4)
    out.update(instantiation=GC.instantiation(scene), tier=scene.grad_tex_tier(), n_textures=len(scene.data().textures))
    return out


def unit_tangents(scene, what):
    import test_fwd as F
    mats, ems = wall_indices(scene)
    tan = F.Tangents(scene)
    if what == "rho":
        tan.mats[mats] = 1.0
    else:
        tan.ems[ems] = 1.0
    return tan


def gpu_fwd(which):
    """mtr_render_fwd: the tangent image for d rho = 1 on every wall, then d Le = 1"""
    import fwd_gpu_cases as FC
    import grad_gpu_cases as GC
    D, rr = (4, 5) if which == "lds_D4" else (-1, 3)
    size = FWD_SIZE_INF_GPU if D < 0 else GPU_SIZE
    scene = mesh_room(_tmp(), MESH_LARGE, D, rr, size) if which == "hbm_inf" else room(D, rr, size)
    out = {"instantiation": GC.instantiation(scene), "tier": FC.tier(scene, size[1])}
    for what, e, f in (("rho", d_radiance_d_rho(D), d_radiance_d_rho), ("le", d_radiance_d_le(D), d_radiance_d_le)):
        _, s, _ = FC.gpu_fwd(scene, unit_tangents(scene, what), seed=0, spp=size[1])
        out["d_" + what] = verdict(pixels(s), e, [f(x) for x in wrong_orders(D)])
    return out


def gpu_cameras(org):
    """the D = 2 room through every camera configuration against the oracle at the same seed"""
    from conftest import rel_l2
    out = {}
    for name in CAMERAS:
        scene = camera_room(name, **ORGANISATIONS[org])
        s, t, info = gpu_film(scene)
        s3, t3 = oracle_film(scene)
        out[name] = {"rel_s": rel_l2(s, s3), "rel_t": rel_l2(t, t3), "scale": float(np.abs(t3).max()), "info": info}
    return out


if __name__ == "__main__":
    case, args = sys.argv[1], sys.argv[2:]
    import torch
    torch.cuda.set_device(0)
    out = {"orders": gpu_orders, "inclusions": gpu_inclusions, "mesh": gpu_mesh, "extended": gpu_extended,
           "polarized": lambda g: gpu_polarized(g == "glass"), "grad": gpu_grad, "grad_tex": gpu_grad_tex, "fwd": gpu_fwd,
           "cameras": gpu_cameras}[case](*args)
    print(json.dumps(out))
