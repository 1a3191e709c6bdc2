"""Reverse-mode gradients of transient_path (mtr_render_grad, mtr_grad.h): the host build of the gradient arithmetic against
finite differences of the unchanged CPU oracle at the same seed, on diffuse-only Cornell-class scenes with rr_depth >= max_depth
(the seeded estimator is then a polynomial in the albedos of degree < max_depth, which the five-point stencil differentiates
exactly), and the Python surface (mi.traverse keys, params.update(), the refusals).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_grad():
    """tests/host_grad.cpp with the flags of build_host_harness() (__graft_entry__.py)"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_grad.so")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "host_grad.cpp"), os.path.join(csrc, "mtr_scene_host.cpp"), os.path.join(csrc, "mtr_bvh.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mtr_core.h", "mtr_grad.h", "mtr_scene_host.h", "mtr_bvh.h", "mtr_knobs.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-DMTR_EXPERIMENTS", "-o", tmp] + srcs, check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hg():
    return C.CDLL(build_host_grad())


def _mi():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    return mi


def angular_spot():
    """a second, `angulararea` luminaire on the Cornell box's back wall"""
    from mitransient_amd.transform import ScalarTransform4f as T
    return dict(type="rectangle", to_world=T().translate([0.4, 0.3, -0.99]).scale([0.2, 0.2, 0.2]),
                bsdf=dict(type="diffuse", reflectance=dict(type="rgb", value=[0.3, 0.4, 0.5])),
                emitter=dict(type="angulararea", cutoff_angle=60.0, beam_width=30.0,
                             radiance=dict(type="rgb", value=[2.0, 3.0, 0.0])))


def cornell(res=16, bins=32, max_depth=4, start_opl=3.5, bin_width=0.1, crop=None, angular=False, share=False, rr_depth=None,
            blue=None, **integ):
    """cornell_box() at a small size, rr_depth > max_depth unless `rr_depth` says otherwise; angular: a second, `angulararea`
    luminaire on the back wall; blue: the blue channel of every reflectance (test_grad_general.py: 1.0 keeps rr_prob constant)"""
    import mitransient_amd as mitr
    mi = _mi()
    d = mitr.cornell_box()
    d["integrator"].update(max_depth=max_depth, rr_depth=max(max_depth, 1) + 1 if rr_depth is None else rr_depth, **integ)
    d["sensor"]["film"].update(width=res, height=res, temporal_bins=bins, start_opl=start_opl, bin_width_opl=bin_width)
    if crop is not None:
        d["sensor"]["film"].update(crop_width=crop[0], crop_height=crop[1], crop_offset_x=crop[2], crop_offset_y=crop[3])
    if blue is not None:
        for name in ("white", "red", "green"):
            refl = d[name]["reflectance"]
            refl["value"] = list(refl["value"][:2]) + [blue]
    if angular:
        d["spot"] = angular_spot()
    if share:      # one inline BSDF dictionary on two shapes: each of their keys must own a record
        shared = dict(type="twosided", bsdf=dict(type="diffuse", reflectance=dict(type="rgb", value=[0.6, 0.5, 0.4])))
        d["floor"]["bsdf"] = shared
        d["back"]["bsdf"] = shared
    return mi.load_dict(d)


def render_params(scene, seed=3, spp=8):
    integ = scene.integrator()
    return integ.render_params(scene.sensors()[0].film(), seed, spp)


def oracle_loss(scene, params, g_s, g_t):
    """sum g_s . steady + sum g_t . transient of the oracle's developed tensors, in f64"""
    from oracle import oracle
    sd = scene.data()
    t4, s4, _ = oracle.render(sd, params, use_bvh=True)
    t3, s3 = oracle.develop(sd.film, t4, s4)
    return float(np.sum(g_s.astype(np.float64) * s3) + np.sum(g_t.astype(np.float64) * t3)), s3, t3


def host_grad(hg, scene, params, g_s, g_t):
    """the host build's (grad_materials, grad_emitters), f64; g_s (crop_h, crop_w, 3) goes to the accumulator layout"""
    sd = scene.data()
    f = sd.film
    gs_full = np.zeros((f.height, f.width, 3), np.float32)
    gs_full[:g_s.shape[0], :g_s.shape[1]] = g_s
    gt = np.ascontiguousarray(g_t, dtype=np.float32)
    gm = np.zeros((max(1, sd.n_materials), 3))
    ge = np.zeros((max(1, sd.n_emitters), 3))
    d = sd.desc()
    dp = C.POINTER(C.c_double)
    fp = C.POINTER(C.c_float)
    rc = hg.hg_render_grad(C.byref(d), C.byref(params), gs_full.ctypes.data_as(fp), gt.ctypes.data_as(fp),
                           gm.ctypes.data_as(dp), ge.ctypes.data_as(dp))
    assert rc == 0
    return gm[:sd.n_materials], ge[:sd.n_emitters]


def upstream(scene, kind, seed=1):
    """(g_s, g_t) of the three shapes the tests use: random both, one bin alone, steady alone"""
    f = scene.data().film
    rng = np.random.default_rng(seed)
    g_s = rng.standard_normal((f.crop_height, f.crop_width, 3)).astype(np.float32)
    g_t = rng.standard_normal((f.height, f.width, f.temporal_bins, 3)).astype(np.float32)
    if kind == "one_bin":
        g_s[:] = 0
        keep = g_t[:, :, f.temporal_bins // 3].copy()
        g_t[:] = 0
        g_t[:, :, f.temporal_bins // 3] = keep
    elif kind == "steady":
        g_t[:] = 0
    return g_s, g_t


def fd_material(scene, params, g_s, g_t, m, k, wide=False):
    """five-point stencil of the oracle's loss in channel k of material m.  The loss is a polynomial of degree < max_depth <= 5
    in the albedo, so the stencil is exact for every step; the step is a / 4 rounded down to a power of two (every abscissa
    exact in f32) rather than a / 64: the oracle sums in f32, and its rounding noise over a / 64 is up to 5e-4 of the gradient
    for the red wall's 0.043 channel, against 1e-5 over a / 4.
    wide (test_grad_general.py): the derivative at a of the quartic fitted by least squares to the loss at 16 abscissae from
    a / 8 to a + 1 / 4 instead — as exact for the same polynomial, all abscissae positive (with a negative reflectance the oracle's
    loss leaves the polynomial), and the rounding noise of a small channel is spread over a span that does not shrink with a"""
    sd = scene.data()
    a = float(sd.materials[m].a[k])
    if wide:
        xs = np.linspace(a / 8, a + 0.25, 16).astype(np.float32).astype(np.float64)
        vals = []
        for x in xs:
            sd.materials[m].a[k] = x
            vals.append(oracle_loss(scene, params, g_s, g_t)[0])
        sd.materials[m].a[k] = a
        span = xs[-1] - xs[0]
        return float(np.polyder(np.poly1d(np.polyfit((xs - a) / span, vals, 4)))(0.0) / span)
    h = 2.0 ** np.floor(np.log2(a / 4))
    vals = []
    for j in (-2, -1, 1, 2):
        sd.materials[m].a[k] = a + j * h
        vals.append(oracle_loss(scene, params, g_s, g_t)[0])
    sd.materials[m].a[k] = a
    return (vals[0] - 8 * vals[1] + 8 * vals[2] - vals[3]) / (12 * h)


def within(g, fd, tol):
    """the comparison of check_materials: every channel of a material within tol of the largest finite difference"""
    return bool(np.abs(g - fd).max() <= tol * max(np.abs(fd).max(), 1e-12))


def check_materials(hg, scene, g_s, g_t, mats=None, tol=1e-4, chans=(0, 1, 2), gm=None, report=None, wide=False):
    """gm: the gradients to check (the host build's when None); report: a dictionary that receives {m: (gradient, finite
    differences, error relative to the largest finite difference)} over the channels `chans`"""
    params = render_params(scene)
    if gm is None:
        gm, _ = host_grad(hg, scene, params, g_s, g_t)
    sd = scene.data()
    mats = range(sd.n_materials) if mats is None else mats
    chans = list(chans)
    for m in mats:
        fd = np.array([fd_material(scene, params, g_s, g_t, m, k, wide) for k in chans])
        if report is not None:
            report[m] = (gm[m][chans], fd, float(np.abs(gm[m][chans] - fd).max() / max(np.abs(fd).max(), 1e-12)))
        assert within(gm[m][chans], fd, tol), (m, gm[m], fd)
    return gm


@pytest.mark.parametrize("kind", ["random", "one_bin", "steady"])
def test_albedo_gradients_match_finite_differences(hg, kind):
    scene = cornell()
    g_s, g_t = upstream(scene, kind)
    gm = check_materials(hg, scene, g_s, g_t)
    assert np.all(np.isfinite(gm)) and np.abs(gm).max() > 0


@pytest.mark.parametrize("case", ["camera_unwarp", "discard_direct_light", "hide_emitters", "beyond_last_bin", "crop"])
def test_albedo_gradients_integrator_and_film_cases(hg, case):
    kw = {}
    if case in ("camera_unwarp", "discard_direct_light", "hide_emitters"):
        kw[case] = True
    if case == "camera_unwarp":
        kw["start_opl"] = 0.0
    if case == "beyond_last_bin":
        kw.update(bins=8)               # most contributions land beyond the last bin: they reach the steady image only
    if case == "crop":
        kw.update(crop=(10, 7, 3, 5))
    scene = cornell(**kw)
    g_s, g_t = upstream(scene, "random")
    check_materials(hg, scene, g_s, g_t)


GRAD_REC = np.dtype([("kind", "u4"), ("idx", "u4"), ("flag", "u4"), ("pad", "u4"), ("dist", "f4"), ("c", "f4", (3,))])


def host_records(hg, scene, params, g_s, g_t):
    """the host build's gradients and the records of every lane's replay walk (tests/host_grad.cpp: GradRec)"""
    sd = scene.data()
    f = sd.film
    gs_full = np.zeros((f.height, f.width, 3), np.float32)
    gs_full[:g_s.shape[0], :g_s.shape[1]] = g_s
    gt = np.ascontiguousarray(g_t, dtype=np.float32)
    gm = np.zeros((max(1, sd.n_materials), 3))
    ge = np.zeros((max(1, sd.n_emitters), 3))
    n = C.c_uint64(0)
    d = sd.desc()
    fp = C.POINTER(C.c_float)
    dp = C.POINTER(C.c_double)
    assert hg.hg_grad_records(C.byref(d), C.byref(params), gs_full.ctypes.data_as(fp), gt.ctypes.data_as(fp),
                              gm.ctypes.data_as(dp), ge.ctypes.data_as(dp), C.byref(n)) == 0
    rec = np.zeros(int(n.value), GRAD_REC)
    hg.hg_grad_records_copy(rec.ctypes.data_as(C.c_void_p))
    return gm[:sd.n_materials], ge[:sd.n_emitters], rec, gs_full


def reference_reading(scene, params, rec, gs_full, g_t):
    """transientpath.py:284-299's reading, computed from the replay's records: delta L is read ONCE per vertex, at the vertex's
    own distance, and applied to its emission, to its emitter-sampling term and to every later term (the material gradient of a
    diffuse vertex is delta L (.) the remaining radiance / albedo)"""
    sd = scene.data()
    f = sd.film
    scale = np.float64(np.float32(1.0 / params.spp_total))
    rad = np.array([[sd.emitters[e].radiance[k] for k in range(3)] for e in range(sd.n_emitters)], np.float64)
    alb = np.array([[sd.materials[m].a[k] for k in range(3)] for m in range(sd.n_materials)], np.float64)
    diffuse = [sd.materials[m].type == 0 and sd.materials[m].albedo_texture == 0 for m in range(sd.n_materials)]
    gt = g_t.reshape(f.height * f.width, f.temporal_bins, 3).astype(np.float64)
    gs = gs_full.reshape(-1, 3).astype(np.float64)
    gm = np.zeros((sd.n_materials, 3))
    ge = np.zeros((sd.n_emitters, 3))
    starts = np.flatnonzero(rec["kind"] == 0).tolist() + [len(rec)]
    for a, b in zip(starts[:-1], starts[1:]):
        lane = rec[a + 1:b]
        pix = int(rec[a]["idx"])
        full = [np.asarray(r["c"], np.float64) * rad[r["idx"]] if r["kind"] >= 2 else None for r in lane]
        dL = None
        for j, r in enumerate(lane):
            if r["kind"] == 1:
                bin_ = int(np.floor((np.float32(r["dist"]) - np.float32(f.start_opl)) / np.float32(f.bin_width_opl)))
                dL = gs[pix] * scale + (gt[pix, bin_] * scale if 0 <= bin_ < f.temporal_bins else 0.0)
                if r["flag"] and diffuse[r["idx"]]:
                    # the remaining radiance: this vertex's emitter-sampling term and every later term, its emission excluded
                    rest = [full[i] for i in range(j + 1, len(lane)) if full[i] is not None and not (i == j + 1 and lane[i]["kind"] == 2)]
                    if rest:
                        m = r["idx"]
                        gm[m] += np.where(alb[m] != 0, dL * np.sum(rest, axis=0) / np.where(alb[m] != 0, alb[m], 1), 0)
            else:
                ge[r["idx"]] += dL * np.asarray(r["c"], np.float64)
    return gm, ge


def test_exact_gradient_is_the_references_reading_when_g_t_is_constant_in_time(hg):
    """with g_t constant over time and every term inside the film's window, weighting each term at its own bin (this project)
    and reading delta L once at the vertex distance (the reference) are the same gradient; with a random g_t they are not"""
    scene = cornell(bins=64, start_opl=0.0, bin_width=0.5, angular=True)       # the window [0, 32) holds every term of max_depth 4
    params = render_params(scene)
    g_s, g_t = upstream(scene, "random")
    g_t[:] = g_t[:, :, :1]                                                    # constant over time, per pixel and channel
    gm, ge, rec, gs_full = host_records(hg, scene, params, g_s, g_t)
    f = scene.data().film
    terms = rec[rec["kind"] >= 1]
    assert len(terms) > 1000
    assert np.all(terms["dist"] >= f.start_opl) and np.all(terms["dist"] < f.start_opl + f.temporal_bins * f.bin_width_opl * 0.999)
    rm, re_ = reference_reading(scene, params, rec, gs_full, g_t)
    for ours, ref in ((gm, rm), (ge, re_)):
        assert np.abs(ref).max() > 0
        assert np.abs(ours - ref).max() <= 1e-5 * np.abs(ref).max(), (ours, ref)
    # a g_t that varies over time tells the two readings apart: the test can see a difference
    g_s2, g_t2 = upstream(scene, "random", seed=2)
    gm2, ge2, rec2, gs_full2 = host_records(hg, scene, params, g_s2, g_t2)
    rm2, _ = reference_reading(scene, params, rec2, gs_full2, g_t2)
    assert np.abs(gm2 - rm2).max() > 1e-3 * np.abs(rm2).max()


def test_max_depth_one_has_no_albedo_gradient(hg):
    scene = cornell(max_depth=1)
    g_s, g_t = upstream(scene, "random")
    gm, ge = host_grad(hg, scene, render_params(scene), g_s, g_t)
    assert np.all(gm == 0.0)
    assert np.abs(ge).max() > 0


def test_material_at_several_vertices(hg):
    """`white` covers floor, ceiling, back wall and both boxes: most paths meet it at several vertices (n_m(c) > 1)"""
    scene = cornell(max_depth=5)
    g_s, g_t = upstream(scene, "random", seed=5)
    white = scene.grad_keys()["white.reflectance.value"][1]
    check_materials(hg, scene, g_s, g_t, mats=[white])


def emitter_coefficients(scene, params, g_s, g_t):
    """(n_emitters, 3): the oracle's loss with channel k of emitter e at 1 as the scene's only light"""
    sd = scene.data()
    n = sd.n_emitters
    saved = [[float(sd.emitters[e].radiance[k]) for k in range(3)] for e in range(n)]
    ref = np.zeros((n, 3))
    try:
        for e in range(n):
            for k in range(3):
                for e2 in range(n):
                    for k2 in range(3):
                        sd.emitters[e2].radiance[k2] = 1.0 if (e2, k2) == (e, k) else 0.0
                ref[e, k] = oracle_loss(scene, params, g_s, g_t)[0]
    finally:
        for e in range(n):
            for k in range(3):
                sd.emitters[e].radiance[k] = saved[e][k]
    return ref


def test_emitter_gradients_are_the_linear_coefficients(hg):
    """the estimator is linear in each radiance channel: d loss / d L_e[k] is the loss of a render whose only light is
    channel k of emitter e at 1 — two emitters, one of them `angulararea`"""
    scene = cornell(angular=True)
    g_s, g_t = upstream(scene, "random")
    params = render_params(scene)
    _, ge = host_grad(hg, scene, params, g_s, g_t)
    sd = scene.data()
    assert sd.n_emitters == 2 and sd.emitters[1].angular == 1
    ref = emitter_coefficients(scene, params, g_s, g_t)
    for e in range(2):
        for k in range(3):
            assert abs(ge[e, k] - ref[e, k]) <= 1e-5 * max(abs(ref[e, k]), 1e-12) + 1e-9, (e, k, ge[e, k], ref[e, k])
    assert ge[1, 2] != 0.0          # a radiance channel of 0 still has its gradient


def test_zero_albedo_channel_is_finite(hg):
    scene = cornell()
    p = _mi().traverse(scene)
    p["red.reflectance.value"] = [0.57, 0.0, 0.04]
    p.update()
    g_s, g_t = upstream(scene, "random")
    gm, ge = host_grad(hg, scene, render_params(scene), g_s, g_t)
    red = scene.grad_keys()["red.reflectance.value"][1]
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(ge))
    assert gm[red, 1] == 0.0 and gm[red, 0] != 0.0


def test_traverse_keys_and_update():
    mi = _mi()
    scene = cornell(angular=True, share=True)
    p = mi.traverse(scene)
    for k in ("white.reflectance.value", "red.reflectance.value", "green.reflectance.value", "light.emitter.radiance.value",
              "spot.emitter.radiance.value", "spot.bsdf.reflectance.value", "floor.bsdf.brdf_0.reflectance.value",
              "back.bsdf.brdf_0.reflectance.value"):
        assert k in p, k
        assert len(p[k]) == 3
    assert p["red.reflectance.value"] == pytest.approx([0.570068, 0.0430135, 0.0443706])
    assert not scene._data                   # traverse reads the dictionary: nothing is flattened for it
    floor, back = "floor.bsdf.brdf_0.reflectance.value", "back.bsdf.brdf_0.reflectance.value"
    keys = scene.grad_keys()
    assert keys[floor] == keys[back]         # one shared dictionary, one record, until one of its keys is set
    p[floor] = [0.9, 0.8, 0.7]
    p.update()
    keys = scene.grad_keys()
    assert keys[floor] != keys[back]         # ... then each key owns its record
    mats = [v for v in keys.values() if v[0] == "material"]
    assert len(set(mats)) == len(mats)
    sd = scene.data()
    assert list(sd.materials[keys[floor][1]].a) == pytest.approx([0.9, 0.8, 0.7])
    assert list(sd.materials[keys[back][1]].a) == pytest.approx([0.6, 0.5, 0.4])
    import torch
    p["red.reflectance.value"] = np.array([0.25, 0.5, 0.75])
    p["light.emitter.radiance.value"] = torch.tensor([1.0, 2.0, 3.0])
    p["green.reflectance.value"] = [0.1, 0.2, 0.3]
    p.update()
    sd = scene.data()
    assert list(sd.materials[keys["red.reflectance.value"][1]].a) == [0.25, 0.5, 0.75]
    assert list(sd.emitters[keys["light.emitter.radiance.value"][1]].radiance) == [1.0, 2.0, 3.0]
    assert list(sd.materials[keys["green.reflectance.value"][1]].a) == pytest.approx([0.1, 0.2, 0.3])
    assert mi.traverse(scene)["red.reflectance.value"] == [0.25, 0.5, 0.75]


def _refused(scene, params, match):
    integ = scene.integrator()
    with pytest.raises(ValueError, match=match):
        integ.check_grad_(scene, 0, params)


def test_refusals():
    import torch
    mi = _mi()
    scene = cornell()
    p = mi.traverse(scene)
    p["sensor.film.start_opl"] = torch.tensor(3.0, requires_grad=True)
    _refused(scene, p, "not a differentiable parameter")
    with pytest.raises(ValueError, match="not a differentiable parameter"):
        mi.render(scene, p, spp=4)
    with pytest.raises(NotImplementedError):
        scene.integrator().render_forward(scene, p)
    # the seeds of the two phases must differ
    p = mi.traverse(scene)
    p["red.reflectance.value"] = torch.tensor([0.5, 0.1, 0.1], requires_grad=True)
    with pytest.raises(ValueError, match="seed"):
        mi.render(scene, p, seed=7, seed_grad=7, spp=4)
    # a DistributedRenderer
    from mitransient_amd.distributed import DistributedRenderer
    with pytest.raises(ValueError):
        mi.render(scene, p, integrator=object.__new__(DistributedRenderer), spp=4)
    with pytest.raises(ValueError):
        object.__new__(DistributedRenderer).render_backward(scene, p, (None, None))


def test_refusals_of_variants_integrators_and_films():
    import torch
    import mitransient_amd as mitr
    mi = _mi()
    grad = {"red.reflectance.value": torch.tensor([0.5, 0.1, 0.1], requires_grad=True)}
    for v in ("llvm_ad_mono", "llvm_ad_mono_polarized"):
        mi.set_variant(v)
        try:
            scene = mi.load_dict(mitr.cornell_box())
            _refused(scene, grad, "_ad_rgb")
        finally:
            mi.set_variant("llvm_ad_rgb")
    for film_kw, match in (({"type": "phasor_hdr_film"}, "phasor"), ({"exhaustive_scan": True, "laser_scan_width": 2,
                                                                     "laser_scan_height": 2}, "exhaustive_scan")):
        d = mitr.cornell_box()
        d["sensor"]["film"].update(width=8, height=8, temporal_bins=8, **film_kw)
        if film_kw.get("type") == "phasor_hdr_film":
            d["sensor"]["film"].update(wl_mean=0.5, wl_sigma=0.2)
        scene = mi.load_dict(d)
        _refused(scene, grad, match)
    from mitransient_amd.integrators.transientnlospath import TransientNLOSPath
    scene = cornell()
    nlos = object.__new__(TransientNLOSPath)
    with pytest.raises(ValueError, match="transient_nlos_path"):
        TransientNLOSPath.check_grad_(nlos, scene, 0, grad)
