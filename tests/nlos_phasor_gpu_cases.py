"""One GPU step of tests/test_gpu_nlos_phasor.py, run in a child process of its own (the test gives each step a time limit):
``python tests/nlos_phasor_gpu_cases.py <case>`` prints one JSON line."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from conftest import make_nlos, rel_l2  # noqa: E402
import test_nlos_phasor as NP  # noqa: E402

MTR_ERR_UNSUPPORTED = -5
MODES = {"auto": 0, "fused": 1, "wavefront": 2}


def mono():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_mono")


def camera_scene(F=15, res=(6, 5), spp=32):
    """conftest.make_nlos_camera's scene — transient_nlos_path behind a perspective camera, no nlos_capture_meter — with a
    phasor_hdr_film (make_nlos_camera takes no film)"""
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant("llvm_ad_rgb")
    pose = T().look_at(origin=[-2.0, 0.0, 2.0], target=[0.0, 0.0, 0.0], up=[0, 1, 0])
    white = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.9, 0.9, 0.9]}}}
    film = dict(NP.FILMS[F], width=res[0], height=res[1], start_opl=1.0, rfilter={"type": "box"})
    return mi.load_dict({
        "type": "scene",
        "integrator": {"type": "transient_nlos_path", "max_depth": 5, "nlos_laser_sampling": True,
                       "nlos_hidden_geometry_sampling": True, "capture_type": "single", "temporal_filter": "box"},
        "sensor": {"type": "perspective", "fov": 40.0, "fov_axis": "x", "near_clip": 0.1, "far_clip": 100.0, "to_world": pose,
                   "sampler": {"type": "independent", "sample_count": spp}, "film": film},
        "laser": {"type": "projector", "to_world": pose, "fov": 0.2, "irradiance": {"type": "rgb", "value": [100.0, 100.0, 100.0]}},
        "wall": {"type": "rectangle", "bsdf": white},
        "hidden": {"type": "rectangle", "to_world": T().translate([0.5, 0, 1]).rotate([0, 1, 0], 180).scale(0.5), "bsdf": white},
    })


def textured_hidden():
    """a 4 x 3 bitmap on the hidden quad's reflectance: the extended shading code without lobes"""
    from PIL import Image
    path = os.path.join(tempfile.mkdtemp(prefix="nlos_phasor_"), "albedo.png")
    Image.fromarray(np.random.default_rng(4).integers(40, 250, (3, 4, 3), dtype=np.uint8)).save(path)
    return {"type": "diffuse", "reflectance": {"type": "bitmap", "filename": path}}


SCENES = {
    "confocal_z": lambda F: NP.phasor_nlos("confocal", F, hidden="z"),
    "single_quad": lambda F: NP.phasor_nlos("single", F),
    "meter_first_last": lambda F: NP.phasor_nlos("confocal", F, account_first_and_last_bounces=True),
    "camera": camera_scene,
    "rough_hidden": lambda F: NP.phasor_nlos("confocal", F, hidden_bsdf=dict(NP.ROUGH)),
    "textured_hidden": lambda F: NP.phasor_nlos("confocal", F, hidden_bsdf=textured_hidden()),
    "row_reuse": lambda F: NP.phasor_nlos("confocal", F, sx=128, sy=96, spp=2, hidden="z"),
}


def reference(scene, spp, seed):
    from oracle import oracle
    oracle.build()
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)
    raw, s4, cnt = oracle.render(sd, p, use_bvh=True)
    ph, s3 = oracle.develop(sd.film, raw, s4)
    return ph, raw, s3, cnt


def gpu(scene, spp, seed, mode, through_mi=False):
    """(steady, phasors, raw, counters, organisation that ran) of one render; a refused mode: the error's text"""
    import torch
    import mitransient_amd.mi as mi
    from mitransient_amd._cabi import MitransientAMDError
    integ = scene.integrator()
    integ.mode = MODES[mode]
    integ.collect_stats = True
    try:
        steady, phasors = mi.render(scene, spp=spp, seed=seed) if through_mi else integ.render(scene, seed=seed, spp=spp)
    except MitransientAMDError as e:
        return {"refused": str(e)}
    torch.cuda.synchronize()
    film = scene.sensors()[0].film()
    _, raw = film.develop(raw=True)
    ran = integ.resolved_mode(scene, scene.sensors()[0], spp)           # (mtr_render_plan, the film prepared)
    return {"steady": np.array(steady), "phasors": np.array(phasors), "raw": np.array(raw), "counters": dict(integ.last_counters),
            "ran": ran}


def compare(got, ref, F, shape):
    ph, raw, s3, cnt = ref
    H, W = shape
    out = {"ran": got["ran"],
           "shapes_ok": bool(got["phasors"].shape == (H, W, F, 2) and got["steady"].shape == (H, W, 1) and got["raw"].shape == (H, W, 2 * F + 1)),
           "weight_zero": bool(not got["raw"][..., -1].any()),
           "rel_phasors": rel_l2(got["phasors"], ph), "rel_raw": rel_l2(got["raw"], raw), "rel_steady": rel_l2(got["steady"][..., 0], s3[..., 0]),
           "scale": float(np.abs(ph).max()), "lit": int(np.count_nonzero(s3[..., 0])),
           "counters_equal": bool(all(got["counters"][k] == cnt[k] for k in NP.COUNTERS)),
           "counters": {k: [int(got["counters"][k]), int(cnt[k])] for k in NP.COUNTERS},
           "splats_overflow": int(got["counters"]["splats_overflow"])}
    return out


def parity(name, F, modes=("auto", "fused", "wavefront"), seed=3):
    """the scene in each requested organisation against ONE oracle render"""
    scene = SCENES[name](F)
    mono()
    film = scene.sensors()[0].film()
    W, H = film.size()
    spp = scene.sensors()[0].sampler().sample_count()
    ref = reference(scene, spp, seed)
    out = {}
    for i, m in enumerate(modes):
        got = gpu(scene, spp, seed, m, through_mi=(i == 0))
        out[m] = got if "refused" in got else compare(got, ref, F, (H, W))
    return out


def zero_frequency():
    """F = 15 from f = 0: Im[f = 0] is exactly 0 and Re[f = 0] the GPU's own steady image (another accumulator: not bit-equal)"""
    out = {}
    for m in ("fused", "wavefront"):
        scene = SCENES["confocal_z"](15)
        mono()
        assert float(scene.sensors()[0].film().frequencies[0]) == 0.0
        got = gpu(scene, 32, 5, m)
        ph, s = got["phasors"], got["steady"][..., 0]
        out[m] = {"ran": got["ran"], "im_zero": bool(not ph[..., 0, 1].any()), "rel_re_steady": rel_l2(ph[..., 0, 0], s),
                  "lit": int(np.count_nonzero(s))}
    return out


def film_types():
    """a transient-film NLOS render (amd_deterministic), a phasor one, the transient one again — one context"""
    import torch
    out = {}
    for m in ("fused", "wavefront"):
        a = make_nlos(sx=6, sy=5, capture="confocal", hidden="z", spp=32, amd_deterministic=True)
        b = NP.phasor_nlos("confocal", 151, hidden="z")
        mono()
        for s in (a, b):
            s.integrator().mode = MODES[m]
        s0, t0 = a.integrator().render(a, seed=1, spp=32)
        t0, s0 = np.array(t0), np.array(s0)
        _, ph = b.integrator().render(b, seed=1, spp=32)
        torch.cuda.synchronize()
        s1, t1 = a.integrator().render(a, seed=1, spp=32)
        t1, s1 = np.array(t1), np.array(s1)
        out[m] = {"equal_t": bool(np.array_equal(t0, t1)), "equal_s": bool(np.array_equal(s0, s1)),
                  "rel_t": rel_l2(t1, t0), "rel_s": rel_l2(s1, s0), "nonzero": int(np.count_nonzero(t0)),
                  "phasor_nonzero": int(np.count_nonzero(np.array(ph)))}
    return out


def abi_refusals():
    """mtr_render itself: an Exhaustive capture whose film is swapped for a phasor one, and MTR_FLAG_POLARIZED on the NLOS tier
    (transient and phasor film) — MTR_ERR_UNSUPPORTED, the sentinel-filled tensors untouched"""
    import torch
    from mitransient_amd import _cabi
    from mitransient_amd.runtime import get_context
    from mitransient_amd.scene import film_desc_from
    from test_nlos import exhaustive_scene
    ctx = get_context()

    def render(handle, prm, n_floats, npix):
        t = torch.full((n_floats,), -7.0, device="cuda")
        s = torch.full((npix * 4,), -7.0, device="cuda")
        rc = ctx.lib.mtr_render(handle, C.byref(prm), C.c_void_p(t.data_ptr()), C.c_void_p(s.data_ptr()), None, None)
        torch.cuda.synchronize()
        msg = ctx.lib.mtr_last_error(ctx.handle)
        return {"status": int(rc), "untouched": bool(torch.all(t == -7.0).item() and torch.all(s == -7.0).item()),
                "message": msg.decode() if isinstance(msg, bytes) else str(msg)}

    out = {}
    ex = exhaustive_scene()
    mono()
    h = ex.gpu_handle(ctx, 0)
    ph_film = NP.phasor_nlos("confocal", 15, sx=4, sy=4).sensors()[0].film()
    mono()
    fd = film_desc_from(ph_film)
    ctx.check(ctx.lib.mtr_scene_set_film(h, C.byref(fd)), "mtr_scene_set_film")
    prm = ex.integrator().render_params(ph_film, 0, 4)
    out["exhaustive"] = render(h, prm, 4 * 4 * 31, 16)
    for name, scene in (("polarized_transient", make_nlos(sx=4, sy=4)), ("polarized_phasor", NP.phasor_nlos("confocal", 15, sx=4, sy=4))):
        mono()
        film = scene.sensors()[0].film()
        prm = scene.integrator().render_params(film, 0, 4)
        prm.flags |= _cabi.MTR_FLAG_POLARIZED
        f = scene.data().film
        per_pixel = 2 * f.n_frequencies + 1 if f.n_frequencies else f.temporal_bins * 4
        out[name] = render(scene.gpu_handle(ctx, 0), prm, 16 * per_pixel, 16)
    out["distributed"] = distributed_refusal()
    return out


def distributed_refusal():
    """DistributedRenderer with a faked world of two ranks: the phasor refusal, before any rendering"""
    import torch.distributed as dist
    from mitransient_amd.distributed import DistributedRenderer
    scene = NP.phasor_nlos("confocal", 15)
    mono()
    r = DistributedRenderer(scene)
    orig = dist.is_initialized, dist.get_world_size, dist.get_rank
    dist.is_initialized, dist.get_world_size, dist.get_rank = (lambda: True), (lambda group=None: 2), (lambda group=None: 0)
    try:
        r.render(spp=4)
    except NotImplementedError as e:
        return str(e)
    finally:
        dist.is_initialized, dist.get_world_size, dist.get_rank = orig
    return ""


if __name__ == "__main__":
    case = sys.argv[1].split(":")
    import torch
    torch.cuda.set_device(0)
    if case[0] == "parity":
        out = parity(case[1], int(case[2]), tuple(case[3].split(",")) if len(case) > 3 else ("auto", "fused", "wavefront"))
    else:
        out = {"zero_frequency": zero_frequency, "film_types": film_types, "abi_refusals": abi_refusals}[case[0]]()
    print(json.dumps(out))
