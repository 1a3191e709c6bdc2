"""BASELINE config 4's per-GPU share with the film swapped for a phasor_hdr_film: confocal, 256 x 256, 512 spp, the nlos_Z scene,
temporal_bins=4096, bin_width_opl=0.003, one narrow and one wide band of frequencies — the fused kernel ((Re, Im) rows in LDS)
against the wavefront organisation ((opl, value) records + k_wf_phasor_scatter), alternating, device-event times of mtr_render;
once with the flat-shaded procedural 'Z' (both organisations) and once with config 4's own Z.obj (extended shading: wavefront).
    python tools/nlos_phasor_bench.py [spp] [res] [repeats]
prints one line per (band, organisation): F, the times of every repeat, their median and spread, and the rel-L2 between the two
organisations' phasors."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

# wl_sigma -> F at temporal_bins=4096, bin_width_opl=0.003: 0.9 -> 15, 0.5 -> 27, 0.3 -> 43, 0.03 -> 412
BANDS = {"few": {"wl_mean": 0.05, "wl_sigma": 0.9}, "some": {"wl_mean": 0.05, "wl_sigma": 0.5},
         "narrow": {"wl_mean": 0.05, "wl_sigma": 0.3}, "wide": {"wl_mean": 0.05, "wl_sigma": 0.03}}


def scene_for(band, res, spp, tmp, hidden):
    """config 4's scene with the film swapped.  hidden = "obj": conftest.make_nlos_z's Z.obj through the `obj` plugin (its vertex
    normals select the extended shading code: with a phasor film that is the wavefront organisation alone); "procedural": the
    flat-shaded 'Z' of conftest.make_nlos / tools/nlos_bench.py (plain shading: both organisations)"""
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant("llvm_ad_mono")
    white = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [1.0, 1.0, 1.0]}}
    film = dict(BANDS[band], type="phasor_hdr_film", width=res, height=res, temporal_bins=4096, bin_width_opl=0.003,
                start_opl=1.85, rfilter={"type": "box"})
    relay = mi.load_dict({"type": "rectangle", "bsdf": white,
                          "nlos_sensor": {"type": "nlos_capture_meter", "sampler": {"type": "independent", "sample_count": spp, "seed": 0},
                                          "sensor_origin": [-0.5, 0.0, 0.25], "film": film}})
    laser = mi.load_dict({"type": "projector", "to_world": T().translate([-0.5, 0.0, 0.25]),
                          "irradiance": {"type": "rgb", "value": [1.0, 1.0, 1.0]}, "fov": 0.2})
    d = {"type": "scene", "laser": laser, "relay_wall": relay,
         "integrator": {"type": "transient_nlos_path", "max_depth": -1, "rr_depth": 5, "nlos_laser_sampling": True,
                        "nlos_hidden_geometry_sampling": True, "account_first_and_last_bounces": False,
                        "capture_type": "confocal", "temporal_filter": "box"}}
    if hidden == "obj":
        tris = np.load(os.path.join(ROOT, "tests", "golden", "nlos_Z_geometry.npz"))["tris"]
        lines = [f"v {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}" for v in tris.reshape(-1, 3)]
        lines += [f"f {3 * i + 1} {3 * i + 2} {3 * i + 3}" for i in range(len(tris))]
        obj = os.path.join(tmp, "Z.obj")
        with open(obj, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        d["Z"] = {"type": "obj", "filename": obj, "to_world": T().translate([0.0, 0.0, 1.0]), "bsdf": white}
    else:
        d["z_top"] = {"type": "cube", "to_world": T().translate([0.0, 0.35, 1.0]).scale([0.4, 0.05, 0.004]), "bsdf": white}
        d["z_bot"] = {"type": "cube", "to_world": T().translate([0.0, -0.35, 1.0]).scale([0.4, 0.05, 0.004]), "bsdf": white}
        d["z_diag"] = {"type": "cube", "to_world": T().translate([0.0, 0.0, 1.0]).rotate([0, 0, 1], 40.0).scale([0.5, 0.05, 0.004]), "bsdf": white}
    scene = mi.load_dict(d)
    mitr.nlos.focus_emitter_at_relay_wall_pixel((res / 2, res / 2), relay, laser)
    return scene


def main():
    spp = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    res = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    assert torch.cuda.is_available(), "a timing needs the GPU"
    tmp = tempfile.mkdtemp(prefix="nlos_phasor_bench_")
    from mitransient_amd._cabi import MitransientAMDError
    for hidden in ("procedural", "obj"):
        for band in BANDS:
            scene = scene_for(band, res, spp, tmp, hidden)
            integ = scene.integrator()
            integ.collect_stats = True
            F = len(scene.sensors()[0].film().frequencies)
            times, phasors = {"fused": [], "wavefront": []}, {}
            for r in range(reps + 1):                       # (repeat 0 warms both organisations up)
                for name, mode in (("fused", 1), ("wavefront", 2)):
                    if times[name] is None:
                        continue
                    integ.mode = mode
                    try:
                        _, ph = integ.render(scene, spp=spp, seed=0)
                    except MitransientAMDError as e:        # (the fused mode with extended shading: refused, not timed)
                        print("%s Z, %s band, %s: %s" % (hidden, band, name, e))
                        times[name] = None
                        continue
                    torch.cuda.synchronize()
                    if r:
                        times[name].append(integ.last_times["total_ms"])
                    phasors[name] = np.array(ph, np.float64)
            integ.mode = 0
            auto = integ.resolved_mode(scene, scene.sensors()[0], spp)          # (mtr_render_plan; the film is prepared by now)
            for name in ("fused", "wavefront"):
                if times[name]:
                    t = np.array(times[name])
                    print("%s Z, %s band, F = %d, %dx%d, %d spp, %s: median %.2f ms, min %.2f, max %.2f  [%s]" %
                          (hidden, band, F, res, res, spp, name, np.median(t), t.min(), t.max(), " ".join("%.2f" % x for x in t)))
            rel = float(np.linalg.norm(phasors["fused"] - phasors["wavefront"]) / np.linalg.norm(phasors["wavefront"])) if "fused" in phasors else float("nan")
            print("%s Z, %s band: AUTO resolves to %s; fused vs wavefront phasors rel-L2 %.2e; counters %s" %
                  (hidden, band, auto, rel, integ.last_counters))


if __name__ == "__main__":
    main()
