"""A thin stand-in for the slice of ``import mitsuba as mi`` that mitransient notebooks use
around the transient_path hot path: ``set_variant``, ``load_dict``, ``render``, ``traverse``,
``ScalarTransform4f``, ``ScalarColor3d`` (README.md:154-164 of the reference).

    import mitransient_amd.mi as mi
    mi.set_variant('llvm_ad_rgb')          # accepted; the arithmetic always runs on the MI355X
    import mitransient_amd as mitr
    scene = mi.load_dict(mitr.cornell_box())
    steady, transient = mi.render(scene, spp=1024)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict

from . import _cabi, plugins
from . import variant as _variant_mod
from .scene import Properties, flatten_scene, film_desc_from
from .sensors import IndependentSampler, PerspectiveSensor, RadianceMeter
from .transform import ScalarTransform4f
from .tensor import TensorXf

Transform4f = ScalarTransform4f


def variant():
    return _variant_mod.get()


POLARIZED_VARIANTS = ("llvm_ad_mono_polarized", "cuda_ad_mono_polarized")


def set_variant(*names):
    """The unpolarized ``*_ad_rgb`` variants, and ``*_ad_mono`` (needed by ``phasor_hdr_film``): monochromatic rendering
    = every colour replaced by its luminance, one output channel.  ``llvm_ad_mono_polarized`` / ``cuda_ad_mono_polarized``:
    the same, with polarization tracking (Mueller throughput, Stokes radiance; the wavefront organisation)."""
    for n in names:
        if n in POLARIZED_VARIANTS:
            _variant_mod.set(n)
            return
        if (n.endswith("_rgb") or n.endswith("_mono")) and "polarized" not in n and not n.startswith("scalar"):
            _variant_mod.set(n)
            return
    raise ValueError(f"unsupported variant(s) {names}: mitransient_amd implements the *_ad_rgb / *_ad_mono paths and the "
                     f"polarized {' / '.join(POLARIZED_VARIANTS)} only (no scalar_*, spectral or *_rgb_polarized variants)")


is_monochromatic = _variant_mod.is_monochromatic


def __getattr__(name):
    # ``mi.is_polarized`` reads the variant that is active NOW (a module attribute would freeze it at import time)
    if name == "is_polarized":
        return _variant_mod.is_polarized()
    raise AttributeError(name)


__version__ = "3.7.0-mitransient_amd"       # the Mitsuba generation whose plugin semantics are mirrored (reference: >=3.6,<3.9)


def ScalarPoint3f(*v):
    return [float(x) for x in (v[0] if len(v) == 1 else v)]


Point3f = ScalarPoint3f
Point2f = ScalarPoint2f = ScalarPoint3f        # plain float lists, any length


class util:                                 # namespace, like mitsuba.util
    @staticmethod
    def convert_to_bitmap(data, uint8_srgb=True):
        """``mi.util.convert_to_bitmap``: array -> displayable image (uint8 sRGB by default)"""
        import numpy as np
        from .vis import to_srgb_uint8
        a = np.array(data)
        return to_srgb_uint8(a) if uint8_srgb else a


def ScalarColor3d(*v):
    return [float(x) for x in (v[0] if len(v) == 1 else v)]


ScalarColor3f = ScalarColor3d


_SHAPE_TYPES = ("rectangle", "cube", "obj", "ply", "sphere", "disk", "cylinder")


def _nested(d, pred_dict, pred_obj):
    """the first nested plugin of a dictionary that matches: keys are arbitrary (the notebooks write 'transient_film',
    'nlos_sensor', ...), values are dictionaries or objects that mi.load_dict returned earlier"""
    for v in d.values():
        if isinstance(v, dict) and pred_dict(v):
            return v
        if not isinstance(v, dict) and pred_obj(v):
            return v
    return None


def _make_sensor(sd, shape_obj=None):
    from . import films as _f  # noqa: F401  (registers the film plugins)
    from .films.transient_hdr_film import TransientHDRFilm
    fd = _nested(sd, lambda v: str(v.get("type", "")).endswith("_film") or v.get("type") == "hdrfilm",
                 lambda v: isinstance(v, TransientHDRFilm))
    if fd is None:
        raise ValueError("sensor: a 'film' is required")
    film = fd if isinstance(fd, TransientHDRFilm) else plugins.create_film(fd["type"], Properties(fd["type"], fd))
    smp = sd.get("sampler", {"type": "independent"})
    if smp.get("type") != "independent":
        raise ValueError(f"failed to instantiate unknown plugin of type \"{smp.get('type')}\" (supported samplers: independent)")
    sampler = IndependentSampler(Properties("independent", smp))
    if sd["type"] == "perspective":
        return PerspectiveSensor(sd, film, sampler)
    if sd["type"] == "radiancemeter":
        return RadianceMeter(sd, film, sampler)
    if sd["type"] == "nlos_capture_meter":
        from .sensors.nloscapturemeter import NLOSCaptureMeter
        s = NLOSCaptureMeter(Properties("nlos_capture_meter", sd), film, sampler)
        s.dict_, s.shape_ = sd, shape_obj
        return s
    raise ValueError(f"failed to instantiate unknown plugin of type \"{sd['type']}\" "
                     "(supported sensors: perspective, radiancemeter, nlos_capture_meter)")


def _load_shape(d):
    """a shape dictionary -> Shape object; a nested nlos_capture_meter becomes its sensor"""
    from .shapes import Shape
    from .sensors.nloscapturemeter import NLOSCaptureMeter
    sh = Shape(d)
    for k, v in d.items():
        if isinstance(v, dict) and v.get("type") == "nlos_capture_meter":
            sh.sensor_ = _make_sensor(v, sh)
            sh.sensor_key = k
        elif isinstance(v, NLOSCaptureMeter):              # a sensor object loaded on its own (1-simple-nlos-scenes.ipynb)
            sh.sensor_, sh.sensor_key = v, k
            v.shape_ = sh
    return sh


class Scene:
    def __init__(self, d: Dict[str, Any], base_dir: str = ".", approximate_materials: bool = False, geometry=None):
        self.approximate_materials = approximate_materials
        self.geometry_ = geometry              # pre-flattened triangles + tables (scene.load_geometry), or None
        # differentiable parameters (mi.traverse): one material record per key, and the values set through params.update()
        self.own_materials_ = False
        self.param_values_ = {}
        self.texture_values_ = {}              # {(file, raw): (H, W, 3) f32} texels set through a `.data` key
        from . import integrators as _i, films as _f  # noqa: F401  (registers the plugins)
        from .shapes import Shape
        from .emitters import Projector, _DeltaEmitter, make_delta_emitter
        if d.get("type") != "scene":
            raise ValueError("load_dict(): expected a dictionary with 'type': 'scene'")
        self.base_dir = base_dir
        # objects that were loaded on their own (mi.load_dict(shape) / mi.load_dict(projector)) keep their identity,
        # so that mitransient.nlos.focus_emitter_* edits made later are seen by the render
        self.shape_objs_, self.emitters_, self.sensors_ = {}, [], []
        self.emitter_names_ = []               # the projectors' keys in the scene dictionary (<emitter id>.irradiance.value)
        self.lights_ = {}                      # point / spot emitters by key: the live objects (their records are flattened from them)
        flat = {}
        for k, v in d.items():
            if isinstance(v, Shape):
                self.shape_objs_[k] = v
                flat[k] = v.dict_
            elif isinstance(v, Projector):
                self.emitters_.append(v)
                self.emitter_names_.append(k)
            elif isinstance(v, dict) and v.get("type") == "projector":
                e = Projector(Properties("projector", v))
                e.dict_ = v
                self.emitters_.append(e)
                self.emitter_names_.append(k)
            elif isinstance(v, _DeltaEmitter):                                 # loaded on its own: mi.load_dict(point / spot)
                self.lights_[k] = v
                flat[k] = v.dict_
            elif isinstance(v, dict) and v.get("type") in ("point", "spot"):
                self.lights_[k] = make_delta_emitter(v)
                flat[k] = v
            elif isinstance(v, dict) and v.get("type") in _SHAPE_TYPES:
                self.shape_objs_[k] = _load_shape(v)
                flat[k] = v
            else:
                flat[k] = v
        self.dict_ = flat
        from .integrators.common import TransientADIntegrator
        integ = [v for v in flat.values() if isinstance(v, TransientADIntegrator) or (isinstance(v, dict) and
                 (str(v.get("type", "")).startswith("transient") or v.get("type") in ("path", "direct")))]
        if len(integ) != 1:
            raise ValueError("load_dict(): exactly one integrator is required")
        idict = integ[0]
        self.integrator_ = idict if isinstance(idict, TransientADIntegrator) else \
            plugins.create_integrator(idict["type"], Properties(idict["type"], idict))
        from .integrators.transientnlospath import TransientNLOSPath
        if isinstance(self.integrator_, TransientNLOSPath) and any(
                isinstance(e, dict) and e.get("type") == "angulararea"
                for v in flat.values() if isinstance(v, dict) for e in v.values()):
            # transientnlospath.py:256-260: the NLOS integrator takes exactly one emitter, a projector
            raise ValueError("transient_nlos_path: an angulararea emitter cannot light a NLOS scene (one projector is required)")
        if isinstance(self.integrator_, TransientNLOSPath) and self.lights_:
            raise ValueError(f"transient_nlos_path: a {next(iter(self.lights_.values())).KIND} emitter cannot light a NLOS scene "
                             "(one projector is required)")
        for k, v in flat.items():
            if isinstance(v, dict) and v.get("type") in ("perspective", "radiancemeter"):
                self.sensors_.append(_make_sensor(v))
            elif isinstance(v, RadianceMeter):                                     # loaded on its own: mi.load_dict(radiancemeter)
                self.sensors_.append(v)
        if isinstance(self.integrator_, TransientNLOSPath) and any(isinstance(s, RadianceMeter) for s in self.sensors_):
            raise ValueError("transient_nlos_path: a radiancemeter cannot capture a NLOS scene (use transient_path, or a "
                             "nlos_capture_meter / perspective sensor)")
        self.relay_names_ = {}
        for k, sh in self.shape_objs_.items():
            if sh.sensor() is not None:
                self.sensors_.append(sh.sensor())
                self.relay_names_[id(sh.sensor())] = k
        if not self.sensors_:
            raise ValueError("load_dict(): at least one sensor is required")
        self._data = {}
        self._data_ver = {}
        self._handles = {}
        self._nlos_fp = {}

    def _drop_handles(self, sensor_key):
        lib = _cabi.load_library()
        for k in [k for k in self._handles if k[0] == sensor_key]:
            lib.mtr_scene_destroy(self._handles.pop(k))
            self._nlos_fp.pop(k, None)

    def sensors(self):
        return self.sensors_

    def emitters(self):
        return self.emitters_ + list(self.lights_.values())

    def shapes(self):
        return list(self.shape_objs_.values())

    def integrator(self):
        return self.integrator_

    def data(self, sensor=0):
        """Flat float32 arrays for a sensor (what crosses the C-ABI)."""
        if isinstance(sensor, int):
            sensor = self.sensors_[sensor]
        key = id(sensor)
        # (... or a point / spot emitter did: its position, to_world or angles)
        ver = (getattr(sensor, "version_", 0), sum(getattr(l, "version_", 0) for l in self.lights_.values()))
        if isinstance(sensor, RadianceMeter) and _variant_mod.is_polarized():
            raise ValueError(f"{_variant_mod.get()}: a radiancemeter renders with the unpolarized variants only")
        old = self._data_ver.get(key, (0, 0))
        if key in self._data and old != ver and old[1] == ver[1] and isinstance(sensor, RadianceMeter):
            # a radiancemeter moved (a scan: params["sensor.to_world"] in a loop): the camera record alone is flattened again and
            # handed to the device scenes (mtr_scene_set_camera) — geometry, tables and BVH stay
            from .scene import flatten_radiancemeter
            flatten_radiancemeter(self._data[key], sensor.dict_)
            lib = _cabi.load_library() if any(h[0] == key for h in self._handles) else None
            for hkey in [h for h in self._handles if h[0] == key]:
                if lib.mtr_scene_set_camera(self._handles[hkey], C.byref(self._data[key].camera)) != 0:
                    lib.mtr_scene_destroy(self._handles.pop(hkey))
                    self._nlos_fp.pop(hkey, None)
        elif key in self._data and old != ver:      # the camera moved (params["sensor.to_world"]): re-flatten
            del self._data[key]
            self._drop_handles(key)
        self._data_ver[key] = ver
        if key not in self._data:
            self._data[key] = flatten_scene(self.dict_, sensor.film(), sensor.dict_, self.base_dir,
                                            self.relay_names_.get(key), self.approximate_materials, self.geometry_,
                                            own_materials=self.own_materials_, lights=self.lights_)
            self._apply_params(self._data[key])
        sd = self._data[key]
        sd.film = film_desc_from(sensor.film())
        from .integrators.transientnlospath import TransientNLOSPath
        # NLOS tier (rebuilt from the live objects): a nlos_capture_meter on its relay wall, or — as in the reference's
        # examples/transient-nlos/nlos-z-*.xml — transient_nlos_path behind an ordinary perspective camera
        if key in self.relay_names_ or isinstance(self.integrator_, TransientNLOSPath):
            from .scene import nlos_desc_from
            if _variant_mod.is_polarized():
                raise ValueError(f"{_variant_mod.get()}: the polarized variants render with transient_path only "
                                 "(transient_nlos_path is not available)")
            if len(self.emitters_) != 1:
                raise AssertionError(f"You have defined multiple ({len(self.emitters_)}) emitters in the scene with a "
                                     "NLOS capture meter. You should have only 1.")
            sd.nlos = nlos_desc_from(self.integrator_, sensor, self.emitters_[0], sd.relay_shape)
        return sd

    # -- differentiable parameters (mi.traverse keys of mtr_render_grad) ------------------------------------------
    def param_keys(self):
        """{key: 3 floats}: the differentiable parameters and their values, from the dictionary (nothing is flattened)"""
        from .scene import param_locations, tint_locations, rgb3
        if self.geometry_ is not None:
            return {}
        out = {k: list(self.param_values_.get(k, rgb3(v))) for k, (_, _, v) in param_locations(self.dict_).items()}
        # ... and the specular tints the dictionary sets (<bsdf>.specular_reflectance.value / .specular_transmittance.value)
        if self.approximate_materials in (False, None, "textures"):
            out.update({k: list(self.param_values_.get(k, rgb3(v))) for k, (_, _, v) in tint_locations(self.dict_).items()})
        k = self.laser_key()
        if k is not None:
            out[k] = [float(x) for x in self.emitters_[0].irradiance]
        return out

    def laser_key(self):
        """``<emitter id>.irradiance.value`` of a NLOS scene's projector (the one emitter of transient_nlos_path), else None"""
        from .integrators.transientnlospath import TransientNLOSPath
        if isinstance(self.integrator_, TransientNLOSPath) and len(self.emitters_) == 1:
            return f"{self.emitter_names_[0]}.irradiance.value"
        return None

    def grad_keys(self, sensor=0):
        """{key: ("material" | "emitter", index)}: the parameters mtr_render_grad differentiates, resolved to the flattened
        tables; a NLOS scene's laser is its one "emitter" (grad_emitters of mtr_render_grad is (1, 3))"""
        sd = self.data(sensor)
        k = self.laser_key()
        if k is None or sd.nlos is None:
            return sd.grad_keys
        return {**sd.grad_keys, k: ("emitter", 0)}

    def tint_keys(self, sensor=0):
        """{key: slot}: the constant specular tints mtr_render_grad_tint / mtr_render_fwd_tint differentiate, resolved to the slots
        of mtr_scene_tint_layout: ``specular_reflectance.value`` / ``specular_transmittance.value`` of a conductor,
        roughconductor, dielectric, thindielectric or roughdielectric whose dictionary sets the property.  Empty on a NLOS scene."""
        from .scene import tint_slot_table
        sd = self.data(sensor)
        if sd.nlos is not None:
            return {}
        slots = tint_slot_table(sd.materials, sd.n_materials)
        return {k: slots[mw] for k, mw in sd.tint_params.items()}

    def n_tint_slots(self, sensor=0):
        from .scene import tint_slot_table
        sd = self.data(sensor)
        return len(tint_slot_table(sd.materials, sd.n_materials))

    def texture_locations_(self):
        from .scene import texture_locations
        if self.geometry_ is not None or self.approximate_materials not in (False, None, "textures"):
            return {}
        return texture_locations(self.dict_, self.base_dir)

    def texture_param_keys(self):
        """{key: (H, W, 3) float32}: the texels of the differentiable bitmaps by mitsuba's ``.data`` key — linear RGB, after sRGB
        decoding unless ``raw`` —, from the dictionary and the bitmap files (nothing is flattened)"""
        from .scene import load_bitmap_texture
        out = {}
        for k, tid in self.texture_locations_().items():
            if tid not in self.texture_values_:
                self.texture_values_[tid] = load_bitmap_texture(tid[0], tid[1])
            out[k] = self.texture_values_[tid].copy()
        return out

    def texture_keys(self, sensor=0):
        """{key: index into data().textures}: the bitmaps mtr_render_grad_tex differentiates — every material on them a `diffuse`
        reflectance.  Keys of BSDFs that name one bitmap file share its index."""
        return self.data(sensor).texture_keys

    def grad_tex_tier(self, sensor=0):
        """"none" | "slab" | "global": the tier mtr_render_grad_tex runs for this scene on the current device"""
        from .runtime import get_context
        ctx = get_context()
        t = C.c_uint32(0)
        ctx.check(ctx.lib.mtr_render_grad_tex_tier(self.gpu_handle(ctx, sensor), C.byref(t)), "mtr_render_grad_tex_tier")
        return ("none", "slab", "global")[int(t.value)]

    def set_texture_param(self, key, value):
        """new texels for the bitmap of a ``.data`` key ((H, W, 3), the bitmap's own size): the flattened tables take them
        — and the mean colour that stands in as the materials' `a` —, the device scenes re-upload that one bitmap
        (mtr_scene_set_texture); nothing else is rebuilt"""
        import numpy as np
        from .scene import texture_mean
        cur = self.texture_param_keys()
        if key not in cur:
            raise KeyError(key)
        if hasattr(value, "detach"):
            value = value.detach().cpu().numpy()
        v = np.ascontiguousarray(value, dtype=np.float32)
        if v.shape != cur[key].shape:
            raise ValueError(f"{key}: expected texels of shape {cur[key].shape}, got {v.shape}")
        tid = self.texture_locations_()[key]
        self.texture_values_[tid] = v.copy()
        lib = _cabi.load_library()
        for skey, sd in self._data.items():
            if tid not in sd.texture_ids:
                continue
            self._apply_params(sd)
            i = sd.texture_ids[tid]
            a = np.array([[sd.materials[m].a[c] for c in range(3)] for m in range(max(1, sd.n_materials))], np.float32)
            r = np.array([[sd.emitters[e].radiance[c] for c in range(3)] for e in range(max(1, sd.n_emitters))], np.float32)
            for hkey in [h for h in self._handles if h[0] == skey]:
                h = self._handles[hkey]
                # (the colour tables follow: `a` of the materials on the bitmap is this layer's own f32 mean)
                if lib.mtr_scene_set_texture(h, i, C.c_void_p(sd.textures[i].ctypes.data)) != 0 or \
                        lib.mtr_scene_set_colors(h, C.c_void_p(a.ctypes.data), C.c_void_p(r.ctypes.data)) != 0:
                    lib.mtr_scene_destroy(self._handles.pop(hkey))
                    self._nlos_fp.pop(hkey, None)

    def ensure_own_records(self, keys, sensor=0):
        """every key of ``keys`` must own its material record: a BSDF dictionary that several shapes share is flattened once per
        shape from then on (only when one of its keys is set or differentiated: other scenes keep their tables as they are)"""
        if self.own_materials_:
            return
        sd = self.data(sensor)
        gk = {**{k: i for k, (kind, i) in sd.grad_keys.items() if kind == "material"},
              **{k: m for k, (m, _) in sd.tint_params.items()}}
        # (records are counted per parameter: the two tints of one dielectric share their record and need no copy)
        recs = [(m, k.rsplit(".", 2)[-2]) for k, m in gk.items()]
        if any(k in gk and recs.count((gk[k], k.rsplit(".", 2)[-2])) > 1 for k in keys):
            self.own_materials_ = True
            for key in list(self._data):
                del self._data[key]
                self._drop_handles(key)

    def _apply_params(self, sd):
        import numpy as np
        from .scene import texture_mean
        for tid, v in self.texture_values_.items():
            i = getattr(sd, "texture_ids", {}).get(tid)
            if i is None or sd.textures[i].shape != v.shape:
                continue
            sd.textures[i][...] = v             # in place: descriptors handed out keep pointing at the array
            mean = texture_mean(sd.textures[i])
            for m in range(sd.n_materials):
                if sd.materials[m].albedo_texture == i + 1:
                    for c in range(3):
                        sd.materials[m].a[c] = np.float32(mean[c])
        for k, v in self.param_values_.items():
            if k not in sd.grad_keys:
                continue
            kind, i = sd.grad_keys[k]
            arr = sd.materials[i].a if kind == "material" else sd.emitters[i].radiance
            for c in range(3):
                arr[c] = v[c]
        for k, v in self.param_values_.items():
            if k in sd.tint_params:
                m, which = sd.tint_params[k]
                arr = sd.materials[m].c2 if which else sd.materials[m].c
                for c in range(3):
                    arr[c] = v[c]

    def set_param(self, key, value):
        """a differentiable parameter's new value (3 floats): the flattened tables take it, and the device scenes re-upload their
        material and emitter tables (mtr_scene_set_colors) — no BVH is rebuilt"""
        import numpy as np
        if key.endswith(".data"):
            return self.set_texture_param(key, value)
        if key not in self.param_keys():
            raise KeyError(key)
        if hasattr(value, "detach"):
            value = value.detach().cpu().numpy()
        v = np.asarray(value, dtype=np.float64).reshape(-1)
        if v.size == 1:
            v = np.repeat(v, 3)
        if v.size != 3:
            raise ValueError(f"{key}: expected 3 values, got {v.size}")
        if key == self.laser_key():
            # the projector object takes it: the NLOS description is rebuilt from the live objects on the next render (gpu_handle)
            self.emitters_[0].irradiance = [float(np.float32(x)) for x in v]
            return
        self.ensure_own_records([key])
        self.param_values_[key] = [float(np.float32(x)) for x in v]
        if key.endswith(".intensity.value") and key[:-len(".intensity.value")] in self.lights_:
            self.lights_[key[:-len(".intensity.value")]].intensity = np.asarray(self.param_values_[key], np.float64)      # the live object shows it
        lib = _cabi.load_library()
        for skey, sd in self._data.items():
            self._apply_params(sd)
            a = np.array([[sd.materials[i].a[c] for c in range(3)] for i in range(max(1, sd.n_materials))], np.float32)
            r = np.array([[sd.emitters[i].radiance[c] for c in range(3)] for i in range(max(1, sd.n_emitters))], np.float32)
            for hkey in [h for h in self._handles if h[0] == skey]:
                ok = lib.mtr_scene_set_colors(self._handles[hkey], C.c_void_p(a.ctypes.data), C.c_void_p(r.ctypes.data)) == 0
                if ok and sd.tint_params and sd.nlos is None:          # ... and the tints (mtr_scene_set_tints; no tint keys on the NLOS tier)
                    t = np.array([[[m.c[c] for c in range(3)], [m.c2[c] for c in range(3)]]
                                  for m in sd.materials[:max(1, sd.n_materials)]], np.float32)
                    t0, t1 = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
                    ok = lib.mtr_scene_set_tints(self._handles[hkey], C.c_void_p(t0.ctypes.data), C.c_void_p(t1.ctypes.data)) == 0
                if not ok:
                    lib.mtr_scene_destroy(self._handles.pop(hkey))     # (the NLOS tier: the next render creates the scene again)
                    self._nlos_fp.pop(hkey, None)

    def gpu_handle(self, ctx, sensor=0):
        if isinstance(sensor, int):
            sensor = self.sensors_[sensor]
        key = (id(sensor), ctx.device_index)
        sd = self.data(sensor)
        if key not in self._handles:
            h = C.c_void_p()
            d = sd.desc()
            ctx.check(ctx.lib.mtr_scene_create(ctx.handle, C.byref(d), C.byref(h)), "mtr_scene_create")
            self._handles[key] = h
        h = self._handles[key]
        fd = sd.film
        ctx.check(ctx.lib.mtr_scene_set_film(h, C.byref(fd)), "mtr_scene_set_film")
        if sd.nlos is not None:
            # TransientNLOSPath.prepare re-derives its tables on every render; here only when the description changed
            # (laser moved by nlos.focus_emitter_*, integrator property, film size): mtr_scene_set_nlos reallocates
            # four device tables and retraces the scanned points, which is not free per pass / per band
            d = sd.desc()
            n = sd.nlos
            n_val = type(n).from_buffer_copy(n)
            n_val.shapes = None                       # the table is compared by value, not by address
            fp = (bytes(n_val), bytes(memoryview(sd.shapes)),
                  int(fd.width), int(fd.height), int(fd.laser_scan_width), int(fd.laser_scan_height))
            if self._nlos_fp.get(key) != fp:
                ctx.check(ctx.lib.mtr_scene_set_nlos(h, d.nlos), "mtr_scene_set_nlos")
                self._nlos_fp[key] = fp
        return h

    def gpu_traits(self, sensor=0):
        """MTR_TRAIT_* bits of the scene on the current device (which specialised kernels its tables select)"""
        from .runtime import get_context
        ctx = get_context()
        t = C.c_uint32(0)
        ctx.check(ctx.lib.mtr_scene_traits(self.gpu_handle(ctx, sensor), C.byref(t)), "mtr_scene_traits")
        return int(t.value)

    def gpu_shadow_hull(self, sensor=0):
        """rectangles a safe shadow ray of the fused kernel is spared (mtr_scene_shadow_hull: the walls of a room of rectangles with one
        rectangular light); 0: the scene is no such room"""
        from .runtime import get_context
        ctx = get_context()
        n = C.c_uint32(0)
        ctx.check(ctx.lib.mtr_scene_shadow_hull(self.gpu_handle(ctx, sensor), C.byref(n)), "mtr_scene_shadow_hull")
        return int(n.value)

    def __del__(self):
        try:
            lib = _cabi.load_library()
            for h in self._handles.values():
                lib.mtr_scene_destroy(h)
        except Exception:
            pass


def load_dict(d: Dict[str, Any], base_dir: str = ".", approximate_materials: bool = False):
    """``mi.load_dict``: a scene dictionary -> Scene; a single shape / projector dictionary -> that object
    (tests/integration/test_nlos.py:86-98 builds the relay wall and the laser this way)."""
    t = d.get("type")
    if t == "scene":
        return Scene(d, base_dir, approximate_materials)
    if t in _SHAPE_TYPES:
        return _load_shape(d)
    if t == "projector":
        from .emitters import Projector
        e = Projector(Properties("projector", d))
        e.dict_ = d
        return e
    if t in ("point", "spot"):
        from .emitters import make_delta_emitter
        return make_delta_emitter(d)
    from . import integrators as _i, films as _f  # noqa: F401  (registers the plugins)
    if str(t).endswith("_film"):                                # stand-alone plugins, as 1-simple-nlos-scenes.ipynb builds them
        return plugins.create_film(t, Properties(t, d))
    if t in ("nlos_capture_meter", "perspective", "radiancemeter"):
        return _make_sensor(d)
    if str(t).startswith("transient"):
        return plugins.create_integrator(t, Properties(t, d))
    raise ValueError(f"load_dict(): unsupported top-level plugin type \"{t}\"")


def _tea32(v0, v1, rounds=4):
    """sample_tea_32 (mitsuba3's TEA, 4 rounds): returns v0"""
    M = 0xFFFFFFFF
    v0, v1, s = v0 & M, v1 & M, 0
    for _ in range(rounds):
        s = (s + 0x9E3779B9) & M
        v0 = (v0 + ((((v1 << 4) & M) + 0xA341316C) ^ ((v1 + s) & M) ^ ((v1 >> 5) + 0xC8013EA4))) & M
        v1 = (v1 + ((((v0 << 4) & M) + 0xAD90777D) ^ ((v0 + s) & M) ^ ((v0 >> 5) + 0x7E95761E))) & M
    return v0


def _grad_values(params):
    """the (key, tensor) pairs of ``params`` whose value is a torch tensor that requires grad or a forward_ad dual tensor"""
    if not params:
        return []
    from .integrators.common import _wants_grad
    return [(k, v) for k, v in params.items() if _wants_grad(v)]


def render(scene: Scene, params=None, sensor=0, integrator=None, seed=0, seed_grad=0, spp=0, spp_grad=0):
    """``mi.render``: returns ``(steady (H,W,3), transient (H,W,T,3))`` like the reference's
    TransientADIntegrator.render (common.py:212-213).  When a value of ``params`` is a torch tensor that requires grad, the
    tensors' ``.torch()`` carry a ``grad_fn``: their backward pass is ``integrator.render_backward`` at ``seed_grad`` (0: a TEA
    scramble of ``seed``, as mitsuba's mi.render) with ``spp_grad`` samples (0: ``spp``).  Inside
    ``torch.autograd.forward_ad.dual_level()`` the values that are dual tensors give the outputs tangents:
    ``integrator.render_forward`` at the same ``seed_grad`` / ``spp_grad``."""
    integ = integrator or scene.integrator()
    grads = _grad_values(params)
    if not grads:
        return integ.render(scene, sensor=sensor, seed=seed, spp=spp)
    if not hasattr(integ, "check_grad_"):
        raise ValueError(f"{type(integ).__name__}: differentiable rendering is available with transient_path on one GPU only")
    integ.check_grad_(scene, sensor, params)              # every refusal before any GPU work
    if spp_grad == 0:
        spp_grad = spp
    if seed_grad == 0:
        seed_grad = _tea32(seed, 1)                       # de-correlates the primal and the differential phase
    elif seed_grad == seed:
        raise ValueError("The primal and differential seed should be different to ensure unbiased gradient computation!")
    if getattr(params, "_dirty", None):
        params.update()
    import torch

    class _Render(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *values):
            steady, transient = integ.render(scene, sensor=sensor, seed=seed, spp=spp)
            return steady.torch().clone(), transient.torch().clone()

        @staticmethod
        def backward(ctx, g_s, g_t):
            g = integ.render_backward(scene, params, grad_in=(g_s, g_t), sensor=sensor, seed=seed_grad, spp=spp_grad)
            # (a 1-element value stands for the three channels: it receives their sum, on its own device like the 3-vector;
            # the (H, W, 3) texels of a `.data` key receive their own shape)
            return tuple(None if k not in g else
                         (g[k] if v.numel() == g[k].numel() else g[k].sum()).to(dtype=v.dtype, device=v.device).reshape(v.shape)
                         for k, v in grads)

        @staticmethod
        def jvp(ctx, *tangents):
            # forward mode (torch.autograd.forward_ad): the outputs' tangents are render_forward at seed_grad / spp_grad
            tan = {k: t for (k, _), t in zip(grads, tangents) if t is not None}
            d_s, d_t = integ.render_forward(scene, params, sensor=sensor, seed=seed_grad, spp=spp_grad, tangents=tan)
            return d_s.torch(), d_t.torch()

    s, t = _Render.apply(*[v for _, v in grads])
    return TensorXf(s), TensorXf(t)


class _Params(dict):
    def __init__(self, objs):
        super().__init__()
        self._objs = objs
        self._dirty = set()

    def __setitem__(self, k, v):
        self._dirty.add(k)
        super().__setitem__(k, v)

    def update(self, *a, **k):
        if a or k:
            return super().update(*a, **k)
        for key in self._dirty:
            obj, attr = self._objs[key]
            if isinstance(obj, Scene):                 # a differentiable parameter (attr is its key)
                obj.set_param(attr, self[key])
                continue
            cur = getattr(obj, attr)
            try:
                setattr(obj, attr, type(cur)(self[key]))
            except Exception:
                setattr(obj, attr, self[key])
        self._dirty.clear()


def traverse(obj):
    """``mi.traverse`` for the film parameters the reference exports (transient_hdr_film.py:295-308) and a perspective
    sensor's or a radiancemeter's ``to_world`` (settable: ``update()`` re-flattens the camera; a radiancemeter's scene stays on
    the device)."""
    objs = {}

    class _CB:
        def __init__(self, prefix, o):
            self.prefix, self.o = prefix, o

        def put(self, name, value, flags=0):
            objs[self.prefix + name] = (self.o, name)

    targets = []
    scene_keys = {}
    if isinstance(obj, Scene):
        # mitsuba's keys of the differentiable parameters: <bsdf id>.reflectance.value,
        # <shape id>.bsdf[.brdf_0].reflectance.value, <shape id>.emitter.radiance.value
        for k, v in obj.param_keys().items():
            objs[k] = (obj, k)
            scene_keys[k] = v
        # ... and <bsdf id>.reflectance.data, <shape id>.bsdf[.brdf_0].reflectance.data: the (H, W, 3) texels of a bitmap
        for k, v in obj.texture_param_keys().items():
            objs[k] = (obj, k)
            scene_keys[k] = v
        # ... <emitter id>.position (point), <emitter id>.to_world / .cutoff_angle / .beam_width (spot): update() re-flattens the scene
        for name, light in obj.lights_.items():
            targets.append((f"{name}.", light))
        for i, s in enumerate(obj.sensors()):
            targets.append((f"sensor{'' if i == 0 else i}.film.", s.film()))
            if isinstance(s, PerspectiveSensor):
                targets.append((f"sensor{'' if i == 0 else i}.", s))
    elif hasattr(obj, "film") and callable(obj.film):               # a sensor: its own keys + "film.*"
        targets.append(("", obj))
        targets.append(("film.", obj.film()))
    else:
        targets.append(("", obj))
    for prefix, o in targets:
        o.traverse(_CB(prefix, o))
    p = _Params(objs)
    for k, (o, attr) in objs.items():
        dict.__setitem__(p, k, scene_keys[k] if k in scene_keys else getattr(o, attr))
    return p


def load_file(path, **kwargs):
    from .xml_loader import load_file as _lf
    return _lf(path, **kwargs)
