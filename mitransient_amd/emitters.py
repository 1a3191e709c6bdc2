"""Emitter objects that live outside shapes: the ``projector`` of the NLOS tier
(the laser of mitransient's NLOS scenes: tests/integration/test_nlos.py:29-39,
examples/transient-nlos/nlos_Z.xml:31-34), and mitsuba's ``point`` and ``spot`` emitters
of transient_path (a pulsed source next to the camera) — `area` emitters are part of their shape."""
from __future__ import annotations

import math

import numpy as np

from .scene import Properties, _color3
from .transform import ScalarTransform4f, to_transform


class Projector:
    """mitsuba's `projector` with a constant `irradiance` [mitsuba3: src/emitters/projector.cpp]:
    a pinhole at ``to_world``'s origin projecting along its +z axis inside ``fov`` degrees."""

    def __init__(self, props: Properties):
        self.to_world = to_transform(props.get("to_world", None))
        self.fov = float(props.get("fov", 0.0))
        if "fov" not in props:
            raise ValueError("projector: 'fov' is required")
        irr = props.get("irradiance", 1.0)
        if isinstance(irr, dict) and irr.get("type") not in ("rgb", "uniform", "spectrum"):
            raise ValueError("projector: only a constant rgb irradiance is supported")
        self.irradiance = _color3(irr, "projector.irradiance")
        self.scale = float(props.get("scale", 1.0))
        self.dict_ = None

    def world_transform(self) -> ScalarTransform4f:
        return self.to_world

    def traverse(self, callback):
        callback.put("to_world", self.to_world, 0)
        callback.put("scale", self.scale, 0)

    def to_string(self):
        return f"Projector[\n  fov = {self.fov},\n  origin = {self.to_world.translation()}\n]"

    __str__ = __repr__ = to_string


def _intensity(props, what):
    v = props.get("intensity", 1.0)
    if isinstance(v, dict) and v.get("type") not in ("rgb", "uniform", "spectrum"):
        raise ValueError(f"{what}: only a constant intensity is supported")
    return _color3(v, f"{what}.intensity")


class _DeltaEmitter:
    """what `point` and `spot` share: geometric attributes whose change re-flattens the scene (``version_``, as a
    perspective sensor's ``to_world``), and a constant ``intensity`` (three floats; mi.Scene.set_param keeps it current when
    ``<id>.intensity.value`` is updated)"""
    _GEOMETRY = ()

    def __setattr__(self, k, v):
        if k in self._GEOMETRY:
            object.__setattr__(self, "version_", getattr(self, "version_", 0) + 1)
        object.__setattr__(self, k, v)

    __str__ = __repr__ = lambda self: self.to_string()


class PointLight(_DeltaEmitter):
    """mitsuba's `point` [mitsuba3: src/emitters/point.cpp]: an isotropic source at ``position`` (or the translation of
    ``to_world``) of constant ``intensity`` (default 1).  sample_direction: ds.p = position, ds.pdf = 1, ds.delta, the weight
    intensity / dist^2; no ray hits it."""
    KIND = "point"
    _GEOMETRY = ("position",)

    def __init__(self, props: Properties):
        if "position" in props and "to_world" in props:
            raise ValueError("point: only one of the parameters 'position' and 'to_world' can be specified at the same time")
        if "position" in props:
            pos = props.get("position")
        else:
            pos = to_transform(props.get("to_world", None)).translation()
        self.position = [float(x) for x in np.asarray(pos, dtype=np.float64).reshape(3)]
        self.intensity = _intensity(props, "point")
        self.dict_ = None

    def traverse(self, callback):
        callback.put("position", self.position, 0)

    def fill_record(self, e):
        """kind, position and intensity of a mtr_emitter"""
        from . import _cabi
        e.kind = _cabi.MTR_EMITTER_POINT
        for k in range(3):
            e.center[k], e.radiance[k] = np.float32(self.position[k]), np.float32(self.intensity[k])

    def to_string(self):
        return f"PointLight[\n  position = {self.position},\n  intensity = {[float(x) for x in self.intensity]}\n]"


class SpotLight(_DeltaEmitter):
    """mitsuba's `spot` [mitsuba3: src/emitters/spot.cpp]: a source at ``to_world``'s origin along its +z axis of constant
    ``intensity`` (default 1) inside ``beam_width`` degrees (default 3/4 of the cutoff), falling linearly in the angle to zero at
    ``cutoff_angle`` (default 20): the curve mitransient's `angulararea` copied.  ``to_world`` must be rigid (a rotation and a
    translation, as look_at gives); a ``texture`` is not supported."""
    KIND = "spot"
    _GEOMETRY = ("to_world", "cutoff_angle", "beam_width")

    def __init__(self, props: Properties):
        if "texture" in props:
            raise ValueError("spot: a 'texture' is not supported (constant intensity only)")
        self.to_world = to_transform(props.get("to_world", None))
        self.cutoff_angle = float(props.get("cutoff_angle", 20.0))
        self.beam_width = float(props.get("beam_width", self.cutoff_angle * 3.0 / 4.0))
        self.intensity = _intensity(props, "spot")
        self.constants()
        self.dict_ = None

    def world_transform(self) -> ScalarTransform4f:
        return self.to_world

    def constants(self):
        """(position, axis, cutoff, cos_cutoff, cos_beam, inv_transition): spot.cpp's constructor on f64, the refusals of a
        cutoff below the beam and of a to_world that is not rigid"""
        cutoff, beam = math.radians(float(self.cutoff_angle)), math.radians(float(self.beam_width))
        if not cutoff >= beam:
            raise ValueError(f"spot: cutoff_angle ({self.cutoff_angle}) must not be smaller than beam_width ({self.beam_width})")
        if not (0.0 < cutoff <= math.pi and beam >= 0.0):
            raise ValueError(f"spot: cutoff_angle ({self.cutoff_angle}) must lie in (0, 180] degrees and beam_width must not be negative")
        m = np.asarray(to_transform(self.to_world).matrix, dtype=np.float64)
        r = m[:3, :3]
        if not np.allclose(r.T @ r, np.eye(3), atol=1e-6) or not np.allclose(m[3], [0, 0, 0, 1]):
            raise ValueError("spot: to_world must be rigid (rotation and translation only)")
        axis = r[:, 2] / np.linalg.norm(r[:, 2])
        # (cutoff == beam: an empty transition, +inf as in _angular_constants — `>= cos_beam` takes every lit direction first)
        return m[:3, 3], axis, cutoff, math.cos(cutoff), math.cos(beam), (math.inf if cutoff == beam else 1.0 / (cutoff - beam))

    def traverse(self, callback):
        callback.put("to_world", self.to_world, 0)
        callback.put("cutoff_angle", self.cutoff_angle, 0)
        callback.put("beam_width", self.beam_width, 0)

    def fill_record(self, e):
        from . import _cabi
        pos, axis, cutoff, cos_cutoff, cos_beam, inv_transition = self.constants()
        e.kind = _cabi.MTR_EMITTER_SPOT
        for k in range(3):
            e.center[k], e.axis[k], e.radiance[k] = np.float32(pos[k]), np.float32(axis[k]), np.float32(self.intensity[k])
        e.cutoff, e.cos_cutoff = np.float32(cutoff), np.float32(cos_cutoff)
        e.cos_beam, e.inv_transition = np.float32(cos_beam), np.float32(inv_transition)

    def to_string(self):
        return (f"SpotLight[\n  origin = {self.to_world.translation()},\n  cutoff_angle = {self.cutoff_angle},\n"
                f"  beam_width = {self.beam_width},\n  intensity = {[float(x) for x in self.intensity]}\n]")


_DELTA_TYPES = {"point": PointLight, "spot": SpotLight}


def make_delta_emitter(d):
    """the object of a `point` / `spot` dictionary"""
    e = _DELTA_TYPES[d["type"]](Properties(d["type"], d))
    e.dict_ = d
    return e
