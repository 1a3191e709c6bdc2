"""Host-side sensor + sampler objects (only what the transient_path hot path touches)."""
from __future__ import annotations

from ..scene import Properties


class IndependentSampler:
    """``independent`` sampler [mitsuba3: src/samplers/independent.cpp]: PCG32 streams seeded by
    TEA(base_seed + seed, lane).  The stream arithmetic itself is in the HIP kernels."""

    def __init__(self, props: Properties):
        self.sample_count_ = int(props.get("sample_count", 4))
        self.base_seed = int(props.get("seed", 0))
        self._wavefront_size = 0
        self._seed_value = self.base_seed
        self.samples_per_wavefront = 1

    def clone(self):
        s = IndependentSampler(Properties("independent", {"sample_count": self.sample_count_, "seed": self.base_seed}))
        return s

    def sample_count(self):
        return self.sample_count_

    def set_sample_count(self, spp):
        self.sample_count_ = int(spp)

    def set_samples_per_wavefront(self, n):
        self.samples_per_wavefront = int(n)

    def seed(self, seed, wavefront_size):
        self._seed_value = (self.base_seed + int(seed)) & 0xFFFFFFFF
        self._wavefront_size = int(wavefront_size)

    def seed_value(self):
        return self._seed_value

    # -- the few host-side draws the plugin layer makes itself (the seeder of multi-pass renders, common.py:72-75) --
    @staticmethod
    def _tea(v0, v1, rounds=4):
        M = 0xFFFFFFFF
        s = 0
        for _ in range(rounds):
            s = (s + 0x9E3779B9) & M
            v0 = (v0 + ((((v1 << 4) & M) + 0xA341316C) ^ ((v1 + s) & M) ^ ((v1 >> 5) + 0xC8013EA4))) & M
            v1 = (v1 + ((((v0 << 4) & M) + 0xAD90777D) ^ ((v0 + s) & M) ^ ((v0 >> 5) + 0x7E95761E))) & M
        return v0, v1

    def next_1d_first(self):
        """The FIRST ``next_1d()`` of every lane of the seeded wavefront, as float32 values: lane j's PCG32 stream is
        seeded with TEA(seed_value, j) [mitsuba3: independent.cpp seed(); drjit PCG32]; same integers as the kernels."""
        import numpy as np
        M64 = (1 << 64) - 1
        out = np.empty(self._wavefront_size, np.float32)
        for j in range(self._wavefront_size):
            v0, v1 = self._tea(self._seed_value, j)
            inc = ((v1 << 1) | 1) & M64
            state = (0 * 0x5851F42D4C957F2D + inc) & M64                 # state = 0; next(); state += initstate; next()
            state = (state + v0) & M64
            old = state = (state * 0x5851F42D4C957F2D + inc) & M64
            xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
            rot = old >> 59
            u = ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF
            out[j] = np.array([(u >> 9) | 0x3F800000], np.uint32).view(np.float32)[0] - np.float32(1.0)
        return out


class PerspectiveSensor:
    def __init__(self, sensor_dict, film, sampler):
        self.dict_ = sensor_dict
        self.film_ = film
        self.sampler_ = sampler
        self.version_ = 0            # bumped when a parameter the flattened camera depends on changes (Scene.data re-flattens)

    @property
    def to_world(self):
        from ..transform import to_transform
        return to_transform(self.dict_.get("to_world"))

    @to_world.setter
    def to_world(self, value):
        from ..transform import to_transform
        self.dict_ = dict(self.dict_, to_world=to_transform(value))
        self.version_ += 1

    def traverse(self, callback):
        """[mitsuba3: Sensor::traverse] the camera-to-world transform"""
        callback.put("to_world", self.to_world)

    def film(self):
        return self.film_

    def sampler(self):
        return self.sampler_


def coordinate_system(n):
    """[mitsuba3: coordinate_system (Duff et al.)] two unit vectors (s, t) that complete the unit vector ``n`` to a frame"""
    import math
    x, y, z = (float(v) for v in n)
    sign = math.copysign(1.0, z)
    a = -1.0 / (sign + z)
    b = x * y * a
    return [sign * (x * x * a) + 1.0, sign * b, -sign * x], [b, sign + y * y * a, -y]


class RadianceMeter(PerspectiveSensor):
    """``radiancemeter`` [mitsuba3: src/sensors/radiancemeter.cpp]: every sample of its 1 x 1 film is the ray from ``origin``
    along ``direction`` (or the local +z axis of ``to_world``) — the receiver of a single-pixel transient measurement.  It is
    flattened to the library's general camera record (radiancemeter_camera): no kernel knows about it."""

    def __init__(self, sensor_dict, film, sampler):
        from ..transform import ScalarTransform4f
        import numpy as np
        d = dict(sensor_dict)
        has_od = "origin" in d or "direction" in d
        if "to_world" in d and has_od:
            raise ValueError("radiancemeter: only one of the parameters 'origin' / 'direction' and 'to_world' can be specified "
                             "at the same time")
        if has_od:
            if "origin" not in d or "direction" not in d:
                raise ValueError("radiancemeter: if the sensor is specified through origin and direction both values must be set")
            o = np.asarray(d.pop("origin"), np.float64).reshape(3)
            v = np.asarray(d.pop("direction"), np.float64).reshape(3)
            if not np.linalg.norm(v) > 0:
                raise ValueError("radiancemeter: 'direction' must not be the zero vector")
            up, _ = coordinate_system(v / np.linalg.norm(v))
            d["to_world"] = ScalarTransform4f().look_at(o, o + v, up)
        if tuple(int(x) for x in film.size()) != (1, 1):
            raise ValueError("radiancemeter: This sensor only supports films of size 1x1 Pixels!")
        super().__init__(d, film, sampler)


def radiancemeter_camera(to_world):
    """(sample_to_camera, to_world, near_clip, far_clip) of a radiancemeter as the library's camera record: a degenerate
    projection that sends every film sample to the local direction (0, 0, 1) — camera_ray (mtr_core.h) then returns the origin
    and the +z axis of ``to_world`` whatever the jitter —, near_clip 0 (the ray starts AT the origin) and the largest finite f32
    as far_clip (tmax stays finite)."""
    import numpy as np
    from ..transform import to_transform
    s2c = np.zeros((4, 4), np.float64)
    s2c[2, 3] = 1.0
    s2c[3, 3] = 1.0
    return s2c, to_transform(to_world).matrix, 0.0, float(np.finfo(np.float32).max)
