"""Helpers to aim the laser of an NLOS scene.  Public names and argument order follow mitransient/nlos.py:5-70;
all three resolve to one world-space point and share ``_aim``.

``capture_geometry`` / ``backproject`` / ``laplacian_filter`` turn a rendered capture back into a volume of the hidden
scene: the sum runs in HIP (``mtr_backproject``, csrc/mtr_backproject.hip), torch is plumbing."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _cabi
from .transform import ScalarTransform4f

_UP = (0.0, 1.0, 0.0)


def _aim(wall, laser, point):
    # Re-orient the laser (its position is kept) and tell the capture meter where it lands: the meter uses
    # the laser->wall distance and the illuminated point when account_first_and_last_bounces is off.
    point = np.asarray(point, dtype=np.float64).reshape(3)
    eye = laser.world_transform().translation()
    laser.to_world = ScalarTransform4f().look_at(origin=eye, target=point, up=list(_UP))
    meter = wall.sensor()
    if meter is not None:
        meter.laser_target = point
        meter.laser_bounce_opl = float(np.linalg.norm(point - eye))


def _wall_point(wall, uv):
    return wall.sample_position(0.0, uv, True).p


def focus_emitter_at_relay_wall_3dpoint(target, relay_wall, emitter):
    """Point the laser at the world-space point ``target`` (nlos.py:5-32)."""
    _aim(relay_wall, emitter, target)


def focus_emitter_at_relay_wall_uv(uv, relay_wall, emitter):
    """Point the laser at the relay-wall point with surface coordinates ``uv`` in [0,1]^2 (nlos.py:35-47)."""
    _aim(relay_wall, emitter, _wall_point(relay_wall, uv))


def focus_emitter_at_relay_wall_pixel(pixel, relay_wall, emitter):
    """Point the laser at the relay-wall point seen by film pixel ``pixel`` (nlos.py:50-70).  The divisor is the
    meter's scan resolution, which for confocal captures differs from the 1x1 film."""
    nx, ny = relay_wall.sensor().film_size
    col, row = (pixel.x, pixel.y) if hasattr(pixel, "x") else (pixel[0], pixel[1])
    _aim(relay_wall, emitter, _wall_point(relay_wall, (float(col) / nx, float(row) / ny)))


# ---------------------------------------------------------------- backprojection
_CAPTURE_NAMES = {_cabi.MTR_CAPTURE_SINGLE: "single", _cabi.MTR_CAPTURE_CONFOCAL: "confocal", _cabi.MTR_CAPTURE_EXHAUSTIVE: "exhaustive"}
_INTERPOLATIONS = {"nearest": _cabi.MTR_BACKPROJECT_NEAREST, "linear": _cabi.MTR_BACKPROJECT_LINEAR}


@dataclass
class CaptureGeometry:
    """Where and when a NLOS capture was taken: what ``backproject`` needs beside the transient tensor.

    ``sensor_points`` (H, W, 3) are the scanned relay-wall points in film order, ``laser_points`` (L, 3) the illuminated ones
    (Confocal: the sensor points; Single: one point; Exhaustive: the grid, point ``l = laser_x * Ly + laser_y``).
    ``sensor_offset`` (H, W) / ``laser_offset`` (L) are the sensor -> wall and laser -> wall path lengths a capture rendered with
    ``account_first_and_last_bounces`` contains, zeros otherwise.  All arrays are float64 numpy."""
    capture_type: int
    sensor_points: np.ndarray
    laser_points: np.ndarray
    sensor_offset: np.ndarray
    laser_offset: np.ndarray
    start_opl: float
    bin_width_opl: float
    temporal_bins: int
    laser_grid: tuple = None                  # Exhaustive: (Lx, Ly) of the film's laser_x / laser_y axes

    def __post_init__(self):
        self.capture_type = int(self.capture_type)
        self.sensor_points = np.asarray(self.sensor_points, dtype=np.float64)
        self.laser_points = np.asarray(self.laser_points, dtype=np.float64).reshape(-1, 3)
        self.sensor_offset = np.asarray(self.sensor_offset, dtype=np.float64)
        self.laser_offset = np.asarray(self.laser_offset, dtype=np.float64).reshape(-1)


def capture_geometry(scene, sensor=0) -> CaptureGeometry:
    """The :class:`CaptureGeometry` of a scene rendered by ``transient_nlos_path`` through a ``nlos_capture_meter``.

    Raises ``ValueError`` for a NLOS scene behind a ``perspective`` camera (no relay wall to scan), for an ``is_confocal``
    1 x 1 meter (one histogram: nothing to backproject), and for an Exhaustive capture without
    ``force_equal_illumination_scanning`` — its laser grid is ray-cast on the device; build the ``CaptureGeometry`` yourself
    with the ``laser_points`` you know."""
    from .integrators.transientnlospath import TransientNLOSPath
    from .sensors.nloscapturemeter import NLOSCaptureMeter
    meter = scene.sensors()[sensor] if isinstance(sensor, int) else sensor
    integ = scene.integrator()
    if not isinstance(integ, TransientNLOSPath):
        raise ValueError("capture_geometry: the scene's integrator is not transient_nlos_path")
    if not isinstance(meter, NLOSCaptureMeter):
        raise ValueError(f"capture_geometry: the sensor is a {type(meter).__name__}, not a nlos_capture_meter: a NLOS scene behind "
                         "a perspective camera has no relay wall whose scan points could be backprojected")
    if meter.is_confocal:
        raise ValueError("capture_geometry: an is_confocal nlos_capture_meter has a 1 x 1 film (one scan point per render); "
                         "render the scan with capture_type 'confocal' on a W x H film instead")
    relay, film = meter.shape(), meter.film()
    if relay is None:
        raise ValueError("capture_geometry: the nlos_capture_meter is not attached to a relay-wall shape")
    W, H = (int(v) for v in film.size())
    pts = np.empty((H, W, 3), np.float64)
    for y in range(H):
        for x in range(W):
            pts[y, x] = np.asarray(relay.sample_position(0.0, ((x + 0.5) / W, (y + 0.5) / H)).p, dtype=np.float64).reshape(3)
    ct = int(integ.capture_type)
    grid = None
    if ct == _cabi.MTR_CAPTURE_CONFOCAL:
        lp = pts.reshape(-1, 3).copy()
    elif ct == _cabi.MTR_CAPTURE_SINGLE:
        lp = np.asarray(meter.laser_target, dtype=np.float64).reshape(1, 3).copy()
    else:
        if not integ.force_equal_grids:
            raise ValueError("capture_geometry: an Exhaustive capture without force_equal_illumination_scanning has a laser grid "
                             "that is ray-cast on the device; pass your laser_points to CaptureGeometry instead")
        grid = (int(film.laser_scan_width), int(film.laser_scan_height))
        if grid[0] * grid[1] != W * H:
            raise ValueError("capture_geometry: force_equal_illumination_scanning needs a laser grid as large as the film")
        lp = pts.reshape(-1, 3).copy()            # point i = sensor point (i // W, i % W); film cell laser_x = i // Ly, laser_y = i % Ly
    if integ.account_first_and_last_bounces:
        emitters = scene.emitters()
        if len(emitters) != 1:
            raise ValueError(f"capture_geometry: a NLOS scene has exactly one emitter, this one has {len(emitters)}")
        lo_origin = np.asarray(emitters[0].world_transform().translation(), dtype=np.float64).reshape(3)
        so = np.linalg.norm(np.asarray(meter.sensor_origin, dtype=np.float64).reshape(3) - pts, axis=-1)
        lo = np.linalg.norm(lo_origin - lp, axis=-1)
    else:
        so, lo = np.zeros((H, W)), np.zeros(len(lp))
    return CaptureGeometry(ct, pts, lp, so, lo, float(film.start_opl), float(film.bin_width_opl), int(film.temporal_bins), grid)


def laplacian_filter(volume):
    """The 7-point negative Laplacian of a (nz, ny, nx) torch tensor with zero padding, ``6 v - (its six neighbours)``: the
    usual sharpening of a backprojected volume.  Torch ops on whatever device the tensor lives on (CPU tensors too)."""
    import torch
    if volume.ndim != 3:
        raise ValueError(f"laplacian_filter: a (nz, ny, nx) volume is expected, got shape {tuple(volume.shape)}")
    p = torch.nn.functional.pad(volume, (1, 1, 1, 1, 1, 1))
    return (6.0 * volume - p[2:, 1:-1, 1:-1] - p[:-2, 1:-1, 1:-1] - p[1:-1, 2:, 1:-1] - p[1:-1, :-2, 1:-1]
            - p[1:-1, 1:-1, 2:] - p[1:-1, 1:-1, :-2])


def _checked_call(transient, g, volume_min, volume_max, resolution, interpolation, channel, filter):
    """Everything ``backproject`` can refuse without a GPU; returns (S, L, T, has a channel axis, vmin, vmax, (nx, ny, nz))"""
    if not isinstance(g, CaptureGeometry):
        raise ValueError("backproject: geometry must be a CaptureGeometry (see capture_geometry)")
    if interpolation not in _INTERPOLATIONS:
        raise ValueError(f"backproject: interpolation must be 'nearest' or 'linear', not {interpolation!r}")
    if filter not in (None, "laplacian"):
        raise ValueError(f"backproject: filter must be None or 'laplacian', not {filter!r}")
    if g.capture_type not in _CAPTURE_NAMES:
        raise ValueError(f"backproject: unknown capture type {g.capture_type}")
    if g.sensor_points.ndim != 3 or g.sensor_points.shape[-1] != 3:
        raise ValueError(f"backproject: sensor_points must be (H, W, 3), got {g.sensor_points.shape}")
    H, W = g.sensor_points.shape[:2]
    S, L, T = H * W, len(g.laser_points), int(g.temporal_bins)
    if S == 0 or L == 0 or T <= 0:
        raise ValueError("backproject: a capture of zero size")
    if g.sensor_offset.size != S or g.laser_offset.size != L:
        raise ValueError(f"backproject: the offsets must match the points ({S} sensor, {L} laser), got {g.sensor_offset.size} and {g.laser_offset.size}")
    if g.capture_type == _cabi.MTR_CAPTURE_CONFOCAL and L != S:
        raise ValueError(f"backproject: a confocal capture has one laser point per sensor point ({S}), the geometry has {L}")
    if g.capture_type == _cabi.MTR_CAPTURE_SINGLE and L != 1:
        raise ValueError(f"backproject: a single capture has one laser point, the geometry has {L}")
    if not g.bin_width_opl > 0.0:
        raise ValueError(f"backproject: bin_width_opl must be positive, got {g.bin_width_opl}")
    shape = tuple(int(v) for v in transient.shape)
    exhaustive = g.capture_type == _cabi.MTR_CAPTURE_EXHAUSTIVE
    if exhaustive:
        if len(shape) not in (5, 6):
            raise ValueError(f"backproject: an exhaustive capture is (H, W, Lx, Ly, T) or (H, W, Lx, Ly, T, C), got {shape}")
        if shape[2] * shape[3] != L:
            raise ValueError(f"backproject: the capture's laser grid {shape[2:4]} does not match the geometry's {L} laser points")
        t_axis = 4
    else:
        if len(shape) not in (3, 4):
            raise ValueError(f"backproject: a {_CAPTURE_NAMES[g.capture_type]} capture is (H, W, T) or (H, W, T, C), got {shape}")
        t_axis = 2
    if shape[:2] != (H, W):
        raise ValueError(f"backproject: the capture is {shape[0]} x {shape[1]} scan points, the geometry {H} x {W}")
    if shape[t_axis] != T:
        raise ValueError(f"backproject: the capture has {shape[t_axis]} time bins, the geometry {T}")
    has_c = len(shape) == t_axis + 2
    if channel is not None:
        if not has_c:
            raise ValueError("backproject: channel= needs a capture with a channel axis")
        if not 0 <= int(channel) < shape[-1]:
            raise ValueError(f"backproject: channel {channel} is outside the capture's {shape[-1]} channels")
    if has_c and shape[-1] == 0:
        raise ValueError("backproject: a capture without channels")
    vmin = np.asarray(volume_min, dtype=np.float64).reshape(-1)
    vmax = np.asarray(volume_max, dtype=np.float64).reshape(-1)
    if vmin.size != 3 or vmax.size != 3 or not np.all(np.isfinite(vmin)) or not np.all(np.isfinite(vmax)):
        raise ValueError("backproject: volume_min and volume_max are three finite coordinates each")
    if not np.all(np.float32(vmax) > np.float32(vmin)):
        raise ValueError(f"backproject: an empty volume box {vmin.tolist()} .. {vmax.tolist()}")
    res = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(v) for v in resolution)
    if len(res) != 3 or min(res) <= 0:
        raise ValueError(f"backproject: resolution is a positive int or (nx, ny, nz), got {resolution!r}")
    return S, L, T, has_c, vmin, vmax, res


def backproject(transient, geometry, volume_min, volume_max, resolution, interpolation="nearest", channel=None, filter=None):
    """Backproject a NLOS capture into a volume of the hidden scene, on the GPU (``mtr_backproject``).

    ``transient``: what ``mi.render`` returned (used where it lies, no host copy), a torch tensor or a numpy array, of shape
    (H, W, T) or (H, W, T, C), an Exhaustive capture (H, W, Lx, Ly, T[, C]); channels are averaged unless ``channel=k`` picks
    one; other dtypes and non-contiguous input are converted.  ``geometry``: a :class:`CaptureGeometry`
    (:func:`capture_geometry`).  The volume is the axis-aligned box ``volume_min`` .. ``volume_max`` with ``resolution`` =
    n or (nx, ny, nz) voxels; voxel ``v`` receives ``sum over (s, l) of H[s, l, bin(|P_s - v| + |v - P_l| + offsets)]``, with
    ``interpolation`` "nearest" (the bin a rendered path of that length was splatted into) or "linear" (between bin centres).
    ``filter="laplacian"`` applies :func:`laplacian_filter`.  Returns a CUDA torch tensor (nz, ny, nx); the sum has a fixed
    order, the same call gives the same bits.

    Out of scope: autograd through ``backproject`` (the result carries no graph), phasor-field reconstruction, LCT / f-k
    migration, non-rectangular relay walls in ``capture_geometry`` (a hand-built ``CaptureGeometry`` takes any points).
    Shape and geometry mismatches raise ``ValueError`` before the GPU is touched."""
    from .tensor import TensorXf
    if isinstance(transient, TensorXf):
        transient = transient.torch()
    if not hasattr(transient, "shape"):
        transient = np.asarray(transient)
    g = geometry
    S, L, T, has_c, vmin, vmax, res = _checked_call(transient, g, volume_min, volume_max, resolution, interpolation, channel, filter)

    from .runtime import get_context
    ctx = get_context()
    import torch
    dev = torch.device("cuda", ctx.device_index)
    t = transient if isinstance(transient, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(transient))
    t = t.detach().to(device=dev, dtype=torch.float32)
    if has_c:
        t = t[..., int(channel)] if channel is not None else (t[..., 0] if t.shape[-1] == 1 else t.mean(dim=-1))
    t = t.contiguous()

    def dev_f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    sp, lp = dev_f32(g.sensor_points.reshape(-1, 3)), dev_f32(g.laser_points)
    so, lo = dev_f32(g.sensor_offset.reshape(-1)), dev_f32(g.laser_offset)
    volume = torch.empty((res[2], res[1], res[0]), dtype=torch.float32, device=dev)
    d = _cabi.mtr_backproject_desc()
    d.capture_type, d.interpolation = g.capture_type, _INTERPOLATIONS[interpolation]
    d.n_sensor, d.n_laser, d.temporal_bins = S, L, T
    d.start_opl, d.bin_width_opl = np.float32(g.start_opl), np.float32(g.bin_width_opl)
    for k in range(3):
        d.volume_min[k], d.volume_max[k] = np.float32(vmin[k]), np.float32(vmax[k])
    d.nx, d.ny, d.nz = res
    d.sensor_points, d.laser_points, d.sensor_offset, d.laser_offset = sp.data_ptr(), lp.data_ptr(), so.data_ptr(), lo.data_ptr()
    with torch.cuda.device(dev):
        ctx.bind_current_stream()
        ctx.check(ctx.lib.mtr_backproject(ctx.handle, C.byref(d), C.c_void_p(t.data_ptr()), C.c_void_p(volume.data_ptr())), "mtr_backproject")
    # (t, sp, lp, so, lo are released to torch's caching allocator, which hands them out again in stream order)
    return laplacian_filter(volume) if filter == "laplacian" else volume
