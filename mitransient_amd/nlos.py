"""Helpers to aim the laser of an NLOS scene.  Public names and argument order follow mitransient/nlos.py:5-70;
all three resolve to one world-space point and share ``_aim``.

``capture_geometry`` / ``backproject`` / ``laplacian_filter`` turn a rendered capture back into a volume of the hidden
scene: the sum runs in HIP (``mtr_backproject``, csrc/mtr_backproject.hip), torch is plumbing.  ``forward_project`` is its
transpose (``mtr_forward_project``, csrc/mtr_forward_project.hip): the two are each other's autograd backward, and
``reconstruct_cgls`` iterates them to fit a volume to a capture.  ``phasor_backproject`` does the
same for the phasors a ``phasor_hdr_film`` develops (``mtr_phasor_backproject``, csrc/mtr_phasor_backproject.hip), and
``phasor_forward_project`` is its conjugate transpose (``mtr_phasor_forward_project``, csrc/mtr_phasor_forward_project.hip): the
same pairing in the frequency domain, with autograd and ``phasor_reconstruct_cgls``.  ``fk_migration`` is the closed-form
reconstruction of a confocal capture of a planar wall: two ``torch.fft`` transforms with three HIP passes around them
(``mtr_fk_prepare`` / ``mtr_fk_stolt`` / ``mtr_fk_finish``, csrc/mtr_fk.hip)."""
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


def _checked_geometry(who, g):
    """what both reconstructions refuse in a geometry, without a GPU; returns (H, W, S, L)"""
    if not isinstance(g, CaptureGeometry):
        raise ValueError(f"{who}: geometry must be a CaptureGeometry (see capture_geometry)")
    if g.capture_type not in _CAPTURE_NAMES:
        raise ValueError(f"{who}: unknown capture type {g.capture_type}")
    if g.sensor_points.ndim != 3 or g.sensor_points.shape[-1] != 3:
        raise ValueError(f"{who}: sensor_points must be (H, W, 3), got {g.sensor_points.shape}")
    H, W = g.sensor_points.shape[:2]
    S, L = H * W, len(g.laser_points)
    if S == 0 or L == 0:
        raise ValueError(f"{who}: a capture of zero size")
    if g.sensor_offset.size != S or g.laser_offset.size != L:
        raise ValueError(f"{who}: the offsets must match the points ({S} sensor, {L} laser), got {g.sensor_offset.size} and {g.laser_offset.size}")
    if g.capture_type == _cabi.MTR_CAPTURE_CONFOCAL and L != S:
        raise ValueError(f"{who}: a confocal capture has one laser point per sensor point ({S}), the geometry has {L}")
    if g.capture_type == _cabi.MTR_CAPTURE_SINGLE and L != 1:
        raise ValueError(f"{who}: a single capture has one laser point, the geometry has {L}")
    return H, W, S, L


def _checked_rows(who, shape, g, H, W, L, what):
    """the leading axes of a capture tensor against the geometry; returns the index of the time / frequency axis"""
    if g.capture_type == _cabi.MTR_CAPTURE_EXHAUSTIVE:
        if len(shape) not in (5, 6):
            raise ValueError(f"{who}: an exhaustive capture is {what[1]}, got {shape}")
        if shape[2] * shape[3] != L:
            raise ValueError(f"{who}: the capture's laser grid {shape[2:4]} does not match the geometry's {L} laser points")
        axis = 4
    else:
        if len(shape) not in (3, 4):
            raise ValueError(f"{who}: a {_CAPTURE_NAMES[g.capture_type]} capture is {what[0]}, got {shape}")
        axis = 2
    if shape[:2] != (H, W):
        raise ValueError(f"{who}: the capture is {shape[0]} x {shape[1]} scan points, the geometry {H} x {W}")
    return axis


def _checked_box(who, volume_min, volume_max, resolution):
    """(vmin, vmax, (nx, ny, nz)) of a call's volume"""
    vmin = np.asarray(volume_min, dtype=np.float64).reshape(-1)
    vmax = np.asarray(volume_max, dtype=np.float64).reshape(-1)
    if vmin.size != 3 or vmax.size != 3 or not np.all(np.isfinite(vmin)) or not np.all(np.isfinite(vmax)):
        raise ValueError(f"{who}: volume_min and volume_max are three finite coordinates each")
    if not np.all(np.float32(vmax) > np.float32(vmin)):
        raise ValueError(f"{who}: an empty volume box {vmin.tolist()} .. {vmax.tolist()}")
    res = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(v) for v in resolution)
    if len(res) != 3 or min(res) <= 0:
        raise ValueError(f"{who}: resolution is a positive int or (nx, ny, nz), got {resolution!r}")
    return vmin, vmax, res


def _checked_call(transient, g, volume_min, volume_max, resolution, interpolation, channel, filter, who="backproject"):
    """Everything ``backproject`` can refuse without a GPU; returns (S, L, T, has a channel axis, vmin, vmax, (nx, ny, nz))"""
    if interpolation not in _INTERPOLATIONS:
        raise ValueError(f"{who}: interpolation must be 'nearest' or 'linear', not {interpolation!r}")
    if filter not in (None, "laplacian"):
        raise ValueError(f"{who}: filter must be None or 'laplacian', not {filter!r}")
    H, W, S, L = _checked_geometry(who, g)
    T = int(g.temporal_bins)
    if T <= 0:
        raise ValueError(f"{who}: a capture of zero size")
    if not g.bin_width_opl > 0.0:
        raise ValueError(f"{who}: bin_width_opl must be positive, got {g.bin_width_opl}")
    shape = tuple(int(v) for v in transient.shape)
    t_axis = _checked_rows(who, shape, g, H, W, L, ("(H, W, T) or (H, W, T, C)", "(H, W, Lx, Ly, T) or (H, W, Lx, Ly, T, C)"))
    if shape[t_axis] != T:
        raise ValueError(f"{who}: the capture has {shape[t_axis]} time bins, the geometry {T}")
    has_c = len(shape) == t_axis + 2
    if channel is not None:
        if not has_c:
            raise ValueError(f"{who}: channel= needs a capture with a channel axis")
        if not 0 <= int(channel) < shape[-1]:
            raise ValueError(f"{who}: channel {channel} is outside the capture's {shape[-1]} channels")
    if has_c and shape[-1] == 0:
        raise ValueError(f"{who}: a capture without channels")
    vmin, vmax, res = _checked_box(who, volume_min, volume_max, resolution)
    return S, L, T, has_c, vmin, vmax, res


class _Projection:
    """One geometry and one volume box on the device: what ``mtr_backproject`` and ``mtr_forward_project`` share in a call and
    in the autograd graph of a call.  ``run(entry, src)`` launches either on a contiguous f32 CUDA tensor."""

    def __init__(self, ctx, g, S, L, T, vmin, vmax, res, interpolation, capture_shape):
        import torch
        self.ctx, self.dev = ctx, torch.device("cuda", ctx.device_index)

        def dev_f32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)
        # (the four arrays live as long as this object: a graph that holds it can run its backward later)
        self.arrays = (dev_f32(g.sensor_points.reshape(-1, 3)), dev_f32(g.laser_points), dev_f32(g.sensor_offset.reshape(-1)),
                       dev_f32(g.laser_offset))
        d = self.desc = _cabi.mtr_backproject_desc()
        d.capture_type, d.interpolation = g.capture_type, _INTERPOLATIONS[interpolation]
        d.n_sensor, d.n_laser, d.temporal_bins = S, L, T
        d.start_opl, d.bin_width_opl = np.float32(g.start_opl), np.float32(g.bin_width_opl)
        for k in range(3):
            d.volume_min[k], d.volume_max[k] = np.float32(vmin[k]), np.float32(vmax[k])
        d.nx, d.ny, d.nz = res
        d.sensor_points, d.laser_points, d.sensor_offset, d.laser_offset = (t.data_ptr() for t in self.arrays)
        self.shapes = {"mtr_backproject": (res[2], res[1], res[0]), "mtr_forward_project": tuple(capture_shape)}

    def run(self, entry, src):
        import torch
        src = src.to(device=self.dev, dtype=torch.float32).contiguous()
        other = "mtr_forward_project" if entry == "mtr_backproject" else "mtr_backproject"
        if tuple(src.shape) != self.shapes[other]:
            raise ValueError(f"{entry}: the input has shape {tuple(src.shape)}, {self.shapes[other]} is expected")
        out = torch.empty(self.shapes[entry], dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            self.ctx.bind_current_stream()
            self.ctx.check(getattr(self.ctx.lib, entry)(self.ctx.handle, C.byref(self.desc), C.c_void_p(src.data_ptr()),
                                                        C.c_void_p(out.data_ptr())), entry)
        # (src is released to torch's caching allocator, which hands it out again in stream order)
        return out


_functions = None


def _autograd_pair():
    """(Backproject, ForwardProject): the two kernels as torch.autograd.Functions, each the other's backward — the operators are
    transposes of one another (csrc/mtr_forward_project.h)"""
    global _functions
    if _functions is None:
        import torch

        class Backproject(torch.autograd.Function):
            @staticmethod
            def forward(fctx, capture, projection):
                fctx.projection = projection
                return projection.run("mtr_backproject", capture)

            @staticmethod
            def backward(fctx, grad_volume):
                return ForwardProject.apply(grad_volume, fctx.projection), None

        class ForwardProject(torch.autograd.Function):
            @staticmethod
            def forward(fctx, volume, projection):
                fctx.projection = projection
                return projection.run("mtr_forward_project", volume)

            @staticmethod
            def backward(fctx, grad_capture):
                return Backproject.apply(grad_capture, fctx.projection), None

        _functions = (Backproject, ForwardProject)
    return _functions


def _as_tensor(value):
    """(a torch tensor of what a call was handed, whether a graph is wanted through it)"""
    import torch
    t = value if isinstance(value, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(value))
    wanted = bool(t.requires_grad and torch.is_grad_enabled() and (t.is_floating_point() or t.is_complex()))
    return (t if wanted else t.detach()), wanted


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

    Autograd: a torch tensor that requires grad (``transient.torch()`` of a render whose ``params`` hold such tensors
    included), with grad enabled, gives a volume with a ``grad_fn`` — the backward pass is :func:`forward_project`, the
    transpose, so a loss on the volume reaches the capture and through ``mi.render`` the scene parameters; the channel
    selection and the filter are torch ops and differentiate by themselves.  Any other input takes the same path as ever,
    gives the same bits and carries no graph.

    A capture rendered in the frequency domain (``phasor_hdr_film``) is reconstructed by :func:`phasor_backproject`.
    A confocal capture of a planar wall also has the closed-form ``N^3 log N`` reconstruction of :func:`fk_migration`.
    Out of scope: the light-cone transform (LCT), non-rectangular relay walls in ``capture_geometry`` (a hand-built
    ``CaptureGeometry`` takes any points).  Shape and geometry mismatches raise ``ValueError`` before the GPU is touched."""
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
    t, wanted = _as_tensor(transient)
    t = t.to(device=torch.device("cuda", ctx.device_index), dtype=torch.float32)
    if has_c:
        t = t[..., int(channel)] if channel is not None else (t[..., 0] if t.shape[-1] == 1 else t.mean(dim=-1))
    t = t.contiguous()
    projection = _Projection(ctx, g, S, L, T, vmin, vmax, res, interpolation, t.shape)
    volume = _autograd_pair()[0].apply(t, projection) if wanted else projection.run("mtr_backproject", t)
    return laplacian_filter(volume) if filter == "laplacian" else volume


def _checked_forward_call(who, shape, g, volume_min, volume_max, interpolation):
    """Everything ``forward_project`` can refuse without a GPU; returns (S, L, T, vmin, vmax, (nx, ny, nz), the capture's shape)"""
    if interpolation not in _INTERPOLATIONS:
        raise ValueError(f"{who}: interpolation must be 'nearest' or 'linear', not {interpolation!r}")
    H, W, S, L = _checked_geometry(who, g)
    T = int(g.temporal_bins)
    if T <= 0:
        raise ValueError(f"{who}: a capture of zero size")
    if not g.bin_width_opl > 0.0:
        raise ValueError(f"{who}: bin_width_opl must be positive, got {g.bin_width_opl}")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError(f"{who}: a (nz, ny, nx) volume is expected, got shape {shape}")
    if g.capture_type == _cabi.MTR_CAPTURE_EXHAUSTIVE:
        grid = g.laser_grid
        if grid is None:
            raise ValueError(f"{who}: an exhaustive geometry needs laser_grid = (Lx, Ly) to shape the capture")
        grid = tuple(int(v) for v in grid)
        if len(grid) != 2 or grid[0] * grid[1] != L:
            raise ValueError(f"{who}: laser_grid {grid} does not match the geometry's {L} laser points")
        capture_shape = (H, W, grid[0], grid[1], T)
    else:
        capture_shape = (H, W, T)
    vmin, vmax, res = _checked_box(who, volume_min, volume_max, (shape[2], shape[1], shape[0]))
    return S, L, T, vmin, vmax, res, capture_shape


def forward_project(volume, geometry, volume_min, volume_max, interpolation="nearest"):
    """The transpose of :func:`backproject`: scatter a volume of the hidden scene into the capture it would produce, on the GPU
    (``mtr_forward_project``) — the three-bounce forward model of a hidden volume without the cosine and 1/r^2 factors, the
    gradient of a backprojection, and the other half of every iterative reconstruction (:func:`reconstruct_cgls`).

    ``volume``: (nz, ny, nx), a torch tensor on any device and of any dtype, a numpy array or a ``TensorXf``; the resolution is
    its shape, the box ``volume_min`` .. ``volume_max``.  Capture cell ``(s, l, b)`` receives the sum of the voxels whose path
    length ``backproject`` looks up in bin ``b`` — with the same weights, bit for bit, so that with the same arguments
    ``<backproject(y), x> = <y, forward_project(x)>`` up to f32 rounding.  Returns a CUDA f32 tensor (H, W, T); for an Exhaustive
    geometry (H, W, Lx, Ly, T) with (Lx, Ly) = ``geometry.laser_grid``.  The cells are summed with float atomics in LDS, whose
    order is not fixed: the same call gives the same capture to rounding, not to bits.

    Autograd: a volume that requires grad gives a capture with a ``grad_fn`` whose backward is ``backproject``.
    Refusals are ``ValueError`` before the GPU is touched."""
    from .tensor import TensorXf
    if isinstance(volume, TensorXf):
        volume = volume.torch()
    if not hasattr(volume, "shape"):
        volume = np.asarray(volume)
    g = geometry
    S, L, T, vmin, vmax, res, capture_shape = _checked_forward_call("forward_project", volume.shape, g, volume_min, volume_max, interpolation)
    from .runtime import get_context
    ctx = get_context()
    import torch
    t, wanted = _as_tensor(volume)
    t = t.to(device=torch.device("cuda", ctx.device_index), dtype=torch.float32).contiguous()
    projection = _Projection(ctx, g, S, L, T, vmin, vmax, res, interpolation, capture_shape)
    return _autograd_pair()[1].apply(t, projection) if wanted else projection.run("mtr_forward_project", t)


def reconstruct_cgls(transient, geometry, volume_min, volume_max, resolution, iterations=10, interpolation="linear", channel=None):
    """Fit a hidden volume to a capture: CGLS on ``min |forward_project(x) - y|`` from ``x = 0``, one ``forward_project`` and one
    ``backproject`` per iteration on the GPU, the rest torch ops.

    ``transient`` and ``channel`` as in :func:`backproject` (channels are averaged unless one is picked).  Returns
    ``(volume, residuals)``: the CUDA f32 volume (nz, ny, nx) after ``iterations`` steps and ``residuals[k] = |r_k| / |y|`` as
    Python floats, ``k = 0 .. iterations`` (``residuals[0] = 1``).  The result carries no graph.  A capture that is all zero
    returns a zero volume."""
    who = "reconstruct_cgls"
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"{who}: iterations is a positive int, got {iterations!r}")
    from .tensor import TensorXf
    if isinstance(transient, TensorXf):
        transient = transient.torch()
    if not hasattr(transient, "shape"):
        transient = np.asarray(transient)
    g = geometry
    S, L, T, has_c, vmin, vmax, res = _checked_call(transient, g, volume_min, volume_max, resolution, interpolation, channel, None, who)
    from .runtime import get_context
    ctx = get_context()
    import torch
    with torch.no_grad():
        y = _as_tensor(transient)[0].to(device=torch.device("cuda", ctx.device_index), dtype=torch.float32)
        if has_c:
            y = y[..., int(channel)] if channel is not None else (y[..., 0] if y.shape[-1] == 1 else y.mean(dim=-1))
        y = y.contiguous()
        projection = _Projection(ctx, g, S, L, T, vmin, vmax, res, interpolation, y.shape)

        def dot(a):
            return float(torch.sum(a.double() * a.double()))
        r = y.clone()
        s = projection.run("mtr_backproject", r)
        x, p = torch.zeros_like(s), s.clone()
        gamma, norm_y = dot(s), dot(y) ** 0.5
        residuals = [1.0]
        for _ in range(int(iterations)):
            if gamma == 0.0:                        # (converged, or y = 0)
                residuals.append(residuals[-1])
                continue
            q = projection.run("mtr_forward_project", p)
            alpha = gamma / dot(q)
            x += alpha * p
            r -= alpha * q
            s = projection.run("mtr_backproject", r)
            gamma, last = dot(s), gamma
            p = s + (gamma / last) * p
            residuals.append(dot(r) ** 0.5 / norm_y)
    return x, residuals

# ---------------------------------------------------------------- phasor-field reconstruction
_FLT_MAX = float(np.finfo(np.float32).max)


def uniform_frequency_step(frequencies):
    """The spacing of a uniformly spaced frequency table, or 0.0 for any other table — what ``phasor_backproject`` hands the
    kernel as ``freq_step``.  In float64: ``step = (f[F-1] - f[0]) / (F - 1)``; the table is uniform if every ``f[k]`` is within
    2 float32 ulps of ``max|f|`` of ``f[0] + k step``.  ``F == 1`` or ``step <= 0`` is not."""
    f = np.asarray(frequencies, dtype=np.float64).reshape(-1)
    if f.size < 2:
        return 0.0
    step = (f[-1] - f[0]) / (f.size - 1)
    if not step > 0.0 or not float(np.float32(step)) > 0.0:
        return 0.0
    tol = 2.0 * float(np.spacing(np.float32(np.abs(f).max())))
    return float(step) if np.all(np.abs(f - (f[0] + np.arange(f.size) * step)) <= tol) else 0.0


def _checked_phasor_setup(who, g, frequencies, weights, window):
    """What the phasor calls refuse in a geometry, a frequency table, weights and a window, without a GPU; returns (H, W, S, L,
    frequencies f32, weights f32 or None, (tau_min, tau_max))"""
    from .films.phasor_hdr_film import PhasorHDRFilm
    H, W, S, L = _checked_geometry(who, g)
    if not np.isfinite(np.float32(g.start_opl)):
        raise ValueError(f"{who}: start_opl must be finite, got {g.start_opl}")
    film = frequencies if isinstance(frequencies, PhasorHDRFilm) else None
    freq = np.ascontiguousarray(film.frequencies_f32 if film is not None else np.asarray(frequencies, dtype=np.float64).reshape(-1),
                                dtype=np.float32)
    F = int(freq.size)
    if F == 0 or not np.all(np.isfinite(freq)):
        raise ValueError(f"{who}: frequencies is a PhasorHDRFilm or a sequence of F >= 1 finite floats")
    if isinstance(weights, str):
        if weights != "gaussian":
            raise ValueError(f"{who}: weights must be None, an (F,) array or 'gaussian', not {weights!r}")
        if film is None:
            raise ValueError(f"{who}: weights='gaussian' needs the PhasorHDRFilm (its wl_mean and wl_sigma) as `frequencies`")
        w = np.exp(-0.5 * ((freq.astype(np.float64) - 1.0 / film.wl_mean) * (6.0 * film.wl_sigma)) ** 2).astype(np.float32)
    elif weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1), dtype=np.float32)
        if w.size != F or not np.all(np.isfinite(w)):
            raise ValueError(f"{who}: weights are {F} finite floats, one per frequency; got {w.size}")
    else:
        w = None
    if window is None:
        win = (-_FLT_MAX, _FLT_MAX)
    elif isinstance(window, str):
        if window != "capture":
            raise ValueError(f"{who}: window must be None, 'capture' or (lo, hi), not {window!r}")
        if not (int(g.temporal_bins) > 0 and g.bin_width_opl > 0.0):
            raise ValueError(f"{who}: window='capture' needs the geometry's temporal_bins and bin_width_opl")
        win = (0.0, float(g.temporal_bins) * float(g.bin_width_opl))
    else:
        win = tuple(float(v) for v in np.asarray(window, dtype=np.float64).reshape(-1))
        if len(win) != 2 or not win[0] <= win[1]:
            raise ValueError(f"{who}: window is (lo, hi) with lo <= hi, got {window!r}")
    return H, W, S, L, freq, w, win


def _checked_phasor_call(shape, is_complex, g, frequencies, weights, window, volume_min, volume_max, resolution, who="phasor_backproject"):
    """Everything ``phasor_backproject`` can refuse without a GPU; returns (S, L, frequencies f32, weights f32 or None,
    (tau_min, tau_max), vmin, vmax, (nx, ny, nz))"""
    H, W, S, L, freq, w, win = _checked_phasor_setup(who, g, frequencies, weights, window)
    F = int(freq.size)
    shape = tuple(int(v) for v in shape)
    if not is_complex:
        if len(shape) < 1 or shape[-1] != 2:
            raise ValueError(f"{who}: real phasors end in a (Re, Im) axis of 2, got {shape}; pass a complex tensor otherwise")
        shape = shape[:-1]
    if len(shape) not in (3, 5):
        raise ValueError(f"{who}: phasors are (H, W, F[, 2]), an exhaustive capture (H, W, Lx, Ly, F[, 2]); got {shape}")
    f_axis = _checked_rows(who, shape + (2,), g, H, W, L, ("(H, W, F[, 2])", "(H, W, Lx, Ly, F[, 2])"))      # (the frequency axis is the last)
    if shape[f_axis] != F:
        raise ValueError(f"{who}: the phasors have {shape[f_axis]} frequencies, the table {F}")
    vmin, vmax, res = _checked_box(who, volume_min, volume_max, resolution)
    return S, L, freq, w, win, vmin, vmax, res


class _PhasorProjection:
    """One geometry, one frequency table and one volume box on the device: what ``mtr_phasor_backproject`` and
    ``mtr_phasor_forward_project`` share in a call and in the autograd graph of a call.  ``run(entry, src)`` launches either on
    a contiguous f32 CUDA tensor of (Re, Im) pairs."""

    def __init__(self, ctx, g, S, L, freq, w, win, vmin, vmax, res, phasor_shape):
        import torch
        self.ctx, self.dev = ctx, torch.device("cuda", ctx.device_index)

        def dev_f32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)
        # (the six arrays live as long as this object: a graph that holds it can run its backward later)
        self.arrays = (dev_f32(g.sensor_points.reshape(-1, 3)), dev_f32(g.laser_points), dev_f32(g.sensor_offset.reshape(-1)),
                       dev_f32(g.laser_offset), dev_f32(freq), dev_f32(w) if w is not None else None)
        d = self.desc = _cabi.mtr_phasor_backproject_desc()
        d.capture_type, d.n_sensor, d.n_laser, d.n_freq = g.capture_type, S, L, int(freq.size)
        d.start_opl, d.freq_step = np.float32(g.start_opl), np.float32(uniform_frequency_step(freq))
        d.tau_min, d.tau_max = np.float32(win[0]), np.float32(win[1])
        for k in range(3):
            d.volume_min[k], d.volume_max[k] = np.float32(vmin[k]), np.float32(vmax[k])
        d.nx, d.ny, d.nz = res
        d.sensor_points, d.laser_points, d.sensor_offset, d.laser_offset, d.frequencies = (t.data_ptr() for t in self.arrays[:5])
        d.weights = self.arrays[5].data_ptr() if w is not None else None
        self.shapes = {"mtr_phasor_backproject": (res[2], res[1], res[0], 2), "mtr_phasor_forward_project": tuple(phasor_shape) + (2,)}

    def run(self, entry, src):
        import torch
        src = src.to(device=self.dev, dtype=torch.float32).contiguous()
        other = "mtr_phasor_forward_project" if entry == "mtr_phasor_backproject" else "mtr_phasor_backproject"
        if tuple(src.shape) != self.shapes[other]:
            raise ValueError(f"{entry}: the input has shape {tuple(src.shape)}, {self.shapes[other]} is expected")
        out = torch.empty(self.shapes[entry], dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            self.ctx.bind_current_stream()
            self.ctx.check(getattr(self.ctx.lib, entry)(self.ctx.handle, C.byref(self.desc), C.c_void_p(src.data_ptr()),
                                                        C.c_void_p(out.data_ptr())), entry)
        # (src is released to torch's caching allocator, which hands it out again in stream order)
        return out


_phasor_functions = None


def _phasor_autograd_pair():
    """(PhasorBackproject, PhasorForwardProject): the two kernels as torch.autograd.Functions on (Re, Im) pairs, each the other's
    backward.  The operators are conjugate transposes of one another (csrc/mtr_phasor_forward_project.h), and on the real view
    the transpose of a complex-linear map A is the real view of A^H: the views around them carry torch's complex convention."""
    global _phasor_functions
    if _phasor_functions is None:
        import torch

        class PhasorBackproject(torch.autograd.Function):
            @staticmethod
            def forward(fctx, phasors, projection):
                fctx.projection = projection
                return projection.run("mtr_phasor_backproject", phasors)

            @staticmethod
            def backward(fctx, grad_volume):
                return PhasorForwardProject.apply(grad_volume, fctx.projection), None

        class PhasorForwardProject(torch.autograd.Function):
            @staticmethod
            def forward(fctx, volume, projection):
                fctx.projection = projection
                return projection.run("mtr_phasor_forward_project", volume)

            @staticmethod
            def backward(fctx, grad_phasors):
                return PhasorBackproject.apply(grad_phasors, fctx.projection), None

        _phasor_functions = (PhasorBackproject, PhasorForwardProject)
    return _phasor_functions


def phasor_backproject(phasors, geometry, frequencies, volume_min, volume_max, resolution, weights=None, window=None):
    """Phasor-field reconstruction: propagate the phasors of a NLOS capture back into a complex volume of the hidden scene, on
    the GPU (``mtr_phasor_backproject``).

    ``phasors``: what ``mi.render`` returned for a scene with a ``phasor_hdr_film`` (used where it lies), a torch tensor or a
    numpy array, of shape (H, W, F, 2) or complex (H, W, F); an Exhaustive capture is (H, W, Lx, Ly, F[, 2]) (the renderer
    refuses that combination: such a tensor is hand-built).  ``geometry``: a :class:`CaptureGeometry` (:func:`capture_geometry`
    works on a scene with a phasor film).  ``frequencies``: the ``PhasorHDRFilm``, or a sequence of F floats.  ``weights``:
    ``None`` (ones), an (F,) array, or ``"gaussian"`` — ``exp(-1/2 ((f - 1 / wl_mean) / sigma_f)^2)`` with
    ``sigma_f = 1 / (6 wl_sigma)``, the band the film selected its frequencies from (needs the film).  ``window``: ``None``,
    ``"capture"`` (path lengths ``[0, temporal_bins * bin_width_opl]`` from ``start_opl``) or ``(lo, hi)``: pairs whose path
    length to a voxel lies outside do not contribute to it.

    Voxel ``v`` receives ``sum over (s, l) in the window, sum over k, of w_k P[s, l, k] exp(+i 2 pi f_k tau)`` with
    ``tau = |P_s - v| + |v - P_l| + offsets - start_opl``.  A uniformly spaced table (:func:`uniform_frequency_step`) is walked
    by rotation between every 16th frequency; any other table evaluates every term.  Returns a ``complex64`` CUDA tensor
    (nz, ny, nx); the sum has a fixed order, the same call gives the same bits.  Shape, geometry and frequency-count mismatches
    raise ``ValueError`` before the GPU is touched.

    Autograd: a torch tensor that requires grad, complex (..., F) or the real view (..., F, 2), with grad enabled, gives a volume
    with a ``grad_fn`` — the backward pass is :func:`phasor_forward_project`, the conjugate transpose, and the gradient lands on
    the tensor that was handed in (the complex / real views are torch ops of the graph).  Any other input takes the same path
    as ever, gives the same bits and carries no graph.  The gradient of a ``phasor_hdr_film`` *render* on the NLOS tier is not
    offered: the chain from a phasor volume to a scene parameter stops at the phasors."""
    from .tensor import TensorXf
    if isinstance(phasors, TensorXf):
        phasors = phasors.torch()
    if not hasattr(phasors, "shape"):
        phasors = np.asarray(phasors)
    is_complex = phasors.is_complex() if hasattr(phasors, "is_complex") else np.iscomplexobj(phasors)
    g = geometry
    S, L, freq, w, win, vmin, vmax, res = _checked_phasor_call(phasors.shape, is_complex, g, frequencies, weights, window,
                                                               volume_min, volume_max, resolution)
    from .runtime import get_context
    ctx = get_context()
    import torch
    t, wanted = _as_tensor(phasors)
    projection = _PhasorProjection(ctx, g, S, L, freq, w, win, vmin, vmax, res, tuple(t.shape[:-1] if not is_complex else t.shape))
    t = t.to(device=projection.dev)
    if is_complex:
        t = torch.view_as_real(t.resolve_conj())
    t = t.to(dtype=torch.float32).contiguous()
    volume = _phasor_autograd_pair()[0].apply(t, projection) if wanted else projection.run("mtr_phasor_backproject", t)
    return torch.view_as_complex(volume)


def phasor_forward_project(volume, geometry, frequencies, volume_min, volume_max, weights=None, window=None):
    """The conjugate transpose of :func:`phasor_backproject`: the phasors a complex volume of the hidden scene would produce, on
    the GPU (``mtr_phasor_forward_project``) — the forward model of a phasor-field reconstruction, its gradient, and the other
    half of :func:`phasor_reconstruct_cgls`.

    ``volume``: complex (nz, ny, nx), real (nz, ny, nx, 2) with a (Re, Im) axis, or real (nz, ny, nx) (an albedo volume, zero
    imaginary part); a torch tensor on any device, a numpy array or a ``TensorXf``.  The resolution is its shape, the box
    ``volume_min`` .. ``volume_max``.  ``frequencies``, ``weights`` and ``window`` exactly as in :func:`phasor_backproject`.
    Element ``(s, l, k)`` receives ``w_k sum over the voxels v in the window of U(v) exp(-i 2 pi f_k tau)`` — for a real
    non-negative volume the film's own convention, the phasors of a volume of scatterers without cosines and 1/r^2.  The factors
    are the conjugates of the ones ``phasor_backproject`` multiplies by, bit for bit, so that with the same arguments
    ``<phasor_backproject(y), x> = <y, phasor_forward_project(x)>`` up to f32 rounding.  Returns a ``complex64`` CUDA tensor
    (H, W, F); for an Exhaustive geometry (H, W, Lx, Ly, F) with (Lx, Ly) = ``geometry.laser_grid``.  The sums have a fixed order,
    the same call gives the same bits.

    Autograd: a volume that requires grad gives phasors with a ``grad_fn`` whose backward is ``phasor_backproject``; a real
    volume receives the real part of the gradient.  Refusals are ``ValueError`` before the GPU is touched."""
    who = "phasor_forward_project"
    from .tensor import TensorXf
    if isinstance(volume, TensorXf):
        volume = volume.torch()
    if not hasattr(volume, "shape"):
        volume = np.asarray(volume)
    is_complex = volume.is_complex() if hasattr(volume, "is_complex") else np.iscomplexobj(volume)
    g = geometry
    H, W, S, L, freq, w, win = _checked_phasor_setup(who, g, frequencies, weights, window)
    shape = tuple(int(v) for v in volume.shape)
    pairs = len(shape) == 4 and not is_complex
    if pairs and shape[-1] != 2:
        raise ValueError(f"{who}: a real 4-d volume ends in a (Re, Im) axis of 2, got {shape}")
    if len(shape) != (4 if pairs else 3) or min(shape) <= 0:
        raise ValueError(f"{who}: a complex or real (nz, ny, nx) or a real (nz, ny, nx, 2) volume is expected, got shape {shape}")
    if g.capture_type == _cabi.MTR_CAPTURE_EXHAUSTIVE:
        grid = g.laser_grid
        if grid is None:
            raise ValueError(f"{who}: an exhaustive geometry needs laser_grid = (Lx, Ly) to shape the phasors")
        grid = tuple(int(v) for v in grid)
        if len(grid) != 2 or grid[0] * grid[1] != L:
            raise ValueError(f"{who}: laser_grid {grid} does not match the geometry's {L} laser points")
        phasor_shape = (H, W, grid[0], grid[1], int(freq.size))
    else:
        phasor_shape = (H, W, int(freq.size))
    vmin, vmax, res = _checked_box(who, volume_min, volume_max, (shape[2], shape[1], shape[0]))
    from .runtime import get_context
    ctx = get_context()
    import torch
    t, wanted = _as_tensor(volume)
    projection = _PhasorProjection(ctx, g, S, L, freq, w, win, vmin, vmax, res, phasor_shape)
    t = t.to(device=projection.dev)
    if is_complex:
        t = torch.view_as_real(t.resolve_conj())
    elif not pairs:
        t = torch.stack((t, torch.zeros_like(t)), dim=-1)
    t = t.to(dtype=torch.float32).contiguous()
    out = _phasor_autograd_pair()[1].apply(t, projection) if wanted else projection.run("mtr_phasor_forward_project", t)
    return torch.view_as_complex(out)


def phasor_reconstruct_cgls(phasors, geometry, frequencies, volume_min, volume_max, resolution, iterations=10, weights=None, window=None):
    """Fit a complex hidden volume to measured phasors: CGLS on ``min |phasor_forward_project(x) - y|`` from ``x = 0``, one
    ``phasor_forward_project`` and one ``phasor_backproject`` per iteration on the GPU, the rest torch ops (the inner products
    are accumulated in float64).

    ``phasors``, ``frequencies``, ``weights`` and ``window`` as in :func:`phasor_backproject`.  Returns ``(volume, residuals)``:
    the ``complex64`` CUDA volume (nz, ny, nx) after ``iterations`` steps and ``residuals[k] = |r_k| / |y|`` as Python floats,
    ``k = 0 .. iterations`` (``residuals[0] = 1``).  The result carries no graph.  Phasors that are all zero return a zero
    volume.  Regularised solvers are out of scope."""
    who = "phasor_reconstruct_cgls"
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"{who}: iterations is a positive int, got {iterations!r}")
    from .tensor import TensorXf
    if isinstance(phasors, TensorXf):
        phasors = phasors.torch()
    if not hasattr(phasors, "shape"):
        phasors = np.asarray(phasors)
    is_complex = phasors.is_complex() if hasattr(phasors, "is_complex") else np.iscomplexobj(phasors)
    g = geometry
    S, L, freq, w, win, vmin, vmax, res = _checked_phasor_call(phasors.shape, is_complex, g, frequencies, weights, window,
                                                               volume_min, volume_max, resolution, who)
    from .runtime import get_context
    ctx = get_context()
    import torch
    with torch.no_grad():
        y = _as_tensor(phasors)[0]
        projection = _PhasorProjection(ctx, g, S, L, freq, w, win, vmin, vmax, res, tuple(y.shape[:-1] if not is_complex else y.shape))
        y = y.to(device=projection.dev)
        if is_complex:
            y = torch.view_as_real(y.resolve_conj())
        y = y.to(dtype=torch.float32).contiguous()

        def dot(a):                                 # <a, a> of a complex tensor held as (Re, Im) pairs
            return float(torch.sum(a.double() * a.double()))
        r = y.clone()
        s = projection.run("mtr_phasor_backproject", r)
        x, p = torch.zeros_like(s), s.clone()
        gamma, norm_y = dot(s), dot(y) ** 0.5
        residuals = [1.0]
        for _ in range(int(iterations)):
            if gamma == 0.0:                        # (converged, or y = 0)
                residuals.append(residuals[-1])
                continue
            q = projection.run("mtr_phasor_forward_project", p)
            alpha = gamma / dot(q)
            x += alpha * p
            r -= alpha * q
            s = projection.run("mtr_phasor_backproject", r)
            gamma, last = dot(s), gamma
            p = s + (gamma / last) * p
            residuals.append(dot(r) ** 0.5 / norm_y)
    return torch.view_as_complex(x), residuals


# ---------------------------------------------------------------- f-k migration
@dataclass
class _FkPlan:
    """What one ``fk_migration`` call computes on, all of it known without a GPU"""
    H: int
    W: int
    T: int
    q: int
    depth_bins: int               # T'
    z_begin: int
    nz: int
    ax: float
    ay: float
    dz: float                     # depth of one sample: q bin_width / 2
    shift: np.ndarray             # (H, W) int32

    def desc(self):
        d = _cabi.mtr_fk_desc()
        d.height, d.width, d.temporal_bins, d.bin_factor = self.H, self.W, self.T, self.q
        d.depth_bins, d.z_begin, d.nz = self.depth_bins, self.z_begin, self.nz
        d.ax, d.ay = np.float32(self.ax), np.float32(self.ay)
        return d

    def depths(self):
        return (np.arange(self.z_begin, self.z_begin + self.nz, dtype=np.float64) + 0.5) * self.dz


def _next_5_smooth(n):
    """the smallest integer >= n whose prime factors are 2, 3 and 5 (sizes the FFT libraries have fast paths for)"""
    n = max(int(n), 1)
    best = 1
    while best < n:
        best *= 2
    p5 = 1
    while p5 < best:
        p35 = p5
        while p35 < best:
            v = p35
            while v < n:
                v *= 2
            best = min(best, v)
            p35 *= 3
        p5 *= 5
    return best


def _fk_plan(who, g, depth_range=None, bin_factor=1):
    """Everything f-k migration can refuse in a geometry and its options without a GPU, and the grid it would run on"""
    H, W, S, L = _checked_geometry(who, g)
    if g.capture_type != _cabi.MTR_CAPTURE_CONFOCAL:
        raise ValueError(f"{who}: f-k migration needs a confocal capture, this one is {_CAPTURE_NAMES[g.capture_type]} "
                         "(backproject takes every capture type)")
    if H < 2 or W < 2:
        raise ValueError(f"{who}: the scan must be at least 2 x 2 points, got {H} x {W}")
    T = int(g.temporal_bins)
    if T <= 0:
        raise ValueError(f"{who}: a capture of zero size")
    bw = float(g.bin_width_opl)
    if not (bw > 0.0 and np.isfinite(bw) and np.isfinite(g.start_opl)):
        raise ValueError(f"{who}: bin_width_opl must be positive and start_opl finite, got {g.bin_width_opl} and {g.start_opl}")
    if isinstance(bin_factor, bool) or not isinstance(bin_factor, (int, np.integer)):
        raise ValueError(f"{who}: bin_factor must be an integer, got {bin_factor!r}")
    q = int(bin_factor)
    if q < 1:
        raise ValueError(f"{who}: bin_factor must be at least 1, got {q}")
    P = g.sensor_points
    if not np.all(np.isfinite(P)):
        raise ValueError(f"{who}: sensor_points must be finite")
    ex, ey = P[0, 1] - P[0, 0], P[1, 0] - P[0, 0]
    dx, dy = float(np.linalg.norm(ex)), float(np.linalg.norm(ey))
    tol = 1e-6 * max(dx, dy)
    grid = P[0, 0] + np.arange(W)[None, :, None] * ex + np.arange(H)[:, None, None] * ey
    if not (dx > 0.0 and dy > 0.0) or float(np.max(np.linalg.norm(P - grid, axis=-1))) > tol or abs(float(ex @ ey)) > 1e-6 * dx * dy:
        raise ValueError(f"{who}: the scan points must form an orthogonal affine grid P0 + x ex + y ey (a planar wall scanned in "
                         "equal steps); backproject takes any points")
    off = g.sensor_offset.reshape(H, W) + g.laser_offset.reshape(H, W)
    if not np.all(np.isfinite(off)):
        raise ValueError(f"{who}: the offsets must be finite")
    shift = np.rint((float(g.start_opl) - off) / bw)
    if float(np.max(np.abs(shift))) > 2.0 ** 30:
        raise ValueError(f"{who}: the capture starts more than 2^30 bins from the wall")
    zmin, zmax = 0.0, np.inf
    if depth_range is not None:
        try:
            lo, hi = depth_range
        except (TypeError, ValueError):
            raise ValueError(f"{who}: depth_range is (zmin, zmax), got {depth_range!r}") from None
        zmin = 0.0 if lo is None else float(lo)
        zmax = np.inf if hi is None else float(hi)
        if np.isnan(zmin) or np.isnan(zmax) or not zmax > zmin:
            raise ValueError(f"{who}: an empty depth_range {depth_range!r}")
        if not zmax > 0.0:
            raise ValueError(f"{who}: depth_range {depth_range!r} lies behind the wall")
    dz = q * bw / 2.0
    n = -(-(T + max(int(shift.max()), 0)) // q)
    if np.isfinite(zmax):
        n = min(n, max(int(np.ceil(zmax / dz)), 1))
    Tp = _next_5_smooth(n)
    centres = (np.arange(Tp, dtype=np.float64) + 0.5) * dz
    keep = np.nonzero((centres >= zmin) & (centres <= zmax))[0]
    if keep.size == 0:
        raise ValueError(f"{who}: no depth sample of the capture has its centre inside depth_range {depth_range!r} "
                         f"(the samples are {dz} apart and end at {Tp * dz})")
    if H > 0x7fff or W > 0x7fff or Tp > 0x3fffffff:
        raise ValueError(f"{who}: the scan or the depth grid is too large for one call")
    return _FkPlan(H, W, T, q, Tp, int(keep[0]), int(keep.size), dz / dx, dz / dy, dz, shift.astype(np.int32))


def fk_depths(geometry, depth_range=None, bin_factor=1):
    """The (nz,) depth centres, as float64 numpy, of the volume :func:`fk_migration` returns for the same arguments:
    ``(k + 1/2) bin_factor bin_width_opl / 2`` for the depth samples ``k`` whose centres lie inside ``depth_range``."""
    return _fk_plan("fk_depths", geometry, depth_range, bin_factor).depths()


def fk_migration(transient, geometry, depth_range=None, bin_factor=1, channel=None):
    """f-k migration (Lindell, Wetzstein, O'Toole 2019) of a confocal capture of a planar wall, on the GPU: the closed-form
    ``N^3 log N`` reconstruction of the case whose direct sum (:func:`backproject`) costs ``H W nx ny nz``.

    ``transient``: what ``mi.render`` returned (used where it lies, no host copy), a torch tensor or a numpy array, of shape
    (H, W, T) or (H, W, T, C); channels are averaged unless ``channel=k`` picks one.  ``geometry``: a Confocal
    :class:`CaptureGeometry` whose ``sensor_points`` form an orthogonal affine grid ``P0 + x ex + y ey`` (checked to 1e-6 of
    the larger spacing), at least 2 x 2.

    Time origin: bin ``b`` of scan point (y, x) is taken as wall-to-wall bin ``b + shift[y, x]`` with ``shift = round((start_opl -
    sensor_offset - laser_offset) / bin_width_opl)``, an integer: the capture is moved by whole bins, never resampled.  The
    residue is at most half a bin of path length, which is at most ``bin_width_opl / 4`` of depth.  ``bin_factor = q`` adds
    ``q`` consecutive wall-to-wall bins before the migration (f32, in increasing order).

    Returns a CUDA f32 tensor (nz, H, W): voxel (iz, iy, ix) sits at ``sensor_points[iy, ix] + n z`` with ``n`` the wall's
    normal and ``z = fk_depths(...)[iz] = (k + 1/2) q bin_width_opl / 2`` — the method cannot tell the two sides of the wall apart
    and does not need to.  The depth grid has ``T'`` samples, the next 5-smooth integer at or above ``ceil((T + max(shift, 0)) /
    q)``; ``depth_range = (zmin, zmax)`` keeps the samples whose centres lie inside it (either end may be None), and a ``zmax``
    also shortens ``T'`` to what covers it.  The steps: ``sqrt(max(S, 0)) (k + 1/2) / T'`` zero-padded to (2H, 2W, 2T')
    (``mtr_fk_prepare``), ``torch.fft.rfftn``, the Stolt resampling with linear interpolation and the Jacobian ``kz / k'``
    (``mtr_fk_stolt``), ``torch.fft.ifftn``, ``|.|^2`` of the low corner (``mtr_fk_finish``).  No atomics: the same call
    gives the same bits.

    Device memory: with ``N = 2H 2W 2T'``, the padded input (4N bytes) and its half spectrum (about 4N) are alive together, then
    the half spectrum and the resampled spectrum (8N), then the resampled spectrum and the field (8N): 16N bytes at the peak,
    plus the FFT's own workspace (up to the size of its output; where torch returns a transform with permuted strides, a
    contiguous copy of it as well) and the (nz, H, W) volume.  A 256 x 256 x 4096 capture that
    starts 3789 bins from the wall has ``T' = 2000`` with ``bin_factor=4`` and peaks near 16 GiB; with ``bin_factor=1``,
    ``T' = 8000`` and 63 GiB.  ``depth_range=(None, zmax)`` is what shrinks it.

    Not differentiable: a tensor that requires grad raises (detach it yourself if that is what you mean).  ``ValueError``
    before the GPU is touched also for a geometry that is not a Confocal ``CaptureGeometry`` on such a grid, a shape or
    ``temporal_bins`` mismatch, a ``bin_factor`` that is not an integer >= 1, and a ``depth_range`` that is empty or behind the
    wall."""
    who = "fk_migration"
    from .tensor import TensorXf
    if isinstance(transient, TensorXf):
        transient = transient.torch()
    if not hasattr(transient, "shape"):
        transient = np.asarray(transient)
    plan = _fk_plan(who, geometry, depth_range, bin_factor)
    shape = tuple(int(v) for v in transient.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"{who}: a confocal capture is (H, W, T) or (H, W, T, C), got {shape}")
    if shape[:2] != (plan.H, plan.W):
        raise ValueError(f"{who}: the capture is {shape[0]} x {shape[1]} scan points, the geometry {plan.H} x {plan.W}")
    if shape[2] != plan.T:
        raise ValueError(f"{who}: the capture has {shape[2]} time bins, the geometry {plan.T}")
    has_c = len(shape) == 4
    if channel is not None:
        if not has_c:
            raise ValueError(f"{who}: channel= needs a capture with a channel axis")
        if not 0 <= int(channel) < shape[-1]:
            raise ValueError(f"{who}: channel {channel} is outside the capture's {shape[-1]} channels")
    if has_c and shape[-1] == 0:
        raise ValueError(f"{who}: a capture without channels")
    if getattr(transient, "requires_grad", False):
        raise ValueError(f"{who}: the capture requires grad, and f-k migration is not differentiable here; pass "
                         "transient.detach() if the volume is all you want (backproject carries a graph)")

    from .runtime import get_context
    ctx = get_context()
    import torch
    dev = torch.device("cuda", ctx.device_index)
    t = transient if isinstance(transient, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(transient))
    t = t.to(device=dev, dtype=torch.float32)
    if has_c:
        t = t[..., int(channel)] if channel is not None else (t[..., 0] if t.shape[-1] == 1 else t.mean(dim=-1))
    t = t.contiguous()
    return _fk_run(ctx, plan, t)


def _fk_run(ctx, plan, capture):
    """the five steps of a planned call on a contiguous f32 CUDA (H, W, T) capture"""
    import torch
    dev = capture.device
    H, W, Tp = plan.H, plan.W, plan.depth_bins
    desc = plan.desc()
    shift = torch.from_numpy(plan.shift).to(dev)

    def launch(entry, *tensors):
        ctx.bind_current_stream()
        ctx.check(getattr(ctx.lib, entry)(ctx.handle, C.byref(desc), *(C.c_void_p(x.data_ptr()) for x in tensors)), entry)

    with torch.cuda.device(dev), torch.no_grad():
        padded = torch.empty((2 * H, 2 * W, 2 * Tp), dtype=torch.float32, device=dev)
        launch("mtr_fk_prepare", capture, shift, padded)
        spectrum = torch.fft.rfftn(padded).contiguous()       # (torch may hand a multi-axis transform back with permuted strides: then a copy)
        del padded
        resampled = torch.empty((2 * H, 2 * W, 2 * Tp), dtype=torch.complex64, device=dev)
        launch("mtr_fk_stolt", spectrum, resampled)
        del spectrum
        field = torch.fft.ifftn(resampled).contiguous()
        del resampled
        volume = torch.empty((plan.nz, H, W), dtype=torch.float32, device=dev)
        launch("mtr_fk_finish", field, volume)
    return volume
