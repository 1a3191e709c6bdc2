"""Helpers to aim the laser of an NLOS scene.  Public names and argument order follow mitransient/nlos.py:5-70;
all three resolve to one world-space point and share ``_aim``.

``capture_geometry`` / ``backproject`` / ``laplacian_filter`` turn a rendered capture back into a volume of the hidden
scene: the sum runs in HIP (``mtr_backproject``, csrc/mtr_backproject.hip), torch is plumbing.  ``phasor_backproject`` does the
same for the phasors a ``phasor_hdr_film`` develops (``mtr_phasor_backproject``, csrc/mtr_phasor_backproject.hip)."""
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


def _checked_call(transient, g, volume_min, volume_max, resolution, interpolation, channel, filter):
    """Everything ``backproject`` can refuse without a GPU; returns (S, L, T, has a channel axis, vmin, vmax, (nx, ny, nz))"""
    if interpolation not in _INTERPOLATIONS:
        raise ValueError(f"backproject: interpolation must be 'nearest' or 'linear', not {interpolation!r}")
    if filter not in (None, "laplacian"):
        raise ValueError(f"backproject: filter must be None or 'laplacian', not {filter!r}")
    H, W, S, L = _checked_geometry("backproject", g)
    T = int(g.temporal_bins)
    if T <= 0:
        raise ValueError("backproject: a capture of zero size")
    if not g.bin_width_opl > 0.0:
        raise ValueError(f"backproject: bin_width_opl must be positive, got {g.bin_width_opl}")
    shape = tuple(int(v) for v in transient.shape)
    t_axis = _checked_rows("backproject", shape, g, H, W, L, ("(H, W, T) or (H, W, T, C)", "(H, W, Lx, Ly, T) or (H, W, Lx, Ly, T, C)"))
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
    vmin, vmax, res = _checked_box("backproject", volume_min, volume_max, resolution)
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

    A capture rendered in the frequency domain (``phasor_hdr_film``) is reconstructed by :func:`phasor_backproject`.
    Out of scope: autograd through ``backproject`` (the result carries no graph), LCT / f-k migration, non-rectangular relay
    walls in ``capture_geometry`` (a hand-built ``CaptureGeometry`` takes any points).
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


def _checked_phasor_call(shape, is_complex, g, frequencies, weights, window, volume_min, volume_max, resolution):
    """Everything ``phasor_backproject`` can refuse without a GPU; returns (S, L, frequencies f32, weights f32 or None,
    (tau_min, tau_max), vmin, vmax, (nx, ny, nz))"""
    from .films.phasor_hdr_film import PhasorHDRFilm
    who = "phasor_backproject"
    H, W, S, L = _checked_geometry(who, g)
    if not np.isfinite(np.float32(g.start_opl)):
        raise ValueError(f"{who}: start_opl must be finite, got {g.start_opl}")
    film = frequencies if isinstance(frequencies, PhasorHDRFilm) else None
    freq = np.ascontiguousarray(film.frequencies_f32 if film is not None else np.asarray(frequencies, dtype=np.float64).reshape(-1),
                                dtype=np.float32)
    F = int(freq.size)
    if F == 0 or not np.all(np.isfinite(freq)):
        raise ValueError(f"{who}: frequencies is a PhasorHDRFilm or a sequence of F >= 1 finite floats")
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
    vmin, vmax, res = _checked_box(who, volume_min, volume_max, resolution)
    return S, L, freq, w, win, vmin, vmax, res


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
    (nz, ny, nx) without a graph; the sum has a fixed order, the same call gives the same bits.  Shape, geometry and
    frequency-count mismatches raise ``ValueError`` before the GPU is touched."""
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
    dev = torch.device("cuda", ctx.device_index)
    t = phasors if isinstance(phasors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(phasors))
    t = t.detach().to(device=dev)
    if is_complex:
        t = torch.view_as_real(t.resolve_conj())
    t = t.to(dtype=torch.float32).contiguous()

    def dev_f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    sp, lp = dev_f32(g.sensor_points.reshape(-1, 3)), dev_f32(g.laser_points)
    so, lo = dev_f32(g.sensor_offset.reshape(-1)), dev_f32(g.laser_offset)
    fr, wt = dev_f32(freq), (dev_f32(w) if w is not None else None)
    volume = torch.empty((res[2], res[1], res[0], 2), dtype=torch.float32, device=dev)
    d = _cabi.mtr_phasor_backproject_desc()
    d.capture_type, d.n_sensor, d.n_laser, d.n_freq = g.capture_type, S, L, int(freq.size)
    d.start_opl, d.freq_step = np.float32(g.start_opl), np.float32(uniform_frequency_step(freq))
    d.tau_min, d.tau_max = np.float32(win[0]), np.float32(win[1])
    for k in range(3):
        d.volume_min[k], d.volume_max[k] = np.float32(vmin[k]), np.float32(vmax[k])
    d.nx, d.ny, d.nz = res
    d.sensor_points, d.laser_points, d.sensor_offset, d.laser_offset = sp.data_ptr(), lp.data_ptr(), so.data_ptr(), lo.data_ptr()
    d.frequencies, d.weights = fr.data_ptr(), (wt.data_ptr() if wt is not None else None)
    with torch.cuda.device(dev):
        ctx.bind_current_stream()
        ctx.check(ctx.lib.mtr_phasor_backproject(ctx.handle, C.byref(d), C.c_void_p(t.data_ptr()), C.c_void_p(volume.data_ptr())),
                  "mtr_phasor_backproject")
    # (t, sp .. wt are released to torch's caching allocator, which hands them out again in stream order)
    return torch.view_as_complex(volume)
