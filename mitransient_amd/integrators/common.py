"""``TransientADIntegrator``: host orchestration of a transient render.

Mirrors mitransient/integrators/common.py — ``__init__`` (:22-30), ``prepare`` (:32-85),
``render`` (:122-213), ``add_transient_f`` (:411-422), ``check_transient_`` (:424-447) —
with the Dr.Jit trace replaced by launches of the HIP library: ``sample_rays`` +
``sample`` + the film splats of one pass are ONE call to ``mtr_render``.
``render_backward`` (:325-409) is the reverse mode over the constant diffuse reflectances and emitter radiances — with
``transient_nlos_path``, the projector's irradiance — (one call to ``mtr_render_grad`` per pass); ``render_forward`` (:215-323) is the forward mode over the same parameters of
``transient_path`` (one call to ``mtr_render_fwd``).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Tuple

from .. import _cabi, variant
from ..films.transient_hdr_film import TransientHDRFilm
from ..runtime import get_context
from ..scene import Properties
from ..tensor import TensorXf


def _dual_tangent(v):
    """the tangent of a ``torch.autograd.forward_ad`` dual tensor (inside its dual_level), else None"""
    try:
        import torch
        if not isinstance(v, torch.Tensor):
            return None
        return torch.autograd.forward_ad.unpack_dual(v).tangent
    except Exception:
        return None


def _wants_grad(v):
    """a value of ``params`` that is differentiated: it requires grad (reverse mode) or is a dual tensor (forward mode)"""
    return bool(getattr(v, "requires_grad", False)) or _dual_tangent(v) is not None


class _Seed:
    """stands for a value of ``params`` in check_grad_ when render_forward is given its tangent explicitly"""
    requires_grad = True

    def __init__(self, shape):
        self.shape = tuple(shape)


_MODES = {"auto": _cabi.MTR_MODE_AUTO, "fused": _cabi.MTR_MODE_FUSED, "wavefront": _cabi.MTR_MODE_WAVEFRONT,
          "samples": _cabi.MTR_MODE_SAMPLES}

# A scene whose sensor is a `radiancemeter` renders in the sample-parallel organisation when amd_mode is unset and the library's
# plan accepts the render (MTR_MODE_AUTO otherwise).  DESIGN.md §6 has the measurement this rests on.
RADIANCEMETER_DEFAULTS_TO_SAMPLES = True


class TransientADIntegrator:
    def __init__(self, props: Properties):
        # [mitsuba3: ADIntegrator.__init__] max_depth default 6 (-1 = infinite), rr_depth default 5
        max_depth = int(props.get("max_depth", 6))
        if max_depth < 0 and max_depth != -1:
            raise Exception("\"max_depth\" must be set to -1 (infinite) or a value >= 0")
        self.max_depth = max_depth if max_depth != -1 else 0xFFFFFFFF
        self.rr_depth = int(props.get("rr_depth", 5))
        if self.rr_depth <= 0:
            raise Exception("\"rr_depth\" must be set to a value greater than zero!")
        # hide_emitters: transientpath.py reads it in its "Hide the environment emitter" block after si.bsdf(ray) — a camera ray
        # (depth 0) that MISSES the scene stops being active when the flag is set, which only changes what an ENVIRONMENT emitter
        # would have contributed.  The subset has no environment emitter (a miss contributes nothing either way): parsed, kept,
        # without effect here
        self.hide_emitters = bool(props.get("hide_emitters", False))
        # common.py:25-30
        self.camera_unwarp = bool(props.get("camera_unwarp", False))
        self.discard_direct_light = bool(props.get("discard_direct_light", False))
        _ = props.get("gaussian_stddev", 0.5)      # accepted and ignored, as in the reference
        _ = props.get("temporal_filter", "")
        _ = props.get("block_size", 0)
        # sampler seeding variant (extension; see MTR_FLAG_PCG_INITSEQ_PLUS_LANE in the header): False = TEA(seed, lane) only
        self.pcg_initseq_plus_lane = bool(props.get("amd_pcg_initseq_plus_lane", False))
        # ... and the 64-bit reading of the same call site (MTR_FLAG_PCG_TEA64)
        self.pcg_tea64 = bool(props.get("amd_pcg_tea64", False))
        # order-independent (fixed-point) accumulation in the fused kernel: bit-reproducible renders (extension)
        self.deterministic = bool(props.get("amd_deterministic", False))
        # single-pass film lifecycle (extension): when one pass of the fused kernel renders all samples of all pixels, let its
        # row flush store the developed (H,W,T,3) tensor directly — no cleared 4-channel block, no develop pass.  Same values
        # (the weight channel is 0: develop divides by 1).  False keeps the reference's clear / accumulate / develop steps.
        self.direct_develop = bool(props.get("amd_direct_develop", True))
        # compute units left WITHOUT a workgroup of the persistent fused kernel (extension; mtr_render_params.reserve_cus): room for
        # the kernels of other streams — RCCL's film reduction of the previous row band — while a band renders.  0 on one GPU.
        self.reserve_cus = int(props.get("amd_reserve_cus", 0))
        # shadow rays of the fused kernel skip the rectangles they provably cannot hit (extension; MTR_SHADOW_HULL_SHIFT): the guard
        # distances of that proof times this margin.  1: as derived; larger (whole numbers up to 65535): only more careful, the same
        # picture bit for bit; 0: off
        m = props.get("amd_shadow_hull_margin", 1)
        if not (m == 0 or 1 <= m <= 65535):
            raise Exception("\"amd_shadow_hull_margin\" must be 0 (off) or a value in [1, 65535]")
        self.shadow_hull_margin = 0 if m == 0 else int(math.ceil(m))
        self.mode = _cabi.MTR_MODE_AUTO            # kernel organisation (extension; not a reference key)
        m = props.get("amd_mode", None)
        if m is not None:
            self.mode = _MODES[m]
        self.max_wavefront_size = 2 ** 32          # common.py:51: lanes of one pass
        self.pass_wavefront_size = 2 ** 26 - 1     # common.py:60: lanes per pass once the render is split
        self.last_counters = None      # counters / kernel times of the last mtr_render call ...
        self.last_times = None
        self.total_counters = None     # ... and summed over every pass since the last prepare()
        self.total_times = None
        self.collect_stats = False

    @property
    def amd_mode(self):
        """kernel organisation (extension): "auto" | "fused" | "wavefront" | "samples" (a pixel's samples spread over workgroups:
        films of one or a few pixels with very many samples; transient_path, plain transient_hdr_film)"""
        return {v: k for k, v in _MODES.items()}[int(self.mode)]

    @amd_mode.setter
    def amd_mode(self, m):
        self.mode = _MODES[m]

    def aov_names(self):
        return []

    # -- common.py:32-85 ---------------------------------------------------
    def prepare(self, scene, sensor, seed, spp, aovs, _direct_develop=False):
        film = sensor.film()
        if hasattr(film, "direct_develop"):
            film.direct_develop = bool(_direct_develop)      # only render() asks for the single-pass lifecycle
        sampler = sensor.sampler().clone()
        if spp != 0:
            sampler.set_sample_count(spp)
        spp = sampler.sample_count()
        sampler.set_samples_per_wavefront(spp)
        film_size = film.crop_size()
        self.total_counters, self.total_times = None, None
        n_pixels = film_size[0] * film_size[1]
        wavefront_size = n_pixels * spp
        if wavefront_size > self.max_wavefront_size and int(self.pass_wavefront_size / n_pixels) == 0:
            raise Exception("Your film is too big. Please make it smaller.")      # (before the film's storage is allocated)
        film.prepare(aovs)
        return self._pass_samplers(sensor, sampler, seed, spp, n_pixels)

    def _pass_samplers(self, sensor, sampler, seed, spp, n_pixels):
        """prepare()'s samplers of the passes (common.py:51-85) for a sampler whose sample count is ``spp``"""
        wavefront_size = n_pixels * spp
        if wavefront_size <= self.max_wavefront_size:
            sampler.seed(seed, wavefront_size)
            return [(sampler, spp)]
        # common.py:56-85: more than 2^32 samples cannot run in one pass (32-bit lane index); the reference goes down to
        # 2^26 per pass, each pass with its own sampler whose seed is drawn from a seeder sampler
        spp_per_pass = int(self.pass_wavefront_size / n_pixels)
        if spp_per_pass == 0:
            raise Exception("Your film is too big. Please make it smaller.")
        needs_remainder = spp % spp_per_pass != 0
        num_passes = spp // spp_per_pass + 1 * needs_remainder
        sampler.set_sample_count(num_passes)
        sampler.set_samples_per_wavefront(num_passes)
        sampler.seed(seed, num_passes)
        import numpy as np
        seeds = (sampler.next_1d_first() * np.float32(2 ** 32)).astype(np.uint32)      # mi.UInt32(sampler.next_1d() * 2**32)

        def sampler_per_pass(i):
            spp_i = spp % spp_per_pass if (needs_remainder and i == num_passes - 1) else spp_per_pass
            clone = sensor.sampler().clone()
            clone.set_sample_count(spp_i)
            clone.set_samples_per_wavefront(spp_i)
            clone.seed(int(seeds[i]), n_pixels * spp_i)
            return clone, spp_i

        return [sampler_per_pass(i) for i in range(num_passes)]

    def check_transient_(self, scene, sensor):
        if isinstance(sensor, int):
            sensor = scene.sensors()[sensor]
        if not isinstance(sensor.film(), TransientHDRFilm):
            raise AssertionError("The film of the sensor must be of type transient_hdr_film or phasor_hdr_film")
        from ..sensors import RadianceMeter
        if isinstance(sensor, RadianceMeter) and variant.is_polarized():
            raise ValueError(f"{variant.get()}: a radiancemeter renders with the unpolarized variants only")

    def _samples_by_default(self, sensor):
        """amd_mode unset and the sensor a radiancemeter: ask the plan for the sample-parallel organisation first"""
        from ..sensors import RadianceMeter
        return RADIANCEMETER_DEFAULTS_TO_SAMPLES and int(self.mode) == _cabi.MTR_MODE_AUTO and isinstance(sensor, RadianceMeter)

    def add_transient_f(self, film, pos, ray_weight, sample_scale):
        """common.py:411-422: closure that pre-multiplies the sample scale and splats."""
        return (lambda spec, distance, wavelengths=None, active=None, laser_x=None, laser_y=None:
                film.add_transient_data(pos, distance, wavelengths, spec * sample_scale, ray_weight, active))

    def _flags(self):
        f = 0
        if self.camera_unwarp:
            f |= _cabi.MTR_FLAG_CAMERA_UNWARP
        if self.discard_direct_light:
            f |= _cabi.MTR_FLAG_DISCARD_DIRECT_LIGHT
        if self.pcg_initseq_plus_lane:
            f |= _cabi.MTR_FLAG_PCG_INITSEQ_PLUS_LANE
        if self.pcg_tea64:
            f |= _cabi.MTR_FLAG_PCG_TEA64
        if self.deterministic:
            if variant.is_polarized():          # (the polarized kernels sum f32 Stokes rows: no fixed-point rows)
                raise ValueError(f"{variant.get()}: amd_deterministic is not available with polarization "
                                 "(the Stokes film is summed with f32 atomics; render without amd_deterministic)")
            f |= _cabi.MTR_FLAG_DETERMINISTIC
        if variant.is_polarized():
            f |= _cabi.MTR_FLAG_POLARIZED         # Mueller throughput, Stokes film (wavefront organisation)
        m = int(self.shadow_hull_margin)
        f |= (_cabi.MTR_SHADOW_HULL_OFF if m == 0 else m - 1) << _cabi.MTR_SHADOW_HULL_SHIFT
        return f

    def render_params(self, film, seed_value, spp_total, spp_begin=0, spp_end=None,
                      pixel_begin=0, pixel_end=None, spp_scale=0) -> _cabi.mtr_render_params:
        p = _cabi.mtr_render_params()
        p.spp_total = spp_total
        p.spp_scale = spp_scale          # multi-pass renders: sample_scale = 1 / total_spp of all passes (common.py:173-175)
        p.spp_begin = spp_begin
        p.spp_end = spp_total if spp_end is None else spp_end
        cw, ch = film.crop_size()
        p.pixel_begin = pixel_begin
        p.pixel_end = cw * ch if pixel_end is None else pixel_end
        p.seed = seed_value & 0xFFFFFFFF
        p.max_depth = -1 if self.max_depth >= 0x7FFFFFFF else int(self.max_depth)
        p.rr_depth = int(self.rr_depth)
        p.flags = self._flags()
        p.mode = int(self.mode)
        p.reserve_cus = max(0, int(self.reserve_cus))
        return p

    # -- common.py:122-213 ---------------------------------------------------
    def render(self, scene, sensor=0, seed=0, spp=0, develop=True, evaluate=True,
               progress_callback=None, spp_range=None, pixel_range=None) -> Tuple[TensorXf, TensorXf]:
        if not develop:
            raise Exception("develop=True must be specified when invoking AD integrators")
        if isinstance(sensor, int):
            sensor = scene.sensors()[sensor]
        film = sensor.film()
        self.check_transient_(scene, sensor)
        direct = spp_range is None and pixel_range is None and self._direct_develop_ok(scene, sensor, spp)
        samplers_spps = self.prepare(scene=scene, sensor=sensor, seed=seed, spp=spp, aovs=self.aov_names(), _direct_develop=direct)
        total_spp = sum(s for _, s in samplers_spps)
        self.accumulate(scene, sensor, samplers_spps, total_spp, spp_range, pixel_range, progress_callback)
        return film.develop()

    def _direct_develop_ok(self, scene, sensor, spp):
        """one pass, every sample of every film pixel in one launch of the fused kernel with LDS rows: its row flush can
        store the developed tensor (MTR_FLAG_DEVELOPED_ROWS)"""
        film = sensor.film()
        if not self.direct_develop or type(film) is not TransientHDRFilm:
            return False
        if int(self.mode) == _cabi.MTR_MODE_SAMPLES or self._samples_by_default(sensor):
            return False                                    # the slabs' rows are ADDED into the raw block
        if tuple(film.crop_size()) != tuple(film.size()) or tuple(film.crop_offset()) != (0, 0):
            return False                                    # rows outside the crop window would never be written
        spp = spp if spp != 0 else sensor.sampler().sample_count()
        W, H = film.size()
        if W * H * spp > self.max_wavefront_size:
            return False                                    # split render: several passes add into the block
        ctx = get_context()
        handle = scene.gpu_handle(ctx, sensor)
        params = self.render_params(film, 0, spp)
        mode, ok = C.c_uint32(0), C.c_uint32(0)
        ctx.check(ctx.lib.mtr_render_plan(handle, C.byref(params), C.byref(mode), C.byref(ok)), "mtr_render_plan")
        return bool(ok.value)

    def accumulate(self, scene, sensor, samplers_spps, total_spp, spp_range=None, pixel_range=None,
                   progress_callback=None, rows_are_zero=None, defer_stats=None, developed_partial=False, bands=None):
        """The pass loop of render() (common.py:157-210) without prepare/develop: ADDS into the film.
        ``rows_are_zero``: the caller vouches that the film rows of ``pixel_range`` are untouched since clear() (a render
        split into disjoint row bands: every band's FIRST pass may store its rows instead of read-modify-write).
        ``defer_stats``: "first" / "more" — the call stays asynchronous (no counters / timings are read back); the device
        counters are reset by "first" and keep summing through "more"; read them with ``fetch_counters()``.
        ``bands``: (n, epoch, device pointer of n uint32 words) — band completion words of ONE fused launch over the whole pixel
        range (mtr_render_params.n_bands): word b receives ``epoch`` when band b's rows are in the film."""
        film = sensor.film()
        ctx = get_context(film._device.index)
        ctx.bind_current_stream()
        handle = scene.gpu_handle(ctx, sensor)
        # ``developed_partial``: the caller wants the developed (H,W,T,3) rows of THIS call's samples and pixels only — partial
        # sums it reduces itself (multi-GPU: a 3-channel reduce-scatter instead of a 4-channel one, no clear, no develop)
        direct = film.developed_storage() if hasattr(film, "developed_storage") else None
        if direct is not None and (len(samplers_spps) > 1 or ((spp_range is not None or pixel_range is not None) and not developed_partial)):
            direct = None
            film._ensure_raw()                    # (a direct-develop film asked to accumulate in parts: back to the block)
        tptr = C.c_void_p((direct if direct is not None else film.transient_storage.torch_tensor()).data_ptr())
        sptr = C.c_void_p(film.steady_accum().data_ptr())
        multi = len(samplers_spps) > 1
        if multi and spp_range is not None:
            raise NotImplementedError("sample sharding of a multi-pass (> 2^32 lanes) render: shard by rows instead")
        for i, (sampler_i, spp_i) in enumerate(samplers_spps):
            s0, s1 = (0, spp_i) if spp_range is None else spp_range
            p0, p1 = (0, None) if pixel_range is None else pixel_range
            # a pass of a split render indexes its lanes with ITS sample count (its own sampler) and scales by the total
            params = self.render_params(film, sampler_i.seed_value(), spp_i if multi else total_spp, s0, s1, p0, p1,
                                        spp_scale=total_spp if multi else 0)
            if bands is not None:
                if multi:
                    raise NotImplementedError("band completion words of a multi-pass render")
                params.n_bands, params.band_epoch, params.band_done = int(bands[0]), int(bands[1]) & 0xFFFFFFFF, int(bands[2])
            if direct is not None:
                params.flags |= _cabi.MTR_FLAG_DEVELOPED_ROWS  # the row flush stores the developed (H,W,T,3) rows whole
            elif film.film_is_zero or (rows_are_zero and i == 0):
                params.flags |= _cabi.MTR_FLAG_FILM_ZERO      # first pass after clear(): row flushes may store
            film.film_is_zero = False
            if bands is None and direct is None and self._samples_by_default(sensor):
                params.mode = _cabi.MTR_MODE_SAMPLES          # ... when the plan accepts it (a refusal: MTR_MODE_AUTO as before)
                if ctx.lib.mtr_render_plan(handle, C.byref(params), C.byref(C.c_uint32(0)), None) != 0:
                    params.mode = _cabi.MTR_MODE_AUTO
            stats_now = self.collect_stats and defer_stats is None
            if defer_stats == "more" or (defer_stats == "first" and i > 0):
                params.flags |= _cabi.MTR_FLAG_KEEP_COUNTERS
            cnt = _cabi.mtr_counters() if stats_now else None
            tim = _cabi.mtr_kernel_times() if stats_now else None
            ctx.check(ctx.lib.mtr_render(handle, C.byref(params), tptr, sptr,
                                         C.byref(cnt) if cnt is not None else None,
                                         C.byref(tim) if tim is not None else None), "mtr_render")
            if stats_now:
                self.last_counters, self.last_times = cnt.as_dict(), tim.as_dict()
                if self.total_counters is None:
                    self.total_counters = {k: 0 for k in self.last_counters if k != "reserved"}
                    self.total_times = {k: 0 for k in self.last_times}
                for k in self.total_counters:
                    self.total_counters[k] += self.last_counters[k]
                for k in self.total_times:
                    self.total_times[k] += self.last_times[k]
            if direct is not None:
                film._developed_written = True    # (a band of a banded render counts: its caller covers the other rows)
            if progress_callback:
                progress_callback((i + 1) / len(samplers_spps))

    def developed_rows_ok(self, scene, sensor, total_spp, spp_range=None, pixel_range=None):
        """would mtr_render honour MTR_FLAG_DEVELOPED_ROWS for this (partial) render of a plain transient_hdr_film?"""
        film = sensor.film()
        if not self.direct_develop or type(film) is not TransientHDRFilm:
            return False
        if int(self.mode) == _cabi.MTR_MODE_SAMPLES or self._samples_by_default(sensor):
            return False
        if tuple(film.crop_size()) != tuple(film.size()) or tuple(film.crop_offset()) != (0, 0):
            return False
        W, H = film.size()
        if W * H * total_spp > self.max_wavefront_size:
            return False
        ctx = get_context()
        handle = scene.gpu_handle(ctx, sensor)
        s0, s1 = (0, total_spp) if spp_range is None else spp_range
        p0, p1 = (0, None) if pixel_range is None else pixel_range
        params = self.render_params(film, 0, total_spp, s0, s1, p0, p1)
        mode, ok = C.c_uint32(0), C.c_uint32(0)
        ctx.check(ctx.lib.mtr_render_plan(handle, C.byref(params), C.byref(mode), C.byref(ok)), "mtr_render_plan")
        return bool(ok.value)

    def resolved_mode(self, scene, sensor, total_spp, spp_range=None, pixel_range=None):
        """the kernel organisation mtr_render would run (MTR_MODE_AUTO resolved by the library): "fused" | "wavefront"
        ("samples" on request, or by default for a radiancemeter).
        Callers that overlap several calls of one render on different streams need it: only the fused organisation
        keeps its per-launch state apart."""
        film = sensor.film()
        ctx = get_context(film._device.index)
        handle = scene.gpu_handle(ctx, sensor)
        s0, s1 = (0, total_spp) if spp_range is None else spp_range
        p0, p1 = (0, None) if pixel_range is None else pixel_range
        params = self.render_params(film, 0, total_spp, s0, s1, p0, p1)
        mode = C.c_uint32(0)
        if self._samples_by_default(sensor):
            params.mode = _cabi.MTR_MODE_SAMPLES
            if ctx.lib.mtr_render_plan(handle, C.byref(params), C.byref(mode), None) == 0:
                return "samples"
            params.mode = _cabi.MTR_MODE_AUTO
        ctx.check(ctx.lib.mtr_render_plan(handle, C.byref(params), C.byref(mode), None), "mtr_render_plan")
        return {v: k for k, v in _MODES.items()}[int(mode.value)]

    def reset_counters(self, film):
        """zero the device counters on the CURRENT stream (then every call of the render passes defer_stats="more")"""
        ctx = get_context(film._device.index)
        ctx.bind_current_stream()
        ctx.check(ctx.lib.mtr_counters_reset(ctx.handle), "mtr_counters_reset")

    def fetch_counters(self, film):
        """counters summed on the device over the deferred calls of one render (the caller synchronised their streams)"""
        ctx = get_context(film._device.index)
        cnt = _cabi.mtr_counters()
        ctx.check(ctx.lib.mtr_counters_read(ctx.handle, C.byref(cnt)), "mtr_counters_read")
        self.last_counters = cnt.as_dict()
        self.total_counters = {k: v for k, v in self.last_counters.items() if k != "reserved"}
        return self.total_counters

    # -- common.py:215-323 -----------------------------------------------------
    def render_forward(self, scene, params, sensor=0, seed=0, spp=0, tangents=None):
        """The tangent ``(steady (ch, cw, 3), transient (H, W, T, 3))`` of what ``render`` returns, for the seeded estimator with
        sampling detached — the transpose of ``render_backward``.  ``tangents``: ``{key: tensor}`` over the keys
        ``render_backward`` differentiates, ``(3,)`` (a 1-element value: all three channels) or the ``(H, W, 3)`` texels of a
        ``.data`` key; ``None``: the tangents of the values of ``params`` that are ``torch.autograd.forward_ad`` dual tensors.
        Every refusal is a ``NotImplementedError`` raised before any GPU work."""
        import numpy as np
        import torch
        from .transientnlospath import TransientNLOSPath
        if isinstance(self, TransientNLOSPath):
            raise NotImplementedError("transient_nlos_path: forward-mode differentiation is available with transient_path only "
                                      "(use render_backward)")
        if tangents is None:
            tangents = {k: t for k, t in ((k, _dual_tangent(v)) for k, v in (params or {}).items()) if t is not None}
        probe = {k: v for k, v in (params or {}).items() if _wants_grad(v)}
        probe.update({k: _Seed(getattr(t, "shape", ())) for k, t in tangents.items()})
        try:
            keys = self.check_grad_(scene, sensor, probe)
        except ValueError as e:
            raise NotImplementedError(f"render_forward: {e}") from e
        if isinstance(sensor, int):
            sensor = scene.sensors()[sensor]
        film = sensor.film()
        sampler = sensor.sampler().clone()
        if spp != 0:
            sampler.set_sample_count(spp)
        spp = sampler.sample_count()
        cw, ch = film.crop_size()
        if cw * ch * spp > self.max_wavefront_size:
            raise NotImplementedError("render_forward: a render of more than 2^32 lanes runs in several passes; forward-mode "
                                      "differentiation needs one (common.py:237-240)")
        sd = scene.data(sensor)
        first = np.cumsum([0] + [int(t.shape[0] * t.shape[1]) for t in sd.textures])
        n_m, n_e = max(1, sd.n_materials), max(1, sd.n_emitters)
        tm = np.zeros((n_m, 3), np.float32)
        te = np.zeros((n_e, 3), np.float32)
        tx = tt = None
        for k, t in tangents.items():
            kind, i = keys[k]
            t = np.asarray(t.detach().cpu() if hasattr(t, "detach") else t, dtype=np.float32)
            if kind == "tint":
                if t.size not in (1, 3):
                    raise NotImplementedError(f"render_forward: {k}: a tangent of 1 or 3 elements, got shape {t.shape}")
                if tt is None:
                    tt = np.zeros((max(1, scene.n_tint_slots(sensor)), 3), np.float32)
                tt[i] += t.reshape(-1)
            elif kind == "texture":
                if tx is None:
                    tx = np.zeros((max(1, int(first[-1])), 3), np.float32)
                tx[int(first[i]):int(first[i + 1])] += t.reshape(-1, 3)
            else:
                if t.size not in (1, 3):
                    raise NotImplementedError(f"render_forward: {k}: a tangent of 1 or 3 elements, got shape {t.shape}")
                (tm if kind == "material" else te)[i] += t.reshape(-1)
        if getattr(params, "_dirty", None):
            params.update()
        # -- GPU work from here on ------------------------------------------------
        sampler.set_samples_per_wavefront(spp)
        sampler.seed(seed, cw * ch * spp)
        W, H = film.size()
        T = film.temporal_bins
        dev = film._device if film._device is not None else torch.device("cuda", torch.cuda.current_device())
        ctx = get_context(dev.index)
        ctx.bind_current_stream()
        handle = scene.gpu_handle(ctx, sensor)
        d_tm, d_te = torch.from_numpy(tm).to(dev), torch.from_numpy(te).to(dev)
        d_tx = torch.from_numpy(tx).to(dev) if tx is not None else None
        steady = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        transient = torch.zeros((H, W, T, 3), dtype=torch.float32, device=dev)
        p = self.render_params(film, sampler.seed_value(), spp)
        if tt is not None:
            d_tt = torch.from_numpy(tt).to(dev)
            ctx.check(ctx.lib.mtr_render_fwd_tint(handle, C.byref(p), C.c_void_p(d_tm.data_ptr()), C.c_void_p(d_te.data_ptr()),
                                                  C.c_void_p(d_tx.data_ptr()) if d_tx is not None else None, C.c_void_p(d_tt.data_ptr()),
                                                  C.c_void_p(steady.data_ptr()), C.c_void_p(transient.data_ptr())), "mtr_render_fwd_tint")
            return TensorXf(steady[:ch, :cw].contiguous()), TensorXf(transient)
        ctx.check(ctx.lib.mtr_render_fwd(handle, C.byref(p), C.c_void_p(d_tm.data_ptr()), C.c_void_p(d_te.data_ptr()),
                                         C.c_void_p(d_tx.data_ptr()) if d_tx is not None else None,
                                         C.c_void_p(steady.data_ptr()), C.c_void_p(transient.data_ptr())), "mtr_render_fwd")
        return TensorXf(steady[:ch, :cw].contiguous()), TensorXf(transient)

    # -- common.py:325-409 -----------------------------------------------------
    def check_grad_(self, scene, sensor, params):
        """the refusals of the reverse mode (ValueError), all of them before any GPU work"""
        import numpy as np
        from ..films.phasor_hdr_film import PhasorHDRFilm
        from .transientnlospath import TransientNLOSPath
        v = variant.get() or ""
        if not v.endswith("_ad_rgb"):
            raise ValueError(f"{v}: differentiable rendering is available in the *_ad_rgb variants only")
        nlos = isinstance(self, TransientNLOSPath)
        if nlos:
            from ..emitters import Projector
            ems = scene.emitters()
            if len(ems) != 1 or not isinstance(ems[0], Projector):
                raise ValueError("transient_nlos_path: differentiable rendering needs a scene whose only emitter is a projector")
            if int(self.capture_type) == 3:
                raise ValueError("transient_nlos_path: differentiable rendering is not available for an Exhaustive capture "
                                 "(Single and Confocal are)")
        if isinstance(sensor, int):
            sensor = scene.sensors()[sensor]
        film = sensor.film()
        if isinstance(film, PhasorHDRFilm):
            raise ValueError("phasor_hdr_film: differentiable rendering needs a transient_hdr_film")
        if not isinstance(film, TransientHDRFilm):
            raise ValueError("differentiable rendering needs a transient_hdr_film")
        if film.exhaustive_scan:
            raise ValueError("transient_hdr_film with exhaustive_scan: differentiable rendering is not available")
        wanted = [k for k, val in (params or {}).items() if _wants_grad(val)]
        scene.ensure_own_records([k for k in wanted if k in scene.param_keys()], sensor)     # (albedo and tint keys)
        keys = dict(scene.grad_keys(sensor))
        keys.update({k: ("texture", i) for k, i in scene.texture_keys(sensor).items()})
        if not nlos:       # the specular tints (mtr_render_grad_tint): transient_path only
            keys.update({k: ("tint", i) for k, i in scene.tint_keys(sensor).items()})
        seen = {}
        for k, val in (params or {}).items():
            if not _wants_grad(val):
                continue
            if k not in keys:
                raise ValueError(f"{k}: not a differentiable parameter (the constant reflectance of a diffuse BSDF, the texels of a "
                                 f"bitmap that only diffuse reflectances use, the constant radiance of an area / angulararea "
                                 f"emitter, the constant intensity of a point / spot emitter and the constant irradiance of a NLOS scene's projector are; the constant specular "
                                 f"tints of conductors and dielectrics with transient_path only: {sorted(keys)})")
            if keys[k][0] == "tint" and int(np.prod(tuple(val.shape))) not in (1, 3):
                raise ValueError(f"{k}: a tint of 1 or 3 elements, got shape {tuple(val.shape)}")
            if keys[k][0] == "texture":
                if tuple(val.shape) != tuple(scene.data(sensor).textures[keys[k][1]].shape):
                    raise ValueError(f"{k}: expected texels of shape {tuple(scene.data(sensor).textures[keys[k][1]].shape)}, "
                                     f"got {tuple(val.shape)}")
                if keys[k] in seen:
                    raise ValueError(f"{k} and {seen[keys[k]]} name one bitmap: its gradient is one tensor, differentiate one key")
                seen[keys[k]] = k
        return keys

    def render_backward(self, scene, params, grad_in, sensor=0, seed=0, spp=0):
        """Gradients of  sum g_s . steady + sum g_t . transient  of the seeded estimator (``grad_in = (g_s, g_t)``, the upstream
        gradients of the developed (H, W, 3) / (H, W, T, 3) tensors) with respect to every value of ``params`` that requires grad:
        ``{key: torch.float32 (3,)}`` — ``(H, W, 3)`` for the texels of a ``.data`` key — on the render device.  Sampling is
        detached."""
        import numpy as np
        import torch
        keys = self.check_grad_(scene, sensor, params)
        wanted = [k for k, val in (params or {}).items() if getattr(val, "requires_grad", False)]
        if isinstance(sensor, int):
            sensor = scene.sensors()[sensor]
        film = sensor.film()
        if getattr(params, "_dirty", None):
            params.update()
        # the passes and seeds of render() (prepare, without touching the film: the primal's tensors stay as they are)
        sampler = sensor.sampler().clone()
        if spp != 0:
            sampler.set_sample_count(spp)
        spp = sampler.sample_count()
        sampler.set_samples_per_wavefront(spp)
        n_pixels = film.crop_size()[0] * film.crop_size()[1]
        if n_pixels * spp > self.max_wavefront_size and int(self.pass_wavefront_size / n_pixels) == 0:
            raise Exception("Your film is too big. Please make it smaller.")
        samplers_spps = self._pass_samplers(sensor, sampler, seed, spp, n_pixels)
        total_spp = sum(s for _, s in samplers_spps)
        W, H = film.size()
        cw, ch = film.crop_size()
        T = film.temporal_bins
        dev = film._device if film._device is not None else torch.device("cuda", torch.cuda.current_device())
        g_s, g_t = grad_in
        g_s = torch.zeros((ch, cw, 3), dtype=torch.float32, device=dev) if g_s is None else \
            torch.as_tensor(g_s.torch() if hasattr(g_s, "torch") else g_s).to(device=dev, dtype=torch.float32)
        g_t = torch.zeros((H, W, T, 3), dtype=torch.float32, device=dev) if g_t is None else \
            torch.as_tensor(g_t.torch() if hasattr(g_t, "torch") else g_t).to(device=dev, dtype=torch.float32)
        if tuple(g_s.shape) != (ch, cw, 3) or tuple(g_t.shape) != (H, W, T, 3):
            raise ValueError(f"render_backward: grad_in shapes {tuple(g_s.shape)}, {tuple(g_t.shape)}; expected "
                             f"{(ch, cw, 3)}, {(H, W, T, 3)}")
        # the steady gradient in the accumulator's layout: (H, W, 3), the crop window at the top-left corner (develop's view)
        gs_full = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        gs_full[:ch, :cw] = g_s
        g_t = g_t.contiguous()
        ctx = get_context(dev.index)
        ctx.bind_current_stream()
        handle = scene.gpu_handle(ctx, sensor)
        sd = scene.data(sensor)
        n_m, n_e = max(1, sd.n_materials), max(1, sd.n_emitters)
        gm = torch.zeros((n_m, 3), dtype=torch.float32, device=dev)
        ge = torch.zeros((n_e, 3), dtype=torch.float32, device=dev)
        pm = torch.empty_like(gm)
        pe = torch.empty_like(ge)
        # texel gradients only when a `.data` key asks: mtr_render_grad_tex, all textures' texels in scene order
        textured = any(keys[k][0] == "texture" for k in wanted)
        if textured:
            first = np.cumsum([0] + [int(t.shape[0] * t.shape[1]) for t in sd.textures])
            gx = torch.zeros((int(first[-1]), 3), dtype=torch.float32, device=dev)
            px = torch.empty_like(gx)
        # tint gradients only when a tint key asks: mtr_render_grad_tint, every slot of mtr_scene_tint_layout
        tinted = any(keys[k][0] == "tint" for k in wanted)
        if tinted:
            gtint = torch.zeros((max(1, scene.n_tint_slots(sensor)), 3), dtype=torch.float32, device=dev)
            ptint = torch.empty_like(gtint)
        multi = len(samplers_spps) > 1
        for sampler_i, spp_i in samplers_spps:
            p = self.render_params(film, sampler_i.seed_value(), spp_i if multi else total_spp, 0, spp_i, 0, None,
                                   spp_scale=total_spp if multi else 0)
            if tinted:
                ctx.check(ctx.lib.mtr_render_grad_tint(handle, C.byref(p), C.c_void_p(gs_full.data_ptr()), C.c_void_p(g_t.data_ptr()),
                                                       C.c_void_p(pm.data_ptr()), C.c_void_p(pe.data_ptr()),
                                                       C.c_void_p(px.data_ptr()) if textured else None, C.c_void_p(ptint.data_ptr())),
                          "mtr_render_grad_tint")
                gtint += ptint
                if textured:
                    gx += px
            elif textured:
                ctx.check(ctx.lib.mtr_render_grad_tex(handle, C.byref(p), C.c_void_p(gs_full.data_ptr()), C.c_void_p(g_t.data_ptr()),
                                                      C.c_void_p(pm.data_ptr()), C.c_void_p(pe.data_ptr()), C.c_void_p(px.data_ptr())),
                          "mtr_render_grad_tex")
                gx += px
            else:
                ctx.check(ctx.lib.mtr_render_grad(handle, C.byref(p), C.c_void_p(gs_full.data_ptr()), C.c_void_p(g_t.data_ptr()),
                                                  C.c_void_p(pm.data_ptr()), C.c_void_p(pe.data_ptr())), "mtr_render_grad")
            gm += pm
            ge += pe
        out = {}
        for k in wanted:
            kind, i = keys[k]
            if kind == "texture":
                out[k] = gx[int(first[i]):int(first[i + 1])].reshape(tuple(sd.textures[i].shape)).clone()
            elif kind == "tint":
                out[k] = gtint[i].clone()
            else:
                out[k] = (gm if kind == "material" else ge)[i].clone()
        return out

    def to_string(self):
        return f"{type(self).__name__}[\n  max_depth = {self.max_depth}, \n  rr_depth = {self.rr_depth}\n]"

    __str__ = __repr__ = to_string
