"""``mitransient.vis`` for the unpolarized variants (mitransient/unpolarized_visualization.py): host-side numpy /
matplotlib helpers the reference's notebooks call — ``tonemap_transient`` (:14-18), ``tonemap_grad_transient`` (:21-39),
``save_video`` (:42-62), ``save_frames`` (:65-77), ``show_video`` (:80-122), ``rainbow_visualization`` (:125-151).
Same names, arguments and results; nothing here touches the GPU."""
from __future__ import annotations

import os
import struct

import numpy as np


def _frame(a, axis, i):
    return np.take(a, i, axis=axis)


def to_srgb_uint8(img, srgb_gamma: bool = True):
    """linear float image -> uint8, with the sRGB transfer function (what ``mi.Bitmap.convert(UInt8, srgb_gamma=True)``
    and ``mi.util.convert_to_bitmap`` do)"""
    x = np.clip(np.nan_to_num(np.asarray(img, dtype=np.float64)), 0.0, 1.0)
    if srgb_gamma:
        x = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    out = np.rint(x * 255.0).astype(np.uint8)
    if out.ndim == 3 and out.shape[-1] == 1:
        out = np.repeat(out, 3, axis=-1)
    return out


def tonemap_transient(transient, scaling=1.0):
    """linear tonemap: divide by the 99th percentile of |transient|"""
    tnp = np.array(transient)
    return tnp / np.quantile(np.abs(tnp), 0.99) * scaling


def tonemap_grad_transient(transient, axis_video=2):
    """gradient video -> 'coolwarm' colours: values are normalised by the 99.9th percentile of their magnitude,
    clipped to [-1, 1] and looked up at (v + 1) / 2"""
    if axis_video != 2:
        raise AssertionError("axis_video must be 2")
    tnp = np.array(transient)
    if tnp.ndim == 4:
        tnp = tnp.mean(axis=-1)
    import matplotlib
    cmap = matplotlib.colormaps["coolwarm"] if hasattr(matplotlib, "colormaps") else __import__("matplotlib.cm").cm.get_cmap("coolwarm")
    v = np.clip(tnp.astype(np.float32) / np.float32(np.quantile(np.abs(tnp), 0.999)), -1.0, 1.0)
    return cmap((v + 1.0) / 2.0)[..., :3].astype(np.float32)


def save_video(path, transient, axis_video=2, fps=24, display_video=False):
    """the transient image as an .mp4 (OpenCV 'mp4v'), one frame per index of ``axis_video``"""
    try:
        import cv2
    except ImportError as e:                               # same hard dependency as the reference
        raise ImportError("save_video needs OpenCV (cv2)") from e
    transient = np.asarray(transient)
    h, w = _frame(transient, axis_video, 0).shape[:2]
    writer = cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"mp4v"), fps, (w, h))
    for i in range(transient.shape[axis_video]):
        writer.write(to_srgb_uint8(_frame(transient, axis_video, i))[:, :, ::-1])      # RGB -> BGR
    writer.release()
    if display_video:
        from IPython.display import Video, display
        return display(Video(path, embed=True, width=w, height=h))


def write_exr(path, img):
    """minimal OpenEXR 2 writer: scan lines, no compression, 32-bit float channels (alphabetical order, as the format
    requires); enough for ``save_frames`` without an EXR library"""
    img = np.asarray(img, dtype=np.float32)
    if img.ndim == 2:
        img = img[..., None]
    h, w, c = img.shape
    names = {1: ["Y"], 3: ["B", "G", "R"], 4: ["A", "B", "G", "R"]}.get(c)
    if names is None:
        raise ValueError("write_exr: 1, 3 or 4 channels")
    order = {"Y": 0, "R": 0, "G": 1, "B": 2, "A": 3}

    def attr(name, typ, payload):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload

    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iBBBBii", 2, 0, 0, 0, 0, 1, 1) for n in names) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    header = (attr("channels", "chlist", chlist) + attr("compression", "compression", b"\0") + attr("dataWindow", "box2i", box) +
              attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0") +
              attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) +
              attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    line_bytes = c * w * 4
    offset0 = 8 + len(header) + 8 * h
    with open(path, "wb") as fh:
        fh.write(struct.pack("<ii", 20000630, 2) + header)
        fh.write(b"".join(struct.pack("<Q", offset0 + y * (8 + line_bytes)) for y in range(h)))
        for y in range(h):
            fh.write(struct.pack("<ii", y, line_bytes))
            for n in names:
                fh.write(np.ascontiguousarray(img[y, :, order[n]]).tobytes())


def save_frames(data, folder, axis_video=2):
    """one ``NNN.exr`` per frame of ``data`` along ``axis_video``"""
    os.makedirs(folder, exist_ok=True)
    data = np.asarray(data)
    for i in range(data.shape[axis_video]):
        write_exr(os.path.join(folder, f"{i:03d}.exr"), _frame(data, axis_video, i))


def show_video(input_sample, axis_video=2, uint8_srgb=True, normalize=False):
    """plays the transient video inline (IPython / Jupyter): a matplotlib animation rendered to HTML5 video"""
    import matplotlib.animation as animation
    from IPython.display import HTML, display
    from matplotlib import pyplot as plt
    data = np.asarray(input_sample)
    peak = data.max()

    def picture(i):
        fr = _frame(data, axis_video, i)
        if normalize:
            fr = fr / peak
        return to_srgb_uint8(fr, srgb_gamma=True) if uint8_srgb else np.clip(fr, 0.0, 1.0)

    fig = plt.figure()
    im = plt.imshow(picture(0))
    plt.axis("off")

    def update(i):
        im.set_data(picture(i))
        return im

    ani = animation.FuncAnimation(fig, update, frames=data.shape[axis_video], repeat=False)
    display(HTML(ani.to_html5_video()))
    plt.close()


def rainbow_visualization(steady_state, data_transient, modulo, min_modulo, max_modulo,
                          max_time_bins=None, mode="peak_time_fusion", scale_fusion=1):
    """time-of-flight as colour (Jarabo 2012): each pixel's peak time bin picks a 'jet' colour; pixels whose peak bin
    falls in [min_modulo, max_modulo] modulo ``modulo`` form iso-time bands.  ``sparse_fusion``: bands show the steady
    image; ``rainbow_fusion``: bands show the colour; ``peak_time_fusion``: colour on the bands, steady image elsewhere."""
    import matplotlib
    jet = matplotlib.colormaps["jet"] if hasattr(matplotlib, "colormaps") else __import__("matplotlib.cm").cm.jet
    steady_state = np.asarray(steady_state)
    data_transient = np.asarray(data_transient)
    n_bins = data_transient.shape[2] if max_time_bins is None else max_time_bins
    peak_bin = data_transient.max(axis=-1).argmax(axis=-1)
    phase = peak_bin % modulo
    band = (phase >= min_modulo) & (phase <= max_modulo)
    colour = jet(peak_bin / n_bins)[..., :3]
    out = np.zeros_like(steady_state)
    if mode == "sparse_fusion":
        out[band] = steady_state[band] ** scale_fusion
    elif mode == "rainbow_fusion":
        out[band] = colour[band]
    elif mode == "peak_time_fusion":
        out[band] = colour[band]
        out[~band] = steady_state[~band] ** scale_fusion
    else:
        raise NotImplementedError("Mode not implemented")
    return out


# ---- the polarized variants (mitransient/polarized_visualization.py:193-290): Stokes arrays with S0..S3 on the last axis ----
def _stokes_ratio(stokes, k, s0_minimum):
    s = np.asarray(stokes)
    return s[..., k] / np.maximum(s[..., 0], s0_minimum)


def degree_of_polarization(stokes, s0_minimum=0.01):
    """|(S1, S2, S3)| / max(S0, s0_minimum), clipped to [0, 1]"""
    s = np.asarray(stokes)
    return np.clip(np.sqrt(s[..., 1] ** 2 + s[..., 2] ** 2 + s[..., 3] ** 2) / np.maximum(s[..., 0], s0_minimum), 0.0, 1.0)


def degree_of_linear_polarization(stokes, s0_minimum=0.01):
    """|(S1, S2)| / max(S0, s0_minimum), clipped to [0, 1]"""
    s = np.asarray(stokes)
    return np.clip(np.sqrt(s[..., 1] ** 2 + s[..., 2] ** 2) / np.maximum(s[..., 0], s0_minimum), 0.0, 1.0)


def degree_of_circular_polarization(stokes, s0_minimum=0.01):
    """|S3| / max(S0, s0_minimum), clipped to [0, 1]"""
    return np.clip(np.abs(_stokes_ratio(stokes, 3, s0_minimum)), 0.0, 1.0)


def polarization_generate_false_color(stokes, aolp_intensity_scaling=1.0, s0_minimum=0.01):
    """The false-colour maps of Wilkie and Weidlich, "A standardised polarisation visualisation for images" (2010), on a 0..255
    scale: (degree of polarization in red, angle of linear polarization, the same scaled by the degree of linear polarization,
    type of polarization, chirality).  The angle map encodes the signs of S1 / S0 (green positive, red negative) and S2 / S0
    (yellow positive, blue negative)."""
    dop, dolp, docp = (degree_of_polarization(stokes, s0_minimum), degree_of_linear_polarization(stokes, s0_minimum),
                       degree_of_circular_polarization(stokes, s0_minimum))
    pos = lambda x: np.maximum(x, 0.0)           # noqa: E731
    s1, s2, s3 = (_stokes_ratio(stokes, k, s0_minimum) for k in (1, 2, 3))
    dop_reds = dop[..., None] * np.array([255.0, 0.0, 0.0])
    aolp = 255.0 * (np.stack([pos(-s1), pos(s1), np.zeros_like(s1)], axis=-1) + np.stack([pos(s2), pos(s2), pos(-s2)], axis=-1))
    aolp_scaled = aolp * aolp_intensity_scaling * dolp[..., None]
    top = dolp[..., None] * np.array([22.0, 247.0, 247.0]) + docp[..., None] * np.array([252.0, 251.0, 10.0])
    chirality = 255.0 * np.stack([pos(s3), pos(s3), pos(-s3)], axis=-1) * docp[..., None]
    return dop_reds, aolp, aolp_scaled, top, chirality


class DisplayMethod:
    """where show_video_polarized sends the frames (the reference's enum of the same name)"""
    ShowVideo, SaveVideo, SaveFrames = 0, 1, 2


def show_video_polarized(stokes, degree_of_polarization, angle_of_polarization, type_of_polarization, chirality, save_path=None,
                         display_method=DisplayMethod.ShowVideo, fps=24, intensity_cutoff=0.9, gamma=1.1, show_false_color=True):
    """the transient Stokes video: S0 (tonemapped to its ``intensity_cutoff`` quantile, then ``gamma``), next to the false-colour
    maps when ``show_false_color``.  ShowVideo plays it inline as ``show_video`` does; SaveFrames writes one EXR per time bin
    under ``save_path``.  (SaveVideo, the reference's mp4 through OpenCV, is not available.)"""
    s = np.asarray(stokes, dtype=np.float64)
    s0 = s[..., 0]
    top = np.quantile(s0, intensity_cutoff) if s0.size else 1.0
    inten = np.clip(s0 / (top if top > 0 else 1.0), 0.0, 1.0) ** (1.0 / gamma)
    panels = [np.repeat(inten[..., None], 3, axis=-1)]
    if show_false_color:
        panels += [np.asarray(m, dtype=np.float64) / 255.0 for m in (degree_of_polarization, angle_of_polarization,
                                                                     type_of_polarization, chirality)]
    frames = np.concatenate(panels, axis=1)                     # (H, 5 W, T, 3): the panels side by side
    if display_method == DisplayMethod.SaveFrames:
        save_frames(frames.astype(np.float32), save_path, axis_video=2)
        return None
    if display_method == DisplayMethod.SaveVideo:
        raise NotImplementedError("show_video_polarized: DisplayMethod.SaveVideo (mp4 through OpenCV) is not available; "
                                  "use SaveFrames or ShowVideo")
    return show_video(frames, axis_video=2, uint8_srgb=False)
