#!/usr/bin/env python
"""Decodes the two AoLP (angle of linear polarization) figures of mitransient's polarization examples —
examples/polarization/render_cbox_polarized_and_visualization.ipynb, cell 11: ``plt.imshow(aolp[..., 120, :])``, time bin 120 of
a 4096 spp transient render; ..._steady.ipynb, cell 13: ``plt.imshow(aolp.squeeze())`` of Mitsuba's own `stokes` + `path`
render, 4096 spp — both of cornell-box/cbox_polarized{,_steady}.xml at 256 x 256 pixels in llvm_ad_mono_polarized — into the
data fixture ``tests/golden/polarized_figures.npz``.

``aolp`` is the second array of ``polarization_generate_false_color`` (polarized_visualization.py:232-290): per pixel
255 * (max(-s1, 0) + max(s2, 0), max(s1, 0) + max(s2, 0), max(-s2, 0)) with s_k = S_k / max(S0, 0.01).  matplotlib clips a float
RGB image to [0, 1], so a figure channel shows min(1, 255 s) of its sign: 255 (saturated) as soon as |S_k| >= max(S0, 0.01) / 255.
Stored per figure: the 8-bit RGB of the axes' interior resampled to the 256 x 256 data grid by averaging the figure pixels whose
centres fall in each data cell.  Run where the reference tree is available; the tests only read the .npz
(tests/test_polarized.py, tests/test_gpu_polarized.py)."""
import base64
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/examples/polarization"
RES = 256                                        # <default name="res" value="256"/>
FIGURES = [("render_cbox_polarized_and_visualization.ipynb", 11, "transient_bin120"),
           ("render_cbox_polarized_and_visualization_steady.ipynb", 13, "steady")]


def cell_png(nb, cell):
    d = json.load(open(os.path.join(REF, nb)))
    for o in d["cells"][cell].get("outputs", []):
        if "image/png" in o.get("data", {}):
            return np.array(Image.open(io.BytesIO(base64.b64decode(o["data"]["image/png"]))).convert("RGB"))
    raise RuntimeError(f"{nb} cell {cell}: no PNG output")


def axes_interior(rgb):
    """the axes box: rows / columns that are non-white over most of the figure's extent, minus the dark spine lines"""
    nonwhite = rgb.astype(np.int32).sum(-1) < 750
    rows = np.nonzero(nonwhite.mean(1) > 0.6)[0]
    cols = np.nonzero(nonwhite.mean(0) > 0.6)[0]
    y0, y1, x0, x1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
    v = rgb.astype(np.int32).sum(-1) / 3.0
    while v[y0, x0:x1].mean() > 200: y0 += 1
    while v[y1 - 1, x0:x1].mean() > 200: y1 -= 1
    while v[y0:y1, x0].mean() > 200: x0 += 1
    while v[y0:y1, x1 - 1].mean() > 200: x1 -= 1
    return y0 + 1, y1 - 1, x0 + 1, x1 - 1


def to_grid(rgb, box, n=RES):
    y0, y1, x0, x1 = box
    sub = rgb[y0:y1, x0:x1].astype(np.float64)
    iy = np.minimum(((np.arange(y1 - y0) + 0.5) * n / (y1 - y0)).astype(int), n - 1)
    ix = np.minimum(((np.arange(x1 - x0) + 0.5) * n / (x1 - x0)).astype(int), n - 1)
    out = np.zeros((n, n, 3)); cnt = np.zeros((n, n, 1))
    np.add.at(out, (iy[:, None], ix[None, :]), sub)
    np.add.at(cnt, (iy[:, None], ix[None, :]), 1.0)
    return np.round(out / cnt).astype(np.uint8)


def main():
    arrays, meta = {}, {}
    for nb, cell, name in FIGURES:
        rgb = cell_png(nb, cell)
        box = axes_interior(rgb)
        arrays[name] = to_grid(rgb, box)
        meta[name] = dict(notebook=f"examples/polarization/{nb}", cell=cell, spp=4096, res=RES, figure_box=[int(v) for v in box],
                          figure_size=[int(rgb.shape[0]), int(rgb.shape[1])],
                          display="aolp of polarization_generate_false_color, float RGB clipped to [0, 1], 8 bit")
    np.savez_compressed(os.path.join(HERE, "polarized_figures.npz"), meta=json.dumps(meta), **arrays)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
