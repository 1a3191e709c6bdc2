#!/usr/bin/env python
"""Decodes the four steady images of mitransient's angulararea tutorial — examples/angulararea-emitter/
render_{angular,area}_1light.ipynb, cells 4 (the XML's camera, 256 spp) and 7 (the camera of cell 6, 64 spp), rendered by
mitransient 1.2.0 on Mitsuba 3.6.4 at the XML's 200 x 200 pixels — into the data fixture ``tests/golden/angular_figures.npz``.

Each figure is ``plt.imshow((data_steady / np.max(data_steady)) ** (1 / 4.0))`` of an RGB array: matplotlib shows the three channels
as they are (clipped to [0, 1], 8 bits), so the figure's colours ARE the displayed values; no colour map is inverted.  Stored per
figure: the 8-bit RGB of the axes' interior (spines removed) resampled to the 200 x 200 data grid by averaging the figure pixels whose
centres fall in each data cell.  Run where the reference tree is available; the tests only read the .npz
(tests/test_angular_emitter.py, tests/test_gpu_angular_emitter.py)."""
import base64
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/examples/angulararea-emitter"
RES = 200                                        # <default name="res" value="200"/> of both XML files
FIGURES = [("angular", 4, "angular_view1"), ("angular", 7, "angular_view2"), ("area", 4, "area_view1"), ("area", 7, "area_view2")]


def cell_png(nb, cell):
    d = json.load(open(os.path.join(REF, f"render_{nb}_1light.ipynb")))
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
    # the frame: anti-aliased light lines, then ONE black spine line, along each edge of the box
    v = rgb.astype(np.int32).sum(-1) / 3.0
    while v[y0, x0:x1].mean() > 200: y0 += 1
    while v[y1 - 1, x0:x1].mean() > 200: y1 -= 1
    while v[y0:y1, x0].mean() > 200: x0 += 1
    while v[y0:y1, x1 - 1].mean() > 200: x1 -= 1
    y0, y1, x0, x1 = y0 + 1, y1 - 1, x0 + 1, x1 - 1
    return y0, y1, x0, x1


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
        meta[name] = dict(notebook=f"examples/angulararea-emitter/render_{nb}_1light.ipynb", cell=cell,
                          spp=256 if cell == 4 else 64, res=RES, figure_box=[int(v) for v in box],
                          display="(data_steady / max) ** (1/4), RGB, 8 bit")
    np.savez_compressed(os.path.join(HERE, "angular_figures.npz"), meta=json.dumps(meta), **arrays)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
