"""Expected films of scenes lit by mitsuba's `point` / `spot` emitters, by f64 midpoint quadrature.

A delta emitter is sampled with ds.pdf = 1 and never hit, so the direct term at a surface point x seen by a camera ray is closed
form, no integral over the light:

    rho / pi * cos_x * I * falloff(angle to the spot's axis) / d^2        at the optical path length  t_cam + d

with d = |p - x| (transientpath.py:188-218 with `mis_em = 1`, :210).  The camera integral over a pixel is a midpoint grid of
S x S sub-pixel rays of the product's own perspective matrices (crop windows included); the camera ray starts on the near plane.
The falloff is evaluated in f64 on the f32 constants of the emitter record, as angular_quadrature.falloff.

`variant` names a misreading whose expected film the same rule gives, so that a test can show its tolerance tells them apart:

    "inv_d"       the weight intensity / d instead of / d^2
    "no_cos"      the BSDF value without its cosine
    "plus_d"      the spot's falloff of +ds.d instead of -ds.d
    "mis"         mis_weight(ds.pdf / n, bsdf_pdf) (power heuristic) instead of 1
    "pdf_no_n"    the emitter pick's 1 / n left out of the pdf: the term not multiplied by n_emitters after a uniform pick, i.e. 1 / n
                  of its value

The scenes are planar and convex (a floor; a floor and a wall at right angles): nothing occludes anything."""
import math

import numpy as np

VARIANTS = ("inv_d", "no_cos", "plus_d", "mis", "pdf_no_n")
POINT, SPOT = 1, 2          # mtr_emitter.kind


def falloff(c, e):
    """spot.cpp falloff_curve in f64 on the f32 constants of the emitter record"""
    th = np.arccos(np.clip(c, -1.0, 1.0))
    with np.errstate(invalid="ignore"):                  # (cutoff == beam: 0 * inf in the branch that is never selected)
        b = np.where(c >= e.cos_beam, 1.0, (e.cutoff - th) * e.inv_transition)
    return np.where(c > e.cos_cutoff, b, 0.0)


def camera_rays(scene, S):
    """(crop_h, crop_w, S * S, 3) directions and near-plane origins of the S x S midpoint sub-pixel rays of the crop window"""
    from mitransient_amd.scene import perspective_matrices
    sen = scene.sensors()[0]
    film = sen.film()
    W, H = film.crop_size_
    s2c, tw, near, _ = perspective_matrices(sen.dict_, film.size_, film.crop_size_, film.crop_offset_)
    s2c = np.asarray(s2c, np.float64).reshape(4, 4)
    tw = np.asarray(tw, np.float64).reshape(4, 4)
    o = (np.arange(S) + 0.5) / S
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    sx = (px[..., None, None] + o[None, None, None, :]) / W
    sy = (py[..., None, None] + o[None, None, :, None]) / H
    sx, sy = np.broadcast_arrays(sx, sy)
    P = np.stack([sx, sy, np.zeros_like(sx), np.ones_like(sx)], -1) @ s2c.T
    dl = P[..., :3] / P[..., 3:]
    dl /= np.linalg.norm(dl, axis=-1, keepdims=True)
    d = dl @ tw[:3, :3].T
    org = tw[:3, 3] + d * (near / dl[..., 2:3])
    return W, H, d.reshape(H, W, S * S, 3), org.reshape(H, W, S * S, 3)


class Plane:
    """a rectangle  c + u du + v dv, |u|, |v| <= 1, with unit normal n and a diffuse albedo"""

    def __init__(self, c, du, dv, albedo):
        self.c, self.du, self.dv = (np.asarray(x, np.float64) for x in (c, du, dv))
        n = np.cross(self.du, self.dv)
        self.area = 4.0 * np.linalg.norm(n)
        self.n = n / np.linalg.norm(n)
        self.albedo = np.asarray(albedo, np.float64)

    def hit(self, org, d):
        """ray parameter (inf where the ray misses the rectangle or meets its back)"""
        den = d @ self.n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.c - org) @ self.n) / den
        x = org + d * t[..., None] - self.c
        u = (x @ self.du) / (self.du @ self.du)
        v = (x @ self.dv) / (self.dv @ self.dv)
        ok = (den < 0) & (t > 0) & (np.abs(u) <= 1) & (np.abs(v) <= 1)
        return np.where(ok, t, np.inf)

    def blocks(self, x, p):
        """whether the rectangle (either side) lies between the points x (..., 3) and the point p"""
        v = p - x
        den = v @ self.n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.c - x) @ self.n) / den
        y = x + v * t[..., None] - self.c
        u = (y @ self.du) / (self.du @ self.du)
        w = (y @ self.dv) / (self.dv @ self.dv)
        return (t > 1e-9) & (t < 1.0 - 1e-9) & (np.abs(u) <= 1) & (np.abs(w) <= 1)

    def grid(self, M):
        g = (np.arange(M) + 0.5) / M * 2.0 - 1.0
        U, V = [a.reshape(-1) for a in np.meshgrid(g, g)]
        return self.c + U[:, None] * self.du + V[:, None] * self.dv, self.area / (M * M)


def emitter_weight(e, x, variant=None):
    """(I * falloff * 1 / d^2 as (..., 3), unit direction x -> p, d) of the delta emitter record e at the points x"""
    p = np.array(list(e.center), np.float64)
    v = p - x
    d = np.linalg.norm(v, axis=-1)
    w = v / d[..., None]
    g = 1.0 / d if variant == "inv_d" else 1.0 / (d * d)
    if e.kind == SPOT:
        axis = np.array(list(e.axis), np.float64)
        g = g * falloff((w if variant == "plus_d" else -w) @ axis, e)
    return g[..., None] * np.array(list(e.radiance), np.float64), w, d


def direct(e, x, n, albedo, variant=None, n_emitters=1, occluders=()):
    """the emitter-sampling term of emitter e at the surface points x (normal n, diffuse albedo): ((..., 3), d)"""
    g, w, d = emitter_weight(e, x, variant)
    for oc in occluders:
        g = g * ~oc.blocks(x, np.array(list(e.center), np.float64))[..., None]
    cos = np.maximum(w @ n, 0.0)
    lit = cos > 0
    bpdf = cos / math.pi
    f = (1.0 / math.pi) * (lit if variant == "no_cos" else cos)
    if variant == "mis":
        pe = 1.0 / n_emitters
        f = f * pe * pe / (pe * pe + bpdf * bpdf)
    if variant == "pdf_no_n":
        f = f / n_emitters
    return f[..., None] * albedo * g, d


def film_of(scene, planes, S=4, variant=None, emitters=None, bounce=None, M=96, occluders=()):
    """Expected (steady (h, w, 3), mean OPL (h, w) of the direct term, its mean t_cam (h, w); both weighted by the term's
    channel sum, nan in an unlit pixel) of max_depth = 2 (bounce None), or the
    steady film of max_depth = 3 with `bounce`: one more vertex on the other plane (direct + one-bounce transport).
    emitters: indices into the scene's table (default: all of them, which must all be delta emitters).  occluders: Planes that
    shadow the emitters (the camera sees every plane of `planes`, nearest first)."""
    sd = scene.data()
    idx = list(range(sd.n_emitters)) if emitters is None else list(emitters)
    n_em = sd.n_emitters
    W, H, d, org = camera_rays(scene, S)
    t = np.stack([pl.hit(org, d) for pl in planes], 0)
    first = np.argmin(t, 0)
    tmin = np.min(t, 0)
    steady = np.zeros((H, W, 3))
    opl_w = np.zeros((H, W))
    lum = np.zeros((H, W))
    tcam = np.zeros((H, W))
    for k, pl in enumerate(planes):
        sel = (first == k) & np.isfinite(tmin)
        if not sel.any():
            continue
        ii, jj, kk = np.nonzero(sel)
        x = org[ii, jj, kk] + d[ii, jj, kk] * tmin[ii, jj, kk][:, None]
        for i in idx:
            e = sd.emitters[i]
            L, dist = direct(e, x, pl.n, pl.albedo, variant, n_em, occluders)
            np.add.at(steady, (ii, jj), L / (S * S))
            wgt = L.sum(-1)
            np.add.at(opl_w, (ii, jj), wgt * (tmin[ii, jj, kk] + dist))
            np.add.at(lum, (ii, jj), wgt)
            np.add.at(tcam, (ii, jj), wgt * tmin[ii, jj, kk])
        if bounce is not None:
            # one more vertex y on the other plane: rho_x / pi * cos_x * cos_y / r^2 * (direct term at y), integrated over the plane
            other = planes[1 - k]
            Y, dA = other.grid(M)
            Ly = np.zeros((Y.shape[0], 3))
            for i in idx:
                Ly += direct(sd.emitters[i], Y, other.n, other.albedo, variant, n_em)[0]
            for c0 in range(0, x.shape[0], 512):
                xx = x[c0:c0 + 512]
                v = Y[None] - xx[:, None]
                r2 = (v * v).sum(-1)
                r = np.sqrt(r2)
                cx = np.maximum((v @ pl.n) / r, 0.0)
                cy = np.maximum(-(v @ other.n) / r, 0.0)
                G = cx * cy / r2 * dA
                ind = (G @ Ly) * (pl.albedo / math.pi)
                np.add.at(steady, (ii[c0:c0 + 512], jj[c0:c0 + 512]), ind / (S * S))
    with np.errstate(divide="ignore", invalid="ignore"):
        return steady, opl_w / lum, tcam / lum
