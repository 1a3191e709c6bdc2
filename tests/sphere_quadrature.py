"""Expected films of scenes with mitsuba's analytic `sphere`, by f64 NumPy quadrature written apart from the product.

Everything here works on world-space spheres (centre c, radius r) and the product's own perspective matrices
(delta_quadrature.camera_rays: S x S midpoint sub-pixel rays per pixel, origins on the near plane).

    roots            the two solutions of |o + t d - c|^2 = r^2 (nan where the ray misses)
    first_hit        mitsuba's choice among them: the near root, the far one from inside
    seen_ball        coverage and mean hit distance per pixel of a ball in front of (or around) the camera
    sphere_light     the direct term of a sphere light on a diffuse plane: steady value and time profile per pixel, by a
                     midpoint rule over the cone the sphere subtends (uniform in (cos theta, phi): each cell is the same solid angle)
    lens_opl         optical path of the two-refraction chain through a glass ball onto a rectangle
    hidden_ball      the three-bounce term of a NLOS capture of a ball: wall -> ball -> laser spot -> laser

`variant` of sphere_light names a misreading of sphere.cpp whose expected film the same rule gives:

    "area_pdf"       cone samples weighted with the area density dist^2 / (A cos) instead of the cone's
    "no_omc"         the cone density without its (1 - cos theta_max): 1 / (2 pi)
    "em_pdf_area"    the MIS weight of a BSDF-sampled hit computed with dist^2 / (A cos) while emitter sampling uses the cone density
    "inward_normal"  ds.n = -d on an unflipped sphere: dot(ds.d, ds.n) < 0 never holds, the emitter-sampling term vanishes and the
                     BSDF-sampled hit keeps its MIS weight"""
import math

import numpy as np

import delta_quadrature as DQ

VARIANTS = ("area_pdf", "no_omc", "em_pdf_area", "inward_normal")


def roots(org, d, c, r):
    """(near, far) ray parameters, nan where the ray misses; d is unit"""
    l = np.asarray(c, np.float64) - org
    tc = (l * d).sum(-1)
    q = l - d * tc[..., None]
    disc = r * r - (q * q).sum(-1)
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
    return tc - sq, tc + sq


def first_hit(org, d, c, r):
    near, far = roots(org, d, c, r)
    with np.errstate(invalid="ignore"):
        t = np.where(near >= 0, near, far)
        return np.where(np.isfinite(t) & (far >= 0), t, np.inf)


def seen_ball(scene, c, r, S=32):
    """(coverage (h, w), mean hit distance over the covered part of the footprint (h, w), measured from the near plane: the camera
    ray's own parameter)"""
    _, _, d, org = DQ.camera_rays(scene, S)
    t = first_hit(org, d, c, r)
    hit = np.isfinite(t)
    cov = hit.mean(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_t = np.where(hit, t, 0.0).sum(-1) / hit.sum(-1)
    return cov, mean_t


def _cone_dirs(x, c, r, M):
    """M x M directions uniform over the cone a sphere subtends from the points x (n, 3): (n, M*M, 3), the solid angle (n,), cos theta_max"""
    dc = np.asarray(c, np.float64) - x
    D = np.linalg.norm(dc, axis=-1)
    w = dc / D[:, None]
    sin2 = (r / D) ** 2
    cmax = np.sqrt(1.0 - sin2)
    omc = sin2 / (1.0 + cmax)
    g = (np.arange(M) + 0.5) / M
    u1, u2 = [a.reshape(-1) for a in np.meshgrid(g, g)]
    ct = 1.0 - omc[:, None] * u1[None]
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    ph = 2.0 * math.pi * u2
    a = np.where(np.abs(w[:, :1]) < 0.9, np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))
    s = np.cross(w, a); s /= np.linalg.norm(s, axis=-1, keepdims=True)
    t = np.cross(w, s)
    dirs = (st * np.cos(ph))[..., None] * s[:, None] + (st * np.sin(ph))[..., None] * t[:, None] + ct[..., None] * w[:, None]
    return dirs, 2.0 * math.pi * omc, cmax


def sphere_light(scene, plane, c, r, L, S=4, M=64, variant=None, bins=None):
    """direct light of a sphere light (radiance L (3,), wholly above the plane's horizon) on a diffuse Plane, max_depth 2 with
    MIS: (steady (h, w, 3), profile (h, w, T) of channel sums or None, (lo, hi) of t_cam + the distance to the visible cap)"""
    W, H, d, org = DQ.camera_rays(scene, S)
    t = plane.hit(org, d)
    assert np.isfinite(t).all()
    x = (org + d * t[..., None]).reshape(-1, 3)
    tc = t.reshape(-1)
    dirs, omega, cmax = _cone_dirs(x, c, r, M)
    cosx = np.maximum(dirs @ plane.n, 0.0)
    near, _ = roots(x[:, None], dirs, c, r)
    assert np.isfinite(near).all()
    y = x[:, None] + dirs * near[..., None]
    nl = (y - np.asarray(c, np.float64)) / r
    cosl = np.maximum(-(dirs * nl).sum(-1), 0.0)
    f = (1.0 / math.pi) * cosx                      # BSDF value * cos per unit albedo and radiance
    pe = 1.0 / omega[:, None]                       # the cone density
    pb = cosx / math.pi
    area_pdf = near * near / (4.0 * math.pi * r * r * np.maximum(cosl, 1e-300))
    if variant is None:
        val = f                                     # the two MIS weights sum to one
    elif variant == "area_pdf":
        pw = area_pdf
        val = f * pe / pw * (pw * pw / (pw * pw + pb * pb)) + f * (pb * pb / (pb * pb + pw * pw))
    elif variant == "no_omc":
        pw = np.full_like(pe, 1.0 / (2.0 * math.pi))
        val = f * pe / pw * (pw * pw / (pw * pw + pb * pb)) + f * (pb * pb / (pb * pb + pw * pw))
    elif variant == "em_pdf_area":
        val = f * (pe * pe / (pe * pe + pb * pb)) + f * (pb * pb / (pb * pb + area_pdf * area_pdf))
    elif variant == "inward_normal":
        val = f * (pb * pb / (pb * pb + pe * pe))
    else:
        raise ValueError(variant)
    cell = val * (omega / (M * M))[:, None]                         # (n, M*M)
    steady = cell.sum(-1)[:, None] * (plane.albedo * np.asarray(L, np.float64))
    steady = steady.reshape(H, W, S * S, 3).mean(2)
    span = (float((tc[:, None] + near).min()), float((tc[:, None] + near).max()))
    prof = None
    if bins is not None:
        start, width, T = bins
        k = np.floor((tc[:, None] + near - start) / width).astype(np.int64)
        ok = (k >= 0) & (k < T)
        pix = np.repeat(np.arange(H * W), S * S)[:, None] + np.zeros_like(k)
        prof = np.zeros((H * W, T))
        np.add.at(prof, (pix[ok], k[ok]), (cell * float((plane.albedo * np.asarray(L, np.float64)).sum()))[ok] / (S * S))
        prof = prof.reshape(H, W, T)
    return steady, prof, span


def _refract(d, n, eta):
    """Snell: d unit towards the surface, n unit against d, eta = n_t / n_i; (direction, Fresnel transmittance)"""
    ci = -(d * n).sum(-1)
    s2 = (1.0 - ci * ci) / (eta * eta)
    ct = np.sqrt(1.0 - s2)
    t = d / eta + n * (ci / eta - ct)[..., None]
    rs = (ci - eta * ct) / (ci + eta * ct)
    rp = (ct - eta * ci) / (ct + eta * ci)
    return t, 1.0 - 0.5 * (rs * rs + rp * rp)


def lens_opl(scene, c, r, eta, plane, S=16):
    """mean optical path length (from the near plane), weighted by the two Fresnel transmittances, of the chain camera -> ball ->
    inside -> ball -> rectangle over the pixel footprints: (h, w); and the share of footprint rays that complete it"""
    _, _, d, org = DQ.camera_rays(scene, S)
    t1, _ = roots(org, d, c, r)
    ok = np.isfinite(t1)
    p1 = org + d * np.where(ok, t1, 0.0)[..., None]
    n1 = (p1 - c) / r
    d2, T1 = _refract(d, n1, eta)
    _, t2 = roots(p1, d2, c, r)
    p2 = p1 + d2 * t2[..., None]
    n2 = -(p2 - c) / r
    d3, T2 = _refract(d2, n2, 1.0 / eta)
    t3 = plane.hit(p2, d3)
    ok &= np.isfinite(t3)
    wgt = np.where(ok, T1 * T2, 0.0)
    opl = np.where(ok, t1 + eta * t2 + t3, 0.0)
    return (wgt * opl).sum(-1) / wgt.sum(-1), ok.mean(-1)


def sphere_grid(c, r, M):
    """points and unit normals of an equal-area midpoint grid on the sphere (M in z, 2 M in phi) and the cell area"""
    z = 1.0 - 2.0 * (np.arange(M) + 0.5) / M
    ph = 2.0 * math.pi * (np.arange(2 * M) + 0.5) / (2 * M)
    Z, P = [a.reshape(-1) for a in np.meshgrid(z, ph)]
    rho = np.sqrt(1.0 - Z * Z)
    n = np.stack([rho * np.cos(P), rho * np.sin(P), Z], -1)
    return np.asarray(c, np.float64) + r * n, n, 4.0 * math.pi * r * r / (2 * M * M)


def hidden_ball(x_s, n_w, x_l, o_s, o_l, c, r, irradiance, scale, albedo_wall=1.0, albedo_ball=1.0, M=512, bins=None):
    """the three-bounce term of one pixel of a Single capture: sensor origin o_s -> wall point x_s -> ball -> laser spot x_l -> laser
    o_l, both walls points on the relay wall with unit normal n_w; the laser spot is on the projector's axis.  Returns (steady,
    profile (T,) or None, shortest x_l - y - x_s path)"""
    Y, nY, dA = sphere_grid(c, r, M)
    a = Y - x_s; da = np.linalg.norm(a, axis=-1); a /= da[:, None]
    b = x_l - Y; db = np.linalg.norm(b, axis=-1); b /= db[:, None]
    cos_i = np.maximum(a @ n_w, 0.0)                       # at the wall point
    cos_g = np.maximum(-(a * nY).sum(-1), 0.0)             # at the ball, towards the wall point
    cos_o = np.maximum((b * nY).sum(-1), 0.0)              # at the ball, towards the laser spot
    cos_l = np.maximum(-(b @ n_w), 0.0)                    # at the laser spot
    to_l = o_l - x_l; dl = np.linalg.norm(to_l); cos_e = float((to_l / dl) @ n_w)
    G = cos_i * cos_g / (da * da) * cos_o * cos_l / (db * db) * dA
    k = (albedo_wall / math.pi) ** 2 * (albedo_ball / math.pi) * cos_e * (irradiance * math.pi * scale / (dl * dl))
    val = k * G
    opl = np.linalg.norm(x_s - o_s) + da + db + dl
    lit = val > 0
    prof = None
    if bins is not None:
        start, width, T = bins
        idx = np.floor((opl - start) / width).astype(np.int64)
        ok = (idx >= 0) & (idx < T)
        prof = np.zeros(T)
        np.add.at(prof, idx[ok], val[ok])
    return float(val.sum()), prof, float((da + db)[lit].min())
