"""Brute-force ray queries in float64 over a scene DESCRIPTION (SceneData: triangles, the analytic rectangles' and spheres' shape
records) — the plain reference tests/test_walk_cases.py holds the oracle's f32 brute force to.  Nothing of mtr_core.h or the oracle
is restated: Moller-Trumbore, a rectangle as centre and two half edges, a sphere as the roots of a quadratic.

closest(sd, o, d, tmax) -> dict of arrays over the rays:
  prim    original index of the nearest primitive hit within [0, tmax] (a rectangle or sphere reports its first triangle), -1: none
  t, u, v distance and the primitive's coordinates of that hit (triangle: barycentrics of p1, p2; rectangle: local x, y in [-1, 1])
  margin  how far inside its primitive the hit lies: min(u, v, 1 - u - v) of a triangle, min(1 - |x|, 1 - |y|) of a rectangle, inf on a sphere
  cos     |cosine| between the ray and the primitive's normal at the hit
  near    the smallest distance, in the same units as `margin`, by which the ray misses (or lies inside) ANY primitive's border among
          those whose plane it crosses within [0, tmax * (1 + 1e-6)]: a ray with near > band neither gains nor loses a hit by rounding
  gap     (t' - t) / t of the second-nearest hit t' (inf: none): two surfaces that coincide are told apart by rounding alone
  tedge   the smallest |t - tmax| / tmax among those crossings (inf where tmax is): a crossing that rounding can move past tmax
"""
import numpy as np

from mitransient_amd import _cabi


def primitives(sd):
    """[(kind, first original index, data)]: kind "tri" (data (3, 3)), "rect" ((c, du, dv)) or "sphere" ((c, r))"""
    tv = np.asarray(sd.tri_verts, np.float64).reshape(-1, 3, 3)
    out, covered = [], np.zeros(len(tv), bool)
    for s in range(sd.n_shapes):
        sh = sd.shapes[s]
        a, n = int(sh.first_tri), int(sh.n_tris)
        if (sh.kind & 0xff) == _cabi.MTR_SHAPE_SPHERE:
            out.append(("sphere", a, (np.array(list(sh.center), np.float64), float(sh.radius))))
            covered[a:a + n] = True
        elif sh.is_rectangle & 1:
            out.append(("rect", a, (np.array(list(sh.center), np.float64), np.array(list(sh.du), np.float64), np.array(list(sh.dv), np.float64))))
            covered[a:a + n] = True
    for i in np.flatnonzero(~covered):
        out.append(("tri", int(i), tv[i]))
    return out


def _one(kind, data, o, d):
    """(t, u, v, margin, |cos|, valid) of every ray against one primitive; valid: the ray meets its plane / surface at all"""
    n = len(o)
    if kind == "tri":
        p0, e1, e2 = data[0], data[1] - data[0], data[2] - data[0]
        pv = np.cross(d, e2)
        det = pv @ e1
        ok = det != 0.0
        inv = 1.0 / np.where(ok, det, 1.0)
        tv = o - p0
        u = (tv * pv).sum(1) * inv
        qv = np.cross(tv, e1)
        v = (d * qv).sum(1) * inv
        t = qv @ e2 * inv
        nrm = np.cross(e1, e2)
        nl = np.linalg.norm(nrm)
        cos = np.abs(d @ nrm) / (nl if nl > 0 else 1.0)
        return t, u, v, np.minimum(np.minimum(u, v), 1.0 - u - v), cos, ok & (nl > 0)
    if kind == "rect":
        c, du, dv = data
        nrm = np.cross(du, dv)
        nl = np.linalg.norm(nrm)
        den = d @ nrm
        ok = den != 0.0
        t = ((c - o) @ nrm) / np.where(ok, den, 1.0)
        p = o + d * t[:, None] - c
        # local coordinates: p = x du + y dv (du, dv need not be orthogonal)
        g = np.array([[du @ du, du @ dv], [du @ dv, dv @ dv]])
        xy = np.linalg.solve(g, np.stack([p @ du, p @ dv]))
        x, y = xy[0], xy[1]
        return t, x, y, np.minimum(1.0 - np.abs(x), 1.0 - np.abs(y)), np.abs(den) / nl, ok
    c, r = data
    l = c - o
    tc = (l * d).sum(1) / (d * d).sum(1)
    perp = l - d * tc[:, None]
    disc = r * r - (perp * perp).sum(1)
    ok = disc >= 0.0
    root = np.sqrt(np.where(ok, disc, 0.0)) / np.sqrt((d * d).sum(1))
    near, far = tc - root, tc + root
    t = np.where(near >= 0.0, near, far)
    nvec = (o + d * t[:, None] - c) / r
    cos = np.abs((nvec * d).sum(1)) / np.linalg.norm(d, axis=1)
    # margin in units of the radius: how far the ray's closest approach is from grazing
    graze = np.abs(np.sqrt((perp * perp).sum(1)) - r) / r
    return t, np.zeros(n), np.zeros(n), np.where(ok, graze, -graze), cos, np.ones(n, bool)


def closest(sd, o, d, tmax):
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    tmax = np.asarray(tmax, np.float64)
    n = len(o)
    best = {"prim": np.full(n, -1, np.int64), "t": np.full(n, np.inf), "u": np.zeros(n), "v": np.zeros(n),
            "margin": np.full(n, np.inf), "cos": np.ones(n), "near": np.full(n, np.inf), "tedge": np.full(n, np.inf), "gap": np.full(n, np.inf)}
    second = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for kind, first, data in primitives(sd):
            t, u, v, margin, cos, ok = _one(kind, data, o, d)
            if kind == "sphere":
                c, r = data
                inside_all = (np.linalg.norm(o - c, axis=1) < r) & (t > tmax)
                hit = ok & (margin >= 0.0) & (t >= 0.0) & (t <= tmax) & ~inside_all
                reach = np.ones(n, bool)
            else:
                hit = ok & (margin >= 0.0) & (t >= 0.0) & (t <= tmax)
                reach = ok & (t >= -1e-6 * np.abs(t)) & (t <= tmax * (1.0 + 1e-6))
            best["near"] = np.where(reach, np.minimum(best["near"], np.abs(margin)), best["near"])
            te = np.where(np.isfinite(tmax), np.abs(t - tmax) / np.where(np.isfinite(tmax) & (tmax > 0), tmax, 1.0), np.inf)
            best["tedge"] = np.where(ok & (t >= 0.0) & (margin > -1e-4) & np.isfinite(te), np.minimum(best["tedge"], te), best["tedge"])
            second = np.where(hit, np.where(t < best["t"], best["t"], np.minimum(second, t)), second)
            take = hit & ((t < best["t"]) | ((t == best["t"]) & ((best["prim"] < 0) | (first < best["prim"]))))
            for k, val in (("t", t), ("u", u), ("v", v), ("margin", margin), ("cos", cos)):
                best[k] = np.where(take, val, best[k])
            best["prim"] = np.where(take, first, best["prim"])
        best["gap"] = np.where(np.isfinite(second), (second - best["t"]) / np.maximum(best["t"], 1e-300), np.inf)
    return best
