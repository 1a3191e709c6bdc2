"""The ray families of tests/walk_cases.py on the CPU: that each reaches the edge it names (counted from the inputs, so that the device
test, tests/test_gpu_walk.py, cannot pass for want of a case), that the host build's walk — every tree form — equals the oracle's brute
force on them in t bits, primitive and occlusion, and that the oracle's brute force agrees with a plain f64 reference
(tests/walk_reference.py) wherever rounding cannot decide a hit."""
import numpy as np
import pytest

import walk_cases as W
import walk_reference as R

CLOSEST = [(s, f) for s in W.SCENES for f in W.SCENES[s][1] if f != "shadow"]
RANDOM = [s for s in W.SCENES if "random" in W.SCENES[s][1] and (s, "random") not in W.NO_FRACTION and s not in W.COINCIDENT]


@pytest.fixture(scope="module")
def hh(host_harness):
    return host_harness


def _brute(oracle, name, o, d, tm):
    """(t, original index, occlusion) of the oracle's brute force — or, on the scene the oracle cannot describe (W.NO_ORACLE), of the host
    build's BVH2 walk, which test_oracle_brute_force_against_f64_on_random_rays then holds to f64 in the oracle's place"""
    if name in W.NO_ORACLE:
        hit4, orig, occ = W.host_walk(W.host_harness(), W.scene(name), o, d, tm, "bvh2-selects")
        return hit4[:, 0].copy().view(np.float32), orig, occ
    return oracle.intersect(W.scene(name), o, d, tm, use_bvh=False)


@pytest.mark.parametrize("name,family", CLOSEST, ids=[f"{s}-{f}" for s, f in CLOSEST])
def test_family_reaches_its_edges_and_hits_a_fair_share(oracle, name, family):
    r = W.rays(name, family)
    print(f"[walk] {name}/{family}: {r.n} rays, {r.edges}")
    assert r.n > 0 and r.edges and all(v > 0 for v in r.edges.values()), r.edges
    t, prim, occ = _brute(oracle, name, *W.variant_rays(r, "", np.arange(r.n)))
    frac = float((prim >= 0).mean())
    print(f"[walk] {name}/{family}: {frac:.3f} of the rays hit")
    if (name, family) not in W.NO_FRACTION:
        assert 0.20 <= frac <= 0.98, frac


@pytest.mark.parametrize("tree", list(W.HOST_TREES))
@pytest.mark.parametrize("name,family", CLOSEST, ids=[f"{s}-{f}" for s, f in CLOSEST])
def test_host_walk_equals_the_oracles_brute_force(oracle, hh, name, family, tree):
    """the existing property of tests/test_scene_host.py on these rays: t bits, original index, occlusion"""
    r = W.rays(name, family)
    for var, idx in W.variants(r):
        o, d, tm = W.variant_rays(r, var, idx)
        t0, p0, occ0 = _brute(oracle, name, o, d, tm)
        hit4, orig, occ = W.host_walk(hh, W.scene(name), o, d, tm, tree)
        bad = np.flatnonzero((t0.view(np.uint32) != hit4[:, 0]) | (p0 != orig) | (occ0 != occ))
        assert bad.size == 0, (f"{bad.size} of {len(o)} rays differ; " +
                               "; ".join(f"{W.describe(name, family, idx[i])}: oracle t {t0[i]!r} prim {p0[i]} occ {occ0[i]}, host t "
                                         f"{hit4[i, :1].view(np.float32)[0]!r} prim {orig[i]} occ {occ[i]}" for i in bad[:3]))


def test_shadow_rays_host_walk_equals_the_oracle_and_all_three_tiers_occur(oracle, hh):
    """the shadow family: the rays hh_walk_shadow builds give the oracle's occlusion answer, and — with hull_side re-stated in numpy on
    the host classifier's ShadowHull — there are waves whose lanes are all safe, waves with exactly one risky_e lane and no risky_h
    lane, and waves with exactly one risky_h lane"""
    r = W.rays("cornell", "shadow")
    sd = W.scene("cornell")
    hull, traits, _ = W.hull_of(hh, sd)
    assert hull["count"] == 5 and r.n % 256 == 0
    ray7, hit4, orig, occ = W.host_walk_shadow(hh, sd, r.o, r.d, r.tmax)
    t0, p0, occ0 = oracle.intersect(sd, ray7[:, :3], ray7[:, 3:6], ray7[:, 6], use_bvh=False)
    assert np.array_equal(t0.view(np.uint32), hit4[:, 0]) and np.array_equal(p0, orig) and np.array_equal(occ0, occ)
    rh, re = W.hull_tiers(hull, ray7[:, :3])
    rh, re = rh.reshape(-1, 64), re.reshape(-1, 64)
    tiers = {"all-safe": int(np.sum(~rh.any(1) & ~re.any(1))), "one-risky-e": int(np.sum(~rh.any(1) & (re.sum(1) == 1))),
             "one-risky-h": int(np.sum(rh.sum(1) == 1)), "many-risky-h": int(np.sum(rh.sum(1) > 1))}
    print(f"[walk] shadow: {r.n} rays, waves by tier {tiers}, {float(occ.mean()):.3f} occluded, {r.edges}")
    assert all(v > 0 for v in tiers.values()), tiers
    assert 0.05 < occ.mean() < 0.95
    # the refusals the device test relies on are the host classifier's verdicts too
    assert W.hull_of(hh, W.scene("cornell-panel"))[0]["count"] == 0


def test_second_nearest_rays_miss_their_first_candidate(oracle):
    """counted from the inputs: rays whose nearest-entry rectangle box belongs to a rectangle the f64 reference says they miss, and
    rays whose hit lies within 8 ulps of the second entry distance"""
    name = "cornell-panel"
    r = W.rays(name, "second_nearest")
    sd = W.scene(name)
    ent = W.rect_entry_order(sd, r.o, r.d)
    order = np.argsort(ent, axis=1)
    first = order[:, 0]
    ref = R.closest(sd, r.o, r.d, r.tmax)
    rect_first_tri = [f for k, f, _ in R.primitives(sd) if k == "rect"]
    first_is_hit = np.array([rect_first_tri[k] for k in first]) == ref["prim"]
    missed_first = np.isfinite(ent[np.arange(r.n), first]) & ~first_is_hit & (ref["prim"] >= 0)
    second = np.sort(ent, axis=1)[:, 1]
    t32 = ref["t"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        close = np.isfinite(second) & np.isfinite(ref["t"]) & (np.abs(second - ref["t"]) <= 8.0 * np.spacing(t32))
    print(f"[walk] second_nearest: {int(missed_first.sum())} rays miss their first candidate, {int(close.sum())} hit within 8 ulps of the second entry")
    assert missed_first.sum() > 1000 and close.sum() > 100


@pytest.mark.parametrize("name", RANDOM)
def test_oracle_brute_force_against_f64_on_random_rays(oracle, name):
    """every `random` ray whose f64 hit lies farther than 2 kEdgeEps from every border (of every primitive it crosses) and is not
    grazing hits the same primitive in the oracle's brute force, t within TOL and (u, v) within TOL_UV; every ray that f64 says misses
    everything by more than the band misses; at most 2 % of the rays are neither"""
    r = W.rays(name, "random")
    sd = W.scene(name)
    ref = R.closest(sd, r.o, r.d, r.tmax)
    t, prim, _ = _brute(oracle, name, r.o, r.d, r.tmax)
    clear = (ref["near"] > W.BAND) & (ref["tedge"] > 1e-5) & (ref["gap"] > 1e-5)
    hit = clear & (ref["prim"] >= 0) & (ref["cos"] >= W.MIN_COS)
    miss = clear & (ref["prim"] < 0)
    excluded = 1.0 - float((hit | miss).mean())
    assert np.array_equal(prim[hit], ref["prim"][hit]), np.flatnonzero(hit & (prim != ref["prim"]))[:5]
    assert np.all(prim[miss] < 0), np.flatnonzero(miss & (prim >= 0))[:5]
    err_t = float(np.max(np.abs(t[hit] - ref["t"][hit]) / ref["t"][hit])) if hit.any() else 0.0
    hit4, _, _ = W.host_walk(W.host_harness(), sd, r.o, r.d, r.tmax, "bvh2-selects")
    uv = hit4[:, 1:3].view(np.float32).astype(np.float64)
    spheres = np.array([k == "sphere" for k, _, _ in R.primitives(sd)])
    sphere_first = {f for k, f, _ in R.primitives(sd) if k == "sphere"}
    flat = hit & ~np.isin(ref["prim"], list(sphere_first))            # (a sphere's (u, v) is a direction code, not a position on a plane)
    err_uv = float(np.max(np.abs(uv[flat] - np.stack([ref["u"], ref["v"]], 1)[flat]))) if flat.any() else 0.0
    print(f"[walk] {name}/random against f64: {int(hit.sum())} interior hits, {int(miss.sum())} clear misses, {excluded:.4f} excluded, "
          f"max rel err t {err_t:.3e}, max abs err uv {err_uv:.3e} ({int(spheres.sum())} spheres)")
    assert excluded <= W.MAX_EXCLUDED, excluded
    _, tol, _, tol_uv = W.TOLS[name]
    assert err_t <= tol and err_uv <= tol_uv, (err_t, err_uv)


@pytest.mark.xfail(strict=True, reason="culling is conservative only while the padding of a box (2e-5 relative) exceeds the rounding of a slab distance: "
                   "from 12 559 and 14 241 units away (one ulp of t: 1e-3) the oracle's brute force hits the rim of cornell-twin-wall's ceiling "
                   "(t 12559.141, triangle 4) and back wall (t 14241.706, triangle 8) and every tree of the host build — and the MI355X with "
                   "it — reports a miss.  No ray of a render starts there (HISTORY.md); left alone")
def test_walk_equals_brute_force_from_ten_thousand_room_sizes_away(oracle, hh):
    sd = W.scene("cornell-twin-wall")
    words = lambda w: np.array([int(x, 16) for x in w.split()], np.uint32).view(np.float32)          # noqa: E731
    o = np.array([words(a) for a, _ in W.FAR_RAYS]); d = np.array([words(b) for _, b in W.FAR_RAYS])
    tm = np.full(len(o), np.inf, np.float32)
    t0, p0, _ = oracle.intersect(sd, o, d, tm, use_bvh=False)
    hit4, orig, _ = W.host_walk(hh, sd, o, d, tm, "wide")
    assert np.array_equal(p0, orig) and np.array_equal(t0.view(np.uint32), hit4[:, 0]), (p0, orig)


EDGE = [(s, f) for s, f in CLOSEST if f in ("diagonals",)]


@pytest.mark.parametrize("name,family", EDGE, ids=[f"{s}-{f}" for s, f in EDGE])
def test_edge_aimed_rays_do_not_leak(oracle, name, family):
    """the no-leak rule: a ray aimed at a shared edge interior to a closed surface hits something no farther than the primitives f64
    places at the target — it never slips between the two triangles"""
    r = W.rays(name, family)
    sd = W.scene(name)
    t, prim, _ = _brute(oracle, name, r.o, r.d, r.tmax)
    dist = np.linalg.norm(r.target - r.o.astype(np.float64), axis=1)
    leak = np.isinf(r.tmax) & ((prim < 0) | (t > dist * (1.0 + 1e-4)))
    print(f"[walk] {name}/{family}: {int(leak.sum())} of {int(np.isinf(r.tmax).sum())} unbounded rays pass their target")
    assert not leak.any(), "; ".join(W.describe(name, family, i) for i in np.flatnonzero(leak)[:3])


def test_expected_table_lists_every_form_and_the_refusals_are_refusals(hh):
    """the run list the device test asserts: every scene's forms x both flag sets x its families, and the (scene, form) pairs the hook
    must refuse are ones the host classifier rules out"""
    for name in W.SCENES:
        runs = W.expected_runs(name)
        assert {r[1] for r in runs} == set(W.SCENES[name][0]) and {r[2] for r in runs} == set(W.SUFFIXES)
        hull, traits, sizes = W.hull_of(hh, W.scene(name))
        flat = 0 if not traits & 8 else (2 if traits & 16 else 1)
        for form in W.SCENES[name][0]:
            if form.startswith("flat"):
                assert flat == (2 if form == "flat_leaves" else 1), (name, form, traits)
            if form == "q8_hbm":
                assert sizes[3] > 0 or name == "empty", (name, sizes)
            if form.startswith("wide_lds") or form.startswith("flat"):
                assert sizes[4] == 1, (name, sizes)
    info = {n: W.hull_of(hh, W.scene(n)) for n in {s for s, _, _ in W.REFUSALS}}
    assert info["sticks"][2][1] == 0 and not info["sticks"][1] & 8          # no 8-wide tree to stage: never in LDS, no flat top level
    assert not info["mesh-boxes"][1] & 8 and info["cornell"][1] & 8 and not info["cornell"][1] & 16 and info["top-level-triangles"][1] & 16
    assert info["cornell-panel"][0]["count"] == 0 and not info["spheres"][1] & (2 | 4 | 8 | 16 | 64)
