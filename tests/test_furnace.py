"""The white-furnace identity on the CPU: the oracle (oracle/mtr_oracle.c) and the host builds of the product's arithmetic
(tests/host_harness.cpp, host_polarized.cpp, host_grad.cpp, host_grad_tex.cpp, host_fwd.cpp) against the closed forms of
tests/furnace_cases.py — L_D = Le sum rho^k, L_inf = Le / (1 - rho), their derivatives, and S1..S3 = 0 — and the camera
against an f64 pinhole written out from the definition of the field of view.  No expectation here comes from the oracle.

Every comparison is furnace_cases.verdict: |mean - expected| <= 4 se, the power condition 4 se <= 1 % of the expectation, and
the same data must FAIL against expected (1 +- 0.01) and against the neighbouring orders.  Seeds are fixed.  32 x 32 pixels at
128 spp; reverse mode 16 seeds of 32 x 32 x 32; the derivatives of L_inf take more samples (furnace_cases.GRAD_SIZE_INF: why).
No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import furnace_cases as FC
import test_fwd as F
import test_grad as T
import test_grad_texture as X
import test_polarized as P
from conftest import rel_l2
from scene_class_cases import host_class
from test_grad import hg  # noqa: F401  (host build of mtr_grad.h)
from test_fwd import hf  # noqa: F401  (... of mtr_fwd.h)
from test_grad_texture import hgt  # noqa: F401  (... of mtr_grad.h with the texel hook)
from test_polarized import hp  # noqa: F401  (... of mtr_polar.h)

TIERS = ["oracle", "host"]
NO_LOBES, DIFFUSE, FLAT_TOP, ONE_RECT = 32, 1, 8, 2      # MTR_TRAIT_* (include/mitransient_amd.h)


@pytest.fixture(scope="module")
def film(oracle, host_harness):
    """film(tier, scene): the developed (steady, transient) of the oracle or of the host harness, f64"""
    def render(tier, scene, seed=0):
        s, t = FC.oracle_film(scene, seed) if tier == "oracle" else FC.host_film(host_harness, scene, seed)
        return s.astype(np.float64), t.astype(np.float64)
    return render


def check_steady(film, tier, scene, D, label, time_sum=None, rho=FC.RHO, le=FC.LE):
    s, t = film(tier, scene)
    e, others = FC.radiance(D, rho, le), FC.neighbours(D, rho, le)
    vs = [FC.verdict(FC.pixels(s), e, others)]
    FC.assert_verdict(vs[0], f"{tier} {label}")
    if time_sum if time_sum is not None else D > 0:
        vs.append(FC.verdict(FC.pixels(t.sum(2)), e, others))
        FC.assert_verdict(vs[1], f"{tier} {label} (time sum)")
    return s, vs


# -- 1. orders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
def test_orders(film, tier):
    """max_depth 1 (exact in every pixel), 2, 3, 4, 6 without roulette, each order's own term from the pixelwise difference
    of two renders at one seed, then roulette: max_depth 6 at rr_depth 2 and L_inf at rr_depth 3"""
    spp = FC.CPU_SIZE[1]
    prev, vs = None, []
    for D in (1, 2, 3, 4, 6):
        scene = FC.room(D, D + 1)
        if D == 1:
            s, t = film(tier, scene)
            e = FC.radiance(1)
            # every sample is Le, scaled by 1 / spp and added spp times in f32: at most spp roundings of 2^-24 each
            assert np.max(np.abs(s - e) / e) <= spp * 2.0 ** -24
            assert np.max(np.abs(t.sum(2) - e) / e) <= spp * 2.0 ** -24
            assert not FC.holds(FC.pixels(s), 1.01 * e) and not FC.holds(FC.pixels(s), FC.radiance(2))
        else:
            s, v = check_steady(film, tier, scene, D, f"D={D}")
            vs += v
        if prev is not None and D == prev[0] + 1:
            term = np.asarray(FC.LE) * np.asarray(FC.RHO) ** (D - 1)
            v = FC.verdict(FC.pixels(s - prev[1]), term, [term * np.asarray(FC.RHO), term / np.asarray(FC.RHO)])
            FC.assert_verdict(v, f"{tier} D={D} - D={D - 1}")
            vs.append(v)
        prev = (D, s)
    vs += check_steady(film, tier, FC.room(6, 2), 6, "D=6 rr_depth=2")[1]
    vs += check_steady(film, tier, FC.room(-1, 3), -1, "L_inf rr_depth=3")[1]
    print(f"[furnace] orders, {tier}: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs))


def test_the_rooms_classification(host_harness):
    """the rectangle room is the flat-top, several-emitter, all-diffuse scene the GPU tests force through k_fused"""
    traits, ext, polar, _ = host_class(host_harness, FC.room(2, 3))
    assert traits & FLAT_TOP and traits & DIFFUSE and not traits & ONE_RECT and not ext and polar


# -- 2. lossless inclusions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FC.INCLUSIONS))
@pytest.mark.parametrize("tier", TIERS)
def test_lossless_inclusions(film, host_harness, tier, name):
    scene = FC.room(-1, 3, **FC.INCLUSIONS[name]())
    sd = scene.data()
    types = sorted({int(sd.materials[m].type) for m in range(sd.n_materials)})
    assert types == {"glass": [0, 2], "thin": [0, 7], "glass_and_thin": [0, 2, 7]}.get(name, [0])
    if name == "twosided":
        assert sum(int(sd.materials[m].flags) & 1 for m in range(sd.n_materials)) == 1
    if name == "flip_normals":
        assert sum(int(sd.emitters[e].flip_normals) for e in range(sd.n_emitters)) == 2
    _, vs = check_steady(film, tier, scene, -1, f"L_inf {name}")
    print(f"[furnace] inclusions, {tier} {name}: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs))


# -- 3. mesh walls ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,n,mixed", [("small", FC.MESH_SMALL, False), ("large", FC.MESH_LARGE, False), ("mixed", FC.MESH_SMALL, True)])
@pytest.mark.parametrize("tier", TIERS)
def test_mesh_emitter_room(film, tier, tmp_path, which, n, mixed):
    """the room as one unevenly tessellated mesh emitter (triangle areas 49 : 1 and more): area-weighted triangle picking"""
    import grad_gpu_cases as GC
    scene = FC.mesh_room(tmp_path, n, mixed=mixed)
    sd = scene.data()
    assert sd.n_emitters == (4 if mixed else 1) and sum(int(sd.emitters[e].is_mesh) for e in range(sd.n_emitters)) == 1
    assert (sd.tri_verts.shape[0] * GC.TSHADE_BYTES > 64 * 1024) == (which == "large")        # the tables leave LDS
    _, vs = check_steady(film, tier, scene, -1, f"L_inf mesh {which}")
    print(f"[furnace] mesh, {tier} {which}: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs))


# -- 4. extended shading ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bitmap", "lobes"])
@pytest.mark.parametrize("tier", TIERS)
def test_extended_shading(film, host_harness, tier, tmp_path, which):
    scene = FC.bitmap_room(tmp_path, extra={"far": FC.far_rough_conductor()} if which == "lobes" else None)
    traits, ext, _, _ = host_class(host_harness, scene)
    assert ext and bool(traits & NO_LOBES) == (which == "bitmap")
    _, vs = check_steady(film, tier, scene, -1, f"L_inf {which}")
    print(f"[furnace] extended, {tier} {which}: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs))


# -- 5. polarized ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glass", [False, True], ids=["empty", "glass"])
@pytest.mark.parametrize("tier", TIERS)
def test_polarized_room_stays_unpolarized(hp, tier, glass):
    scene = FC.polarized_room(glass, FC.CPU_SIZE)
    spp = FC.CPU_SIZE[1]
    if tier == "oracle":
        t4, s4, _, _ = P.oracle_render(scene, seed=0, spp=spp)
    else:
        t4, s4, _ = P.hp_render(hp, scene, seed=0, spp=spp)
    assert np.all(s4[..., 3] == spp)                                   # every sample has weight 1: dividing by it is the 1 / spp below
    vs = FC.stokes_verdicts(t4)
    FC.assert_verdict(vs["S0"], f"polarized {tier} S0")
    FC.assert_verdict(vs["S123"], f"polarized {tier} S1..S3")
    steady = FC.verdict(FC.pixels(P.steady_s0(s4)), FC.radiance(-1, FC.POL_RHO, FC.POL_LE), FC.neighbours(-1, FC.POL_RHO, FC.POL_LE))
    FC.assert_verdict(steady, f"polarized {tier} steady S0")
    if glass:
        assert np.abs(np.asarray(t4)[..., 1:]).max() > 0               # single paths ARE polarized: the mean is what vanishes
    print(f"[furnace] polarized, {tier} glass={glass}: worst |z| %.2f, worst se/expected %.2e" % FC.worst([vs["S0"], vs["S123"], steady]))


# -- 6. derivatives --------------------------------------------------------------------------------------------------------------
def _seeded_grads(scene, grad):
    g_s, g_t = FC.mean_upstream(scene)
    return [grad(FC.params_of(scene, seed), g_s, g_t) for seed in range(FC.GRAD_SEEDS)]


@pytest.mark.parametrize("D,rr", [(4, 5), (-1, 3)])
def test_reverse_mode_sums(hg, D, rr):
    """sum over the six walls of d / d rho = Le sum k rho^(k-1), of d / d Le = sum rho^k (L_inf: Le / (1 - rho)^2, 1 / (1 - rho)),
    the standard error from 16 gradient seeds"""
    scene = FC.room(D, rr, FC.grad_size(D))
    mats, ems = FC.wall_indices(scene)
    assert len(mats) == len(ems) == 6
    out = _seeded_grads(scene, lambda p, g_s, g_t: T.host_grad(hg, scene, p, g_s, g_t))
    vs = FC.grad_verdicts(np.array([gm[mats].sum(0) for gm, _ in out]), np.array([ge[ems].sum(0) for _, ge in out]), D)
    for k, v in vs.items():
        FC.assert_verdict(v, f"reverse D={D} {k}")
    print(f"[furnace] reverse mode D={D}: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs.values()))


def test_reverse_mode_texel_sums(hgt, tmp_path):
    """rho as a constant bitmap: the texel gradients of the six bitmaps, summed, are the walls' d / d rho"""
    scene = FC.bitmap_room(tmp_path, 4, 5, FC.GRAD_SIZE)
    _, ems = FC.wall_indices(scene)
    out = _seeded_grads(scene, lambda p, g_s, g_t: X.host_grad_tex(hgt, scene, p, g_s, g_t))
    assert all(np.all(gm == 0.0) for gm, _, _ in out)                  # a textured material's own entry stays 0
    vs = FC.grad_verdicts(np.array([sum(g.sum(axis=(0, 1)) for g in gx) for _, _, gx in out]),
                          np.array([ge[ems].sum(0) for _, ge, _ in out]), 4)
    for k, v in vs.items():
        FC.assert_verdict(v, f"reverse, texels {k}")
    print("[furnace] reverse mode, texels: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs.values()))


@pytest.mark.parametrize("D,rr", [(4, 5), (-1, 3)])
def test_forward_mode_tangent_images(hf, D, rr):
    """d rho = 1 on every wall, then d Le = 1 on every emitter: the tangent image's pixels"""
    scene = FC.room(D, rr, FC.FWD_SIZE_INF_CPU if D < 0 else FC.CPU_SIZE)
    orders = FC.wrong_orders(D)
    vs = []
    for what, f in (("rho", FC.d_radiance_d_rho), ("le", FC.d_radiance_d_le)):
        s, _ = F.host_fwd(hf, scene, FC.params_of(scene), FC.unit_tangents(scene, what))
        vs.append(FC.verdict(FC.pixels(s), f(D), [f(x) for x in orders]))
        FC.assert_verdict(vs[-1], f"forward D={D} d_{what}")
    print(f"[furnace] forward mode D={D}: worst |z| %.2f, worst se/expected %.2e" % FC.worst(vs))


# -- camera ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FC.CAMERAS))
def test_camera_rays_are_the_pinholes(oracle, host_harness, name):
    """oracle.camera_ray within 2e-6 of the f64 pinhole in direction and in origin (the near-clip offset included); the host
    harness exports no ray, so its camera is held through a render: its D = 2 room equals the oracle's at the suite's 1e-5"""
    scene = FC.camera_room(name)
    sd = scene.data()
    ox, oy = (FC.CAMERAS[name][3] or (0, 0, 0, 0))[2:]
    for px, py, jx, jy in FC.camera_samples(name):
        o, d, _ = oracle.camera_ray(sd, ox + px, oy + py, jx, jy)           # (the oracle takes film coordinates)
        ro, rd = FC.pinhole_ray(name, px, py, jx, jy)
        assert np.abs(d - rd).max() <= 2e-6 and np.abs(o - ro).max() <= 2e-6, (name, px, py, jx, jy, d, rd, o, ro)
    (s_o, t_o), (s_h, t_h) = FC.oracle_film(scene), FC.host_film(host_harness, scene)
    assert np.abs(t_o).max() > 0 and rel_l2(t_h, t_o) <= 1e-5 and rel_l2(s_h, s_o) <= 1e-5
