"""The *_mono_polarized variants (mitransient's polarization tracking) on the CPU: the variant and ingestion surface, the
Mueller / Fresnel building blocks of mtr_polar.h and of the CPU oracle's f64 polarized path against f64 numpy, whole renders
of the host build of the same arithmetic (tests/host_polarized.cpp) against the oracle (oracle/mtr_oracle.c, f64 Mueller
algebra written apart from mtr_polar.h) on a scene per polarized BSDF — and, for both implementations, the diffuse Cornell
box against the unpolarized render, Brewster's angle, two conductor reflections against Jones calculus, and a rolled camera."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import hh_render, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(ROOT, "tests", "golden", "reference_scenes", "transient", "cornell-box")
FP = C.POINTER(C.c_float)
# the reference scene's gold is the `Au` preset of Mitsuba's spectral IOR tables, which this project does not have: the
# comparisons replace it by this explicit gold-like index (a SUBSTITUTION, not the preset's value)
GOLD_ETA, GOLD_K = 0.47, 2.4


# ---------------------------------------------------------------- builds and helpers
def build_host_polarized():
    """tests/host_polarized.cpp with the flags of build_host_harness() (__graft_entry__.py)"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libhost_polarized.so")
    csrc = os.path.join(ROOT, "mitransient_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "host_polarized.cpp"), os.path.join(csrc, "mtr_scene_host.cpp"), os.path.join(csrc, "mtr_bvh.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("mtr_core.h", "mtr_polar.h", "mtr_scene_host.h", "mtr_bvh.h", "mtr_knobs.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-DMTR_EXPERIMENTS", "-o", tmp] + srcs, check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def hp():
    return C.CDLL(build_host_polarized())


def hp_render(lib, scene, seed=0, spp=4):
    """a whole polarized render of the host build: (H, W, T, 4) Stokes sums, (H, W, 4) = (S0, S1, S2, weight), counters"""
    from mitransient_amd import _cabi
    sd = scene.data()
    f = sd.film
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)
    t4 = np.zeros((f.height, f.width, f.temporal_bins, 4), np.float32)
    s4 = np.zeros((f.height, f.width, 4), np.float32)
    cnt = _cabi.mtr_counters()
    d = sd.desc()
    assert lib.hp_render(C.byref(d), C.byref(p), t4.ctypes.data_as(FP), s4.ctypes.data_as(FP), C.byref(cnt)) == 0
    return t4, s4, cnt.as_dict()


def oracle_render(scene, seed=0, spp=4, **params):
    """the CPU oracle's polarized render: (H, W, T, 4) S0..S3, (H, W, 4) = (S0, S1, S2, weight), counters, and the (H, W)
    pixels where a Russian-roulette decision lay within 1e-5 of its threshold.  ``params``: render_params' keyword arguments"""
    from oracle import oracle
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp, **params)
    return oracle.render_polarized(scene.data(), p, use_bvh=True)


# the parity bar of every polarized comparison with the oracle (the GPU's against the host build too)
TOL, TOL_CHANNEL = 1e-5, 1e-4
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")


def steady_s0(s4):
    """the developed steady image (H, W, 1): S0 / weight"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s4[..., 3:] > 0, s4[..., :1] / s4[..., 3:], 0.0).astype(np.float32)


def assert_matches_oracle(t, s, counters, ref, max_near=0.01):
    """a polarized render against the oracle's `ref` = oracle_render(...): rel-L2 <= TOL on the transient (H, W, T, 4) and the
    steady image — (H, W, 1) developed S0 or the (H, W, 4) accumulator — and <= TOL_CHANNEL on each Stokes channel, outside the
    pixels whose roulette decision sat on its threshold (under max_near of the film); the counters equal where none did"""
    ot, os4, oc, near = ref
    assert t.shape == ot.shape
    assert near.mean() < max_near, near.mean()
    keep = ~near
    os_ = steady_s0(os4) if s.shape[-1] == 1 else os4
    # (a developed steady image with a crop window is (crop_h, crop_w, 1): the accumulator's top-left corner)
    os_, skeep = os_[:s.shape[0], :s.shape[1]], keep[:s.shape[0], :s.shape[1]]
    assert np.abs(ot[..., 0]).max() > 0
    assert rel_l2(t[keep], ot[keep]) <= TOL, rel_l2(t[keep], ot[keep])
    assert rel_l2(s[skeep], os_[skeep]) <= TOL, rel_l2(s[skeep], os_[skeep])
    for k in range(4):
        e = rel_l2(t[keep][..., k], ot[keep][..., k])
        assert e <= TOL_CHANNEL, (k, e)
    if not near.any():
        for k in COUNTERS:
            assert counters[k] == oc[k], (k, counters[k], oc[k])


def cbox_polarized_dict(**params):
    """cornell-box/cbox_polarized.xml (reference examples/polarization) as a dictionary, `Au` replaced by GOLD_ETA / GOLD_K"""
    from mitransient_amd.xml_loader import xml_to_dict
    d = xml_to_dict(os.path.join(CBOX, "cbox_polarized.xml"), **params)
    gold = d["gold"]
    assert gold.pop("material") == "Au"
    gold["eta"], gold["k"] = GOLD_ETA, GOLD_K
    return d


def load_cbox_polarized(variant="llvm_ad_mono_polarized", **params):
    import mitransient_amd.mi as mi
    mi.set_variant(variant)
    return mi.load_dict(cbox_polarized_dict(**params), base_dir=CBOX)


def mat16(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(16))


def call16(fn, *args):
    out = np.zeros(16, np.float32)
    fn(*args, out.ctypes.data_as(FP))
    return out.reshape(4, 4)


def fvec(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def rotator64(theta):
    c, s = math.cos(2 * theta), math.sin(2 * theta)
    return np.array([[1, 0, 0, 0], [0, c, s, 0], [0, -s, c, 0], [0, 0, 0, 1]], np.float64)


def fresnel_amplitudes64(ci, eta):
    """f64 s / p amplitudes of reflection, the sign convention of mitsuba's fresnel_polarized (a_p = (cos_t - eta cos_i) /
    (cos_t + eta cos_i)); eta complex for conductors (light from outside)"""
    eta = complex(eta)
    s2 = 1.0 - ci * ci
    ct = np.sqrt(complex(1.0 - s2 / (eta * eta)))
    if ct.real < 0 or (ct.real == 0 and ct.imag < 0):
        ct = -ct
    a_s = (ci - eta * ct) / (ci + eta * ct)
    a_p = (ct - eta * ci) / (ct + eta * ci)
    return a_s, a_p


def reflection_mueller64(ci, eta):
    a_s, a_p = fresnel_amplitudes64(ci, eta)
    rs, rp = abs(a_s) ** 2, abs(a_p) ** 2
    z = a_s * np.conj(a_p)
    d = abs(z)
    cd, sd = (z.real / d, z.imag / d) if d > 0 else (0.0, 0.0)
    a, b, c = 0.5 * (rs + rp), 0.5 * (rs - rp), math.sqrt(rs * rp)
    return np.array([[a, b, 0, 0], [b, a, 0, 0], [0, 0, c * cd, c * sd], [0, 0, -c * sd, c * cd]])


# ---------------------------------------------------------------- 1. variants and ingestion
def test_polarized_variants_are_accepted():
    import mitransient_amd.mi as mi
    from mitransient_amd import variant
    for v in ("llvm_ad_mono_polarized", "cuda_ad_mono_polarized"):
        mi.set_variant(v)
        assert mi.variant() == v and mi.is_polarized and mi.is_monochromatic() and variant.is_monochromatic()
    mi.set_variant("llvm_ad_mono")
    assert not mi.is_polarized and mi.is_monochromatic()
    mi.set_variant("llvm_ad_rgb")
    assert not mi.is_polarized and not mi.is_monochromatic()


@pytest.mark.parametrize("name", ["llvm_ad_rgb_polarized", "cuda_ad_rgb_polarized", "scalar_mono_polarized", "scalar_rgb",
                                  "llvm_ad_spectral", "llvm_ad_spectral_polarized", "cuda_ad_mono_polarized_double"])
def test_unsupported_variants_name_what_is_supported(name):
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    with pytest.raises(ValueError, match="llvm_ad_mono_polarized"):
        mi.set_variant(name)
    assert mi.variant() == "llvm_ad_rgb"


def test_reference_scene_loads_except_for_the_gold_preset():
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_mono_polarized")
    with pytest.raises(ValueError, match="material presets"):           # `Au`: no spectral IOR tables here
        mi.load_file(os.path.join(CBOX, "cbox_polarized.xml"), res=8).data()      # (scenes are flattened on first use)
    scene = load_cbox_polarized(res=8)
    sd = scene.data()
    f = sd.film
    assert (f.width, f.height, f.temporal_bins) == (8, 8, 400)
    from mitransient_amd import _cabi
    types = sorted({int(sd.materials[i].type) for i in range(sd.n_materials)})
    assert types == [_cabi.MTR_BSDF_DIFFUSE, _cabi.MTR_BSDF_ROUGHCONDUCTOR]
    params = scene.integrator().render_params(scene.sensors()[0].film(), 0, 4)
    assert params.flags & _cabi.MTR_FLAG_POLARIZED
    mi.set_variant("llvm_ad_mono")
    assert not (scene.integrator().render_params(scene.sensors()[0].film(), 0, 4).flags & _cabi.MTR_FLAG_POLARIZED)


def _small_scene(bsdf=None, emitter=None, integrator="transient_path", film_type="transient_hdr_film", variant="llvm_ad_mono_polarized"):
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant(variant)
    film = {"type": film_type, "width": 4, "height": 4, "temporal_bins": 8, "start_opl": 0, "bin_width_opl": 1,
            "rfilter": {"type": "box"}}
    return mi.load_dict({
        "type": "scene",
        "integrator": {"type": integrator},
        "sensor": {"type": "perspective", "fov": 40, "to_world": T().look_at([0, 0, 4], [0, 0, 0], [0, 1, 0]), "film": film},
        "floor": {"type": "rectangle", "bsdf": bsdf or {"type": "diffuse"}},
        "light": {"type": "rectangle", "to_world": T().translate([0, 0, 2]).rotate([1, 0, 0], 180),
                  "emitter": emitter or {"type": "area", "radiance": 1.0}},
    })


@pytest.mark.parametrize("bsdf", [{"type": "diffuse"}, {"type": "conductor", "eta": 0.2, "k": 3.0},
                                  {"type": "roughconductor", "alpha": 0.2, "distribution": "ggx"},
                                  {"type": "roughconductor", "alpha_u": 0.1, "alpha_v": 0.3, "distribution": "beckmann"},
                                  {"type": "dielectric", "int_ior": 1.5},
                                  {"type": "twosided", "bsdf": {"type": "roughconductor", "alpha": 0.3}}])
def test_bsdfs_in_scope_load(bsdf):
    assert _small_scene(bsdf=bsdf).data().n_materials == 2           # (and the light's default diffuse)


@pytest.mark.parametrize("bsdf", [{"type": "plastic"}, {"type": "roughplastic"}, {"type": "roughdielectric", "alpha": 0.1},
                                  {"type": "thindielectric"}, {"type": "twosided", "bsdf": {"type": "plastic"}}])
def test_bsdfs_out_of_scope_are_refused(bsdf):
    with pytest.raises(ValueError, match="not available with polarization"):
        _small_scene(bsdf=bsdf).data()
    _small_scene(bsdf=bsdf, variant="llvm_ad_mono").data()          # (the unpolarized variant keeps them)


def test_other_plugins_out_of_scope_are_refused():
    with pytest.raises(ValueError, match="angulararea emitter is not available with polarization"):
        _small_scene(emitter={"type": "angulararea", "cutoff_angle": 30}).data()
    with pytest.raises(ValueError, match="polarized"):
        _small_scene(film_type="phasor_hdr_film").data()
    from conftest import make_nlos
    import mitransient_amd.mi as mi
    scene = make_nlos()                                      # (make_nlos selects llvm_ad_rgb)
    mi.set_variant("llvm_ad_mono_polarized")
    with pytest.raises(ValueError, match="transient_nlos_path is not available"):
        scene.data()


def test_deterministic_rows_are_refused():
    """amd_deterministic asks for fixed-point rows, which the Stokes film does not have: an error naming the key, not a
    render that quietly sums f32 atomics (the C-ABI refuses MTR_FLAG_DETERMINISTIC too: tests/test_gpu_polarized.py)"""
    import mitransient_amd.mi as mi
    from mitransient_amd import _cabi
    from mitransient_amd.transform import ScalarTransform4f as T
    d = {"type": "scene", "integrator": {"type": "transient_path", "amd_deterministic": True},
         "sensor": {"type": "perspective", "to_world": T().look_at([0, 0, 4], [0, 0, 0], [0, 1, 0]),
                    "film": {"type": "transient_hdr_film", "width": 4, "height": 4, "temporal_bins": 8, "rfilter": {"type": "box"}}},
         "floor": {"type": "rectangle", "bsdf": {"type": "diffuse"}}}
    mi.set_variant("llvm_ad_mono_polarized")
    scene = mi.load_dict(d)
    with pytest.raises(ValueError, match="amd_deterministic"):
        scene.integrator().render_params(scene.sensors()[0].film(), 0, 4)
    mi.set_variant("llvm_ad_mono")                 # (the unpolarized variants keep their deterministic rows)
    scene = mi.load_dict(d)
    assert scene.integrator().render_params(scene.sensors()[0].film(), 0, 4).flags & _cabi.MTR_FLAG_DETERMINISTIC


def test_multi_gpu_sharding_is_refused():
    import torch.distributed as dist
    from mitransient_amd.distributed import DistributedRenderer
    if dist.is_initialized():
        pytest.skip("a process group is already initialised")
    scene = _small_scene()

    class Fake:                         # a two-rank world without a process group
        pass
    r = DistributedRenderer(scene)
    orig = dist.is_initialized, dist.get_world_size, dist.get_rank
    dist.is_initialized, dist.get_world_size, dist.get_rank = (lambda: True), (lambda group=None: 2), (lambda group=None: 0)
    try:
        with pytest.raises(NotImplementedError, match="polarized"):
            r.render(spp=4)
    finally:
        dist.is_initialized, dist.get_world_size, dist.get_rank = orig


# ---------------------------------------------------------------- 2. Mueller algebra
def test_rotators_are_orthogonal_and_compose(hp):
    rng = np.random.default_rng(1)
    for _ in range(50):
        fwd = rng.normal(size=3); fwd /= np.linalg.norm(fwd)
        basis = []
        for _ in range(3):
            v = rng.normal(size=3); v -= fwd * (v @ fwd); basis.append(v / np.linalg.norm(v))
        a, b, c = basis
        Rab = call16(hp.hp_rotate_stokes_basis, fvec(fwd), fvec(a), fvec(b)).astype(np.float64)
        Rbc = call16(hp.hp_rotate_stokes_basis, fvec(fwd), fvec(b), fvec(c)).astype(np.float64)
        Rac = call16(hp.hp_rotate_stokes_basis, fvec(fwd), fvec(a), fvec(c)).astype(np.float64)
        assert np.abs(Rab @ Rab.T - np.eye(4)).max() < 1e-6
        assert np.abs(Rbc @ Rab - Rac).max() < 1e-5
        # the sense: theta from a to b, negative when dot(fwd, cross(a, b)) < 0 (mueller.h rotate_stokes_basis)
        theta = math.atan2(fwd @ np.cross(a, b), a @ b)
        assert np.abs(Rab - rotator64(theta)).max() < 1e-5


def test_stokes_basis_is_orthonormal(hp):
    rng = np.random.default_rng(2)
    w = rng.normal(size=(200, 3)); w /= np.linalg.norm(w, axis=1, keepdims=True)
    w[:3] = [[0, 0, 1], [0, 0, -1], [1, 0, 0]]
    w = np.ascontiguousarray(w, np.float32)
    b = np.zeros_like(w)
    hp.hp_stokes_basis(len(w), w.ctypes.data_as(FP), b.ctypes.data_as(FP))
    assert np.abs(np.linalg.norm(b, axis=1) - 1).max() < 1e-6 and np.abs((b * w).sum(1)).max() < 1e-6


def test_to_world_mueller_keeps_a_depolarizer(hp):
    rng = np.random.default_rng(3)
    D = np.zeros((4, 4), np.float32); D[0, 0] = 0.37
    for _ in range(20):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        wi = rng.normal(size=3); wi /= np.linalg.norm(wi)
        wo = rng.normal(size=3); wo /= np.linalg.norm(wo)
        out = call16(hp.hp_to_world_mueller, mat16(D).ctypes.data_as(FP), fvec(q.T.reshape(-1)), fvec(wi), fvec(wo))
        np.testing.assert_array_equal(out, D)


def _physical(M):
    """M maps physical Stokes vectors (S0 >= |S1..S3|) to physical ones: checked on the pure states and the unpolarized one"""
    rng = np.random.default_rng(4)
    v = rng.normal(size=(300, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    S = np.concatenate([np.ones((300, 1)), v], axis=1)
    S = np.concatenate([S, [[1, 0, 0, 0]]])
    out = S @ M.astype(np.float64).T
    return np.all(out[:, 0] + 2e-6 * np.abs(M).max() >= np.linalg.norm(out[:, 1:], axis=1))


def test_conductor_mueller_against_f64_and_the_scalar_fresnel(hp):
    ci = np.ascontiguousarray(np.linspace(0.0, 1.0, 257)[1:], np.float32)
    for er, ei in ((0.47, 2.4), (0.2, 3.0), (1.5, 0.0), (2.0, 5.0)):
        M = np.zeros((len(ci), 16), np.float32)
        hp.hp_conductor_reflection(len(ci), ci.ctypes.data_as(FP), C.c_float(er), C.c_float(ei), M.ctypes.data_as(FP))
        F = np.zeros(len(ci), np.float32)
        hp.hp_fresnel_scalar(0, len(ci), ci.ctypes.data_as(FP), C.c_float(er), C.c_float(ei), F.ctypes.data_as(FP))
        np.testing.assert_array_equal(M[:, 0], F)                    # M00 IS fresnel_conductor (same operations)
        for i in range(0, len(ci), 8):
            ref = reflection_mueller64(float(ci[i]), complex(er, ei))
            assert np.abs(M[i].reshape(4, 4) - ref).max() < 2e-5, (er, ei, ci[i])
            assert _physical(M[i].reshape(4, 4))


def test_dielectric_mueller_against_f64_and_the_scalar_fresnel(hp):
    ci = np.ascontiguousarray(np.concatenate([np.linspace(-1, 0, 129)[:-1], np.linspace(0, 1, 129)[1:]]), np.float32)
    for eta in (1.5, 1.33, 1 / 1.5):
        R = np.zeros((len(ci), 16), np.float32)
        T = np.zeros((len(ci), 16), np.float32)
        hp.hp_dielectric(len(ci), ci.ctypes.data_as(FP), C.c_float(eta), 0, R.ctypes.data_as(FP))
        hp.hp_dielectric(len(ci), ci.ctypes.data_as(FP), C.c_float(eta), 1, T.ctypes.data_as(FP))
        F = np.zeros(len(ci), np.float32)
        hp.hp_fresnel_scalar(1, len(ci), ci.ctypes.data_as(FP), C.c_float(eta), C.c_float(0), F.ctypes.data_as(FP))
        np.testing.assert_array_equal(R[:, 0], F)                    # M00 IS fresnel_dielectric's r (TIR included)
        # transmission: M00 = 1 - F within 4 ulp of 1 (other operations: (1 + a_s)^2 cos_t / cos_i ...); 0 under TIR
        tir = F == 1.0
        assert np.abs(T[~tir, 0] - (1.0 - F[~tir].astype(np.float64))).max() <= 4 * 2.0 ** -23
        assert np.all(T[tir] == 0)
        for i in range(0, len(ci), 6):
            c = float(ci[i])
            e = eta if c >= 0 else 1.0 / eta
            ref = reflection_mueller64(abs(c), e)
            assert np.abs(R[i].reshape(4, 4) - ref).max() < 2e-5, (eta, c)
            assert _physical(R[i].reshape(4, 4)) and _physical(T[i].reshape(4, 4))


def test_total_internal_reflection_has_a_phase(hp):
    # inside glass beyond the critical angle: r_s = r_p = 1 and the s / p phase difference of the f64 amplitudes
    ci = np.array([-0.3, -0.5], np.float32)
    R = np.zeros((2, 16), np.float32)
    hp.hp_dielectric(2, ci.ctypes.data_as(FP), C.c_float(1.5), 0, R.ctypes.data_as(FP))
    for i in range(2):
        ref = reflection_mueller64(abs(float(ci[i])), 1.0 / 1.5)
        assert abs(ref[2, 3]) > 0.1
        assert np.abs(R[i].reshape(4, 4) - ref).max() < 2e-6


# ---------------------------------------------------------------- 3. the diffuse Cornell box
def host_renderer(lib):
    return lambda scene, seed=0, spp=4: hp_render(lib, scene, seed=seed, spp=spp)


def oracle_renderer(scene, seed=0, spp=4):
    return oracle_render(scene, seed=seed, spp=spp)[:3]


def test_diffuse_cornell_box_matches_the_unpolarized_render(hp, host_harness):
    """S0 of the polarized path IS the unpolarized render on a scene of depolarizers: every Mueller product's M00 is the
    scalar product (its other terms are exact zeros) and the sampler is consumed in the same order — bit equality"""
    _check_diffuse_box(host_renderer(hp), lambda sd, p: hh_render(host_harness, sd, p), exact=True)


def test_diffuse_cornell_box_matches_the_unpolarized_render_in_the_oracle():
    """the same for the oracle, whose polarized S0 is f64 arithmetic against its own f32 unpolarized render: within 1e-6"""
    from oracle import oracle
    _check_diffuse_box(oracle_renderer, lambda sd, p: oracle.render(sd, p, use_bvh=True), exact=False)


def _check_diffuse_box(render, render_unpolarized, exact):
    import mitransient_amd.mi as mi
    path = os.path.join(CBOX, "cbox_diffuse.xml")
    mi.set_variant("llvm_ad_mono")
    su = mi.load_file(path, res=16, spp=8)
    p = su.integrator().render_params(su.sensors()[0].film(), 5, 8)
    tu, s4u, cu = render_unpolarized(su.data(), p)
    mi.set_variant("llvm_ad_mono_polarized")
    sp = mi.load_file(path, res=16, spp=8)
    tp, s4p, cp = render(sp, seed=5, spp=8)
    assert tu.shape == tp.shape
    assert not np.any(tp[..., 1:])
    if exact:
        np.testing.assert_array_equal(tp[..., 0], tu[..., 0])
        np.testing.assert_array_equal(s4p[..., 0], s4u[..., 0])
    else:
        assert rel_l2(tp[..., 0], tu[..., 0]) <= 1e-6 and rel_l2(s4p[..., 0], s4u[..., 0]) <= 1e-6
    np.testing.assert_array_equal(s4p[..., 3], s4u[..., 3])
    np.testing.assert_array_equal(tp[..., 0] != 0, tu[..., 0] != 0)
    for k in ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces"):
        assert cp[k] == cu[k], k
    assert tu[..., 0].sum() > 0


# ---------------------------------------------------------------- 4. / 6. Brewster's angle, a rolled camera
BREWSTER = math.atan(1.5)
D_CAM, D_LIGHT, NEAR = 4.0, 3.0, 0.5


def _brewster_scene(roll_deg=0.0, res=3, fov=0.5, theta=BREWSTER):
    """a smooth dielectric plane (int_ior 1.5) in z = 0, seen at `theta` from its normal in the y-z plane by a narrow camera;
    a large area light in the mirror direction faces the plane.  s polarization is along x, the camera's horizontal axis
    (rolled by roll_deg about the view direction)"""
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant("llvm_ad_mono_polarized")
    cam = np.array([0.0, -math.sin(theta), math.cos(theta)]) * D_CAM
    light = np.array([0.0, math.sin(theta), math.cos(theta)]) * D_LIGHT
    d = -cam / np.linalg.norm(cam)
    up = np.array([0.0, 0.0, 1.0]); up = up - d * (up @ d); up /= np.linalg.norm(up)
    a = math.radians(roll_deg)
    up = up * math.cos(a) + np.cross(d, up) * math.sin(a)
    bw = 0.25
    opl = (D_CAM - NEAR) + D_LIGHT                             # camera ray from the near plane, then plane -> light
    start = opl - 2.5 * bw
    return mi.load_dict({
        "type": "scene",
        "integrator": {"type": "transient_path", "max_depth": 4},
        "sensor": {"type": "perspective", "fov": fov, "near_clip": NEAR, "far_clip": 100.0,
                   "to_world": T().look_at(list(cam), [0, 0, 0], list(up)),
                   "film": {"type": "transient_hdr_film", "width": res, "height": res, "temporal_bins": 5,
                            "start_opl": start, "bin_width_opl": bw, "rfilter": {"type": "box"}}},
        "plane": {"type": "rectangle", "to_world": T().scale([2, 2, 1]), "bsdf": {"type": "dielectric", "int_ior": 1.5}},
        "light": {"type": "rectangle", "to_world": T().look_at(list(light), [0, 0, 0], [0, 0, 1]).scale([2, 2, 1]),
                  "emitter": {"type": "area", "radiance": 1.0}},
    }), cam, d, up


def _dolp(S):
    return np.hypot(S[1], S[2]) / S[0]


def test_brewster_reflection_is_linearly_polarized(hp):
    _check_brewster(host_renderer(hp))


def test_brewster_reflection_is_linearly_polarized_in_the_oracle():
    _check_brewster(oracle_renderer)


def _check_brewster(render):
    scene, cam, d, up = _brewster_scene()
    t4, s4, _ = render(scene, spp=64)
    # all of it in the analytically known bin: (D_CAM - near) + D_LIGHT lies in the middle of bin 2
    per_bin = np.abs(t4[..., 0]).sum(axis=(0, 1))
    assert per_bin[2] > 0 and per_bin.sum() == per_bin[2]
    S = t4.sum(axis=(0, 1, 2)).astype(np.float64)
    # f64 Fresnel over the pixels' angles (half the diagonal of a 0.5 degree field around Brewster's angle): the
    # reflected light's degree of linear polarization is (r_s - r_p) / (r_s + r_p)
    worst = 1.0
    for dth in np.linspace(-0.36, 0.36, 9):
        a_s, a_p = fresnel_amplitudes64(math.cos(BREWSTER + math.radians(dth)), 1.5)
        rs, rp = abs(a_s) ** 2, abs(a_p) ** 2
        worst = min(worst, (rs - rp) / (rs + rp))
    assert worst > 0.999
    assert _dolp(S) >= 0.999 and _dolp(S) >= worst - 1e-6
    # s polarization is horizontal in the camera's Stokes frame (beta_init: basis cross(d, up)): S1 = +S0, S2 = S3 = 0.  (Off
    # the image's vertical centre line the plane of incidence tilts by up to ~0.3 degrees: S2 / S0 of a pixel is up to ~1e-2
    # and cancels between the left and right columns up to the jitter of 64 samples — 9e-4 measured)
    assert S[1] / S[0] > 0.999 and abs(S[2] / S[0]) < 3e-3 and abs(S[3] / S[0]) < 1e-6
    # S0: the reflectance r_s / 2 of the unpolarized light (radiance 1).  The reflected lobe is picked with probability F =
    # r_s / 2 and then weighs R / F (M00 = 1): a Bernoulli estimate — within 4 of its standard deviations
    a_s, _ = fresnel_amplitudes64(math.cos(BREWSTER), 1.5)
    F, n = 0.5 * abs(a_s) ** 2, float(s4[..., 3].sum())
    assert abs(s4[..., 0].sum() / n - F) < 4 * math.sqrt(F * (1 - F) / n)


def test_away_from_brewster_the_reflection_is_partly_polarized(hp):
    theta = math.radians(30.0)
    scene, *_ = _brewster_scene(theta=theta)
    t4, _, _ = hp_render(hp, scene, spp=64)
    S = t4.sum(axis=(0, 1, 2)).astype(np.float64)
    a_s, a_p = fresnel_amplitudes64(math.cos(theta), 1.5)
    rs, rp = abs(a_s) ** 2, abs(a_p) ** 2
    assert abs(S[1] / S[0] - (rs - rp) / (rs + rp)) < 2e-3


ROLLS = [15.0, 30.0, -40.0, 90.0]


@pytest.mark.parametrize("roll", ROLLS)
def test_camera_roll_rotates_the_linear_components(hp, roll):
    """rolling the camera by alpha about its axis rotates (S1, S2) by 2 alpha; S0 and S3 stay.  The sense is the one beta_init
    implies: psi = the angle from the camera's basis cross(d, up) to the polarization direction x, positive about the
    propagation direction -d (mueller.h rotate_stokes_basis), S = S0 DoLP (cos 2 psi, sin 2 psi)"""
    _check_camera_roll(host_renderer(hp), roll)


@pytest.mark.parametrize("roll", ROLLS)
def test_camera_roll_rotates_the_linear_components_in_the_oracle(roll):
    _check_camera_roll(oracle_renderer, roll)


def _check_camera_roll(render, roll):
    s0, *_ = _brewster_scene(0.0)
    s1, cam, d, up = _brewster_scene(roll)
    t0, _, _ = render(s0, spp=64)
    t1, _, _ = render(s1, spp=64)
    A = t0.sum(axis=(0, 1, 2)).astype(np.float64)
    B = t1.sum(axis=(0, 1, 2)).astype(np.float64)
    assert abs(B[0] - A[0]) <= 1e-3 * A[0] and abs(B[3] - A[3]) <= 1e-6 * A[0]
    b = np.cross(d, up); b /= np.linalg.norm(b)
    e = np.array([1.0, 0.0, 0.0])
    psi = math.atan2(-d @ np.cross(b, e), b @ e)
    lin = math.hypot(A[1], A[2])
    assert abs(B[1] - lin * math.cos(2 * psi)) < 2e-3 * A[0]
    assert abs(B[2] - lin * math.sin(2 * psi)) < 2e-3 * A[0]
    assert abs(abs(psi) - math.radians(abs(roll))) < 1e-6 or abs(abs(psi) - math.radians(180 - abs(roll))) < 1e-6


# ---------------------------------------------------------------- 5. two conductor reflections
def _jones_reflect(E, fwd_in, n, fwd_out, eta):
    """f64 Jones calculus of one specular reflection on a 3-vector field: s = n x fwd (normalised) on both sides, p = fwd x s,
    E_out = a_s (E . s_in) s_out + a_p (E . p_in) p_out"""
    a_s, a_p = fresnel_amplitudes64(float(-fwd_in @ n), eta)
    s_in = np.cross(n, fwd_in); s_in /= np.linalg.norm(s_in)
    s_out = np.cross(n, fwd_out); s_out /= np.linalg.norm(s_out)
    return a_s * (E @ s_in) * s_out + a_p * (E @ np.cross(fwd_in, s_in)) * np.cross(fwd_out, s_out)


def test_two_conductor_reflections_against_jones_calculus(hp):
    _check_two_conductors(host_renderer(hp))


def test_two_conductor_reflections_against_jones_calculus_in_the_oracle():
    _check_two_conductors(oracle_renderer)


def _check_two_conductors(render):
    """camera -> gold mirror 1 -> gold mirror 2 -> area light, the two planes of incidence not coplanar (and not the symmetric
    45 / 45 degree crossing, whose polarizations cancel exactly).  Unpolarized light picks up linear and circular polarization;
    the f64 Jones prediction in the camera's Stokes frame (x = cross(d, up), y = fwd x x, fwd = -d; S3 = -2 Im(Ex conj(Ey)), the
    sign convention of mitsuba's Mueller matrices) against the render's sum over 3 x 3 pixels of a 0.5 degree field (the delta
    path's only spread: the pixels' angles — 4e-5 measured)"""
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant("llvm_ad_mono_polarized")
    d0 = np.array([1.0, 0, 0])
    d1 = np.array([0.2, 1, 0.3]); d1 /= np.linalg.norm(d1)
    d2 = np.array([-0.3, 0.6, 0.8]); d2 /= np.linalg.norm(d2)
    P1 = 2 * d0; P2 = P1 + 2 * d1; P3 = P2 + 2 * d2
    n1 = (d1 - d0) / np.linalg.norm(d1 - d0); n2 = (d2 - d1) / np.linalg.norm(d2 - d1)
    gold = {"type": "conductor", "eta": GOLD_ETA, "k": GOLD_K}
    scene = mi.load_dict({
        "type": "scene", "integrator": {"type": "transient_path", "max_depth": 4},
        "sensor": {"type": "perspective", "fov": 0.5, "near_clip": 0.01, "to_world": T().look_at([0, 0, 0], [1, 0, 0], [0, 0, 1]),
                   "film": {"type": "transient_hdr_film", "width": 3, "height": 3, "temporal_bins": 8, "start_opl": 0,
                            "bin_width_opl": 1, "rfilter": {"type": "box"}}},
        "m1": {"type": "rectangle", "to_world": T().look_at(list(P1), list(P1 + n1), [0, 0, 1]).scale(0.3), "bsdf": gold},
        "m2": {"type": "rectangle", "to_world": T().look_at(list(P2), list(P2 + n2), [0, 0, 1]).scale(0.3), "bsdf": gold},
        "light": {"type": "rectangle", "to_world": T().look_at(list(P3), list(P2), [1, 0, 0]), "emitter": {"type": "area", "radiance": 1.0}},
    })
    t4, s4, _ = render(scene, spp=16)
    per_bin = t4[..., 0].sum(axis=(0, 1))
    assert per_bin[5] > 0 and per_bin.sum() == per_bin[5]                 # opl 6 - near clip
    S = t4.sum(axis=(0, 1, 2)).astype(np.float64)
    S = S / S[0]
    eta = complex(GOLD_ETA, GOLD_K)
    up, d = np.array([0, 0, 1.0]), d0
    x = np.cross(d, up); x /= np.linalg.norm(x)
    y = np.cross(-d, x)
    b1 = np.cross(-d2, [1.0, 0, 0]); b1 /= np.linalg.norm(b1)
    J = np.zeros(4)
    for e in (b1, np.cross(-d2, b1)):                      # unpolarized: two incoherent orthogonal fields
        E = _jones_reflect(_jones_reflect(e.astype(complex), -d2, n2, -d1, eta), -d1, n1, -d0, eta)
        ex, ey = E @ x, E @ y
        J += [abs(ex) ** 2 + abs(ey) ** 2, abs(ex) ** 2 - abs(ey) ** 2, 2 * (ex * np.conj(ey)).real, -2 * (ex * np.conj(ey)).imag]
    J = J / J[0]
    assert abs(J[3]) > 0.05 and math.hypot(J[1], J[2]) > 0.1
    assert abs(S[3] - J[3]) < 2e-4
    assert abs(math.hypot(S[1], S[2]) - math.hypot(J[1], J[2])) < 2e-4
    assert np.abs(S[1:] - J[1:]).max() < 2e-4


# ---------------------------------------------------------------- 7. the reference's figures
# tests/golden/polarized_figures.npz (make_polarized_figures.py): the AoLP false colour of the notebooks, 8-bit, 256 x 256.
# A channel shows min(1, 255 s) of its sign, s = S_k / max(S0, 0.01) (polarized_visualization.py:255-269), so a figure pixel
# pins the SIGN of S1 or S2 wherever it is saturated, whatever the gold's exact index:
#   blue 255                   -> S2 < 0, and then green 255 / red 0 -> S1 > 0, red 255 / green 0 -> S1 < 0
#   red = green = 255, blue 0  -> S2 > 0 (S1 not seen: both of its channels are full)
#   blue 0, one of red / green 255 and the other 0 -> the sign of S1
def figure(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "polarized_figures.npz"))[name].astype(np.int32)


def figure_signs(fig):
    R, G, B = fig[..., 0], fig[..., 1], fig[..., 2]
    hi, lo = 250, 5
    s2 = np.where(B >= hi, -1, np.where((R >= hi) & (G >= hi) & (B <= lo), 1, 0))
    s1 = np.where((G >= hi) & (R <= lo), 1, np.where((R >= hi) & (G <= lo), -1, 0))
    s1 = np.where(s2 == 1, 0, s1)
    return s1, s2


def sign_agreement(stokes3, fig):
    """fractions of the figure's pinned pixels where sign(S1), sign(S2) of a render agree"""
    f1, f2 = figure_signs(fig)
    return [float((np.sign(stokes3[..., k]) == f)[f != 0].mean()) for k, f in ((1, f1), (2, f2))], [int((f1 != 0).sum()), int((f2 != 0).sum())]


def test_steady_figure_signs(hp):
    """the steady figure (Mitsuba's own stokes + path integrators) against the host build's steady Stokes image at 64 spp:
    the signs of S1 and S2 on the pixels the figure pins.  Measured: 0.941 / 0.940 of 4662 / 9718 pixels at 64 spp (0.961 /
    0.958 at 96, 0.871 / 0.803 at 16: the rest is the render's noise where |S_k| / S0 is small); the same render with S1, S2
    negated scores 0.059 / 0.059"""
    scene = load_cbox_polarized(res=256)
    _, s4, _ = hp_render(hp, scene, seed=0, spp=64)
    S = s4[..., :3] / np.maximum(s4[..., 3:], 1.0)
    (a1, a2), (n1, n2) = sign_agreement(S, figure("steady"))
    assert n1 > 4000 and n2 > 9000
    assert a1 >= 0.92 and a2 >= 0.92, (a1, a2)


# ---------------------------------------------------------------- 8. the host build against the oracle's f64 polarized path
def bsdf_scene(kind, res=16, bins=64, max_depth=8, rr_depth=5, back_bsdf=None, closed=False, film=None, **integrator):
    """a small box for one polarized lobe: a diffuse floor and back wall, two area lights (one overhead, one to the side, seen
    by the camera) and the lobe on a tilted cube — or, for 'twosided_back', on a tilted mirror whose front faces away from the
    camera.  back_bsdf replaces the back wall's; closed adds a ceiling and three walls around the camera; film: film keys"""
    import mitransient_amd.mi as mi
    from mitransient_amd.transform import ScalarTransform4f as T
    mi.set_variant("llvm_ad_mono_polarized")
    bsdfs = {
        "conductor": {"type": "conductor", "eta": GOLD_ETA, "k": GOLD_K},
        "roughconductor_ggx": {"type": "roughconductor", "alpha": 0.2, "distribution": "ggx", "eta": 0.2, "k": 3.0},
        "roughconductor_beckmann_aniso": {"type": "roughconductor", "alpha_u": 0.08, "alpha_v": 0.35,
                                          "distribution": "beckmann", "eta": 1.1, "k": 2.6},
        "glass": {"type": "dielectric", "int_ior": 1.5},
        "twosided_back": {"type": "twosided", "bsdf": {"type": "conductor", "eta": 0.44, "k": 3.7}},
    }
    if kind == "twosided_back":      # the normal (0, 0, 1) turned away from the camera, then tilted towards the floor
        obj = {"type": "rectangle", "to_world": T().translate([0, 0.8, 0]).rotate([1, 0, 0], 150).scale(0.7)}
    else:
        obj = {"type": "cube", "to_world": T().translate([0, 0.6, 0]).rotate([0, 1, 0], 35).rotate([1, 0, 0], 20).scale(0.5)}
    obj["bsdf"] = bsdfs[kind]
    integ = {"type": "transient_path", "max_depth": max_depth, "rr_depth": rr_depth}
    integ.update(integrator)
    film_d = {"type": "transient_hdr_film", "width": res, "height": res, "temporal_bins": bins, "start_opl": 2.0,
              "bin_width_opl": 16.0 / bins, "rfilter": {"type": "box"}}
    film_d.update(film or {})
    walls = {}
    if closed:
        grey = {"type": "diffuse", "reflectance": 0.8}
        walls = {"ceiling": {"type": "rectangle", "to_world": T().translate([0, 3.2, 1]).rotate([1, 0, 0], 90).scale([3, 4, 1]), "bsdf": grey},
                 "left": {"type": "rectangle", "to_world": T().translate([-3, 1.6, 1]).rotate([0, 1, 0], 90).scale([4, 1.6, 1]), "bsdf": grey},
                 "right": {"type": "rectangle", "to_world": T().translate([3, 1.6, 1]).rotate([0, 1, 0], -90).scale([4, 1.6, 1]), "bsdf": grey},
                 "front": {"type": "rectangle", "to_world": T().translate([0, 1.6, 5]).rotate([0, 1, 0], 180).scale([3, 1.6, 1]), "bsdf": grey}}
    return mi.load_dict({**walls,
        "type": "scene",
        "integrator": integ,
        "sensor": {"type": "perspective", "fov": 45, "to_world": T().look_at([0, 1.2, 4], [0, 0.6, 0], [0, 1, 0]), "film": film_d},
        "floor": {"type": "rectangle", "to_world": T().rotate([1, 0, 0], -90).scale(3), "bsdf": {"type": "diffuse", "reflectance": 0.6}},
        "back": {"type": "rectangle", "to_world": T().translate([0, 1.5, -2]).scale([3, 1.5, 1]),
                 "bsdf": back_bsdf or {"type": "diffuse", "reflectance": 0.4}},
        "object": obj,
        "light": {"type": "rectangle", "to_world": T().translate([0, 3, 0.5]).rotate([1, 0, 0], 90).scale(0.6),
                  "emitter": {"type": "area", "radiance": 6.0}},
        "side_light": {"type": "rectangle", "to_world": T().translate([-1.3, 1.4, 0.0]).rotate([0, 1, 0], 60).scale(0.3),
                       "emitter": {"type": "area", "radiance": 3.0}},
    })


BSDF_KINDS = ["conductor", "roughconductor_ggx", "roughconductor_beckmann_aniso", "glass", "twosided_back"]


def test_cbox_host_build_matches_the_oracle(hp):
    scene = load_cbox_polarized(res=16)
    t, s4, c = hp_render(hp, scene, seed=3, spp=16)
    assert_matches_oracle(t, s4, c, oracle_render(scene, seed=3, spp=16))
    assert np.abs(t[..., 1:3]).max() > 1e-4 * np.abs(t[..., 0]).max()


@pytest.mark.parametrize("kind", BSDF_KINDS)
def test_host_build_matches_the_oracle_per_bsdf(hp, kind):
    scene = bsdf_scene(kind)
    t, s4, c = hp_render(hp, scene, seed=1, spp=32)
    ref = oracle_render(scene, seed=1, spp=32)
    assert_matches_oracle(t, s4, c, ref)
    ot = ref[0]
    # the lobe polarizes what it reflects; circularly too where two interfaces follow each other (inside the glass cube)
    assert np.abs(ot[..., 1:3]).max() > 1e-3 * np.abs(ot[..., 0]).max()
    if kind == "glass":
        assert np.abs(ot[..., 3]).max() > 1e-4 * np.abs(ot[..., 0]).max()


def test_glass_cube_reaches_total_internal_reflection():
    """the glass scene's paths do meet total internal reflection: at max_depth 3 the cube's inside is seen at most once
    through; deeper paths add light that only TIR bounces inside the cube carry (a property of the scene the parity test needs)"""
    shallow = oracle_render(bsdf_scene("glass", max_depth=4), seed=1, spp=16)[0]
    deep = oracle_render(bsdf_scene("glass", max_depth=10), seed=1, spp=16)[0]
    assert np.abs(deep[..., 0]).sum() > np.abs(shallow[..., 0]).sum()


# the f64 building blocks of the oracle against the numpy helpers above (two f64 implementations: about 1e-12)
def test_oracle_conductor_and_dielectric_reflection_against_numpy():
    from oracle import oracle
    for eta in (complex(GOLD_ETA, GOLD_K), complex(0.2, 3.0), complex(2.0, 5.0), 1.5, 1.33):
        for ci in np.linspace(0.0, 1.0, 41)[1:]:
            assert np.abs(oracle.polar_reflection(ci, eta) - reflection_mueller64(ci, eta)).max() < 1e-12, (eta, ci)
    for ci in (-0.3, -0.5, -0.9):                     # inside glass: 1 / eta, total internal reflection below the critical angle
        assert np.abs(oracle.polar_reflection(ci, 1.5) - reflection_mueller64(-ci, 1 / 1.5)).max() < 1e-12, ci


def transmission_mueller64(ci, eta):
    """f64 specular transmission (mueller.h specular_transmission): (1 + a_s)^2 and ((1 - a_p) / eta)^2 times eta cos_t / cos_i"""
    e = eta if ci >= 0 else 1.0 / eta
    ci = abs(ci)
    ct2 = 1.0 - (1.0 - ci * ci) / (e * e)
    if ct2 <= 0:
        return np.zeros((4, 4))
    a_s, a_p = fresnel_amplitudes64(ci, e)
    k = e * math.sqrt(ct2) / ci
    ts, tp = abs(1 + a_s) ** 2, abs((1 - a_p) / e) ** 2
    a, b, c = 0.5 * k * (ts + tp), 0.5 * k * (ts - tp), k * math.sqrt(ts * tp)
    return np.array([[a, b, 0, 0], [b, a, 0, 0], [0, 0, c, 0], [0, 0, 0, c]])


def test_oracle_dielectric_transmission_against_numpy():
    from oracle import oracle
    for eta in (1.5, 1.33):
        for ci in np.concatenate([np.linspace(-1, 0, 21)[:-1], np.linspace(0, 1, 21)[1:]]):
            T = oracle.polar_transmission(ci, eta)
            assert np.abs(T - transmission_mueller64(ci, eta)).max() < 1e-12, (eta, ci)
            R = oracle.polar_reflection(ci, eta)
            assert abs(R[0, 0] + T[0, 0] - 1.0) < 1e-12 or T[0, 0] == 0       # energy: r + t = 1 outside TIR


def test_oracle_basis_rotation_against_numpy():
    from oracle import oracle
    rng = np.random.default_rng(7)
    for _ in range(50):
        fwd = rng.normal(size=3); fwd /= np.linalg.norm(fwd)
        a, b = (v - fwd * (v @ fwd) for v in rng.normal(size=(2, 3)))
        theta = math.atan2(fwd @ np.cross(a / np.linalg.norm(a), b / np.linalg.norm(b)),
                           (a / np.linalg.norm(a)) @ (b / np.linalg.norm(b)))
        assert np.abs(oracle.polar_rotate_basis(fwd, a, b) - rotator64(theta)).max() < 1e-12
        sb = oracle.polar_stokes_basis(fwd)
        assert abs(np.linalg.norm(sb) - 1) < 1e-12 and abs(sb @ fwd) < 1e-12


def test_oracle_to_world_mueller_in_the_identity_frame_is_the_basis_change():
    """in the frame (x, y, z) the local Stokes bases ARE the world ones: to_world_mueller is the identity; in a rotated frame it
    is R_out M R_in^T with the angles between the carried bases and the world's (numpy, f64)"""
    from oracle import oracle
    rng = np.random.default_rng(8)
    M = rng.normal(size=(4, 4))
    wi = rng.normal(size=3); wi /= np.linalg.norm(wi)
    wo = rng.normal(size=3); wo /= np.linalg.norm(wo)
    assert np.abs(oracle.polar_to_world_mueller(M, np.eye(3), wi, wo) - M).max() < 1e-12
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    frame = q.T                                     # rows s, t, n
    def basis(w):
        s = 1.0 if w[2] >= 0 else -1.0
        a = -1.0 / (s + w[2]); b = w[0] * w[1] * a
        return np.array([1 + s * w[0] * w[0] * a, s * b, -s * w[0]])
    def angle(f, c, t):
        return math.atan2(f @ np.cross(c, t), c @ t)
    wiw, wow = frame.T @ wi, frame.T @ wo
    Ri = rotator64(angle(wiw, frame.T @ basis(wi), basis(wiw)))
    Ro = rotator64(angle(wow, frame.T @ basis(wo), basis(wow)))
    assert np.abs(oracle.polar_to_world_mueller(M, frame.reshape(-1), wi, wo) - Ro @ M @ Ri.T).max() < 1e-12
