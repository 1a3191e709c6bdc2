"""k_fused's wave-uniform state: the wave counters are 32 bits wide and drained into the workgroup's 64-bit sums once per work
ticket, the splat log's words and the film constants are re-read from the kernel's argument where they are used.  Renders that
draw several tickets per workgroup (guided shrinking near the end included), the single-launch band path, a crop window and the
instantiations that share the loop (NLOS, fixed-point rows, phasor rows), each against the CPU oracle: relative L2 <= 1e-5 on film
and steady image, the five counters exact.  The ticket's bound itself is host arithmetic and is tested without a GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_cornell, make_nlos, rel_l2

TOL = 1e-5      # the project's bar (BASELINE.json north_star)
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
W, H, BINS, SPP = 48, 40, 64, 96          # pixels x spp = 184320: no multiple of 256


def _gpu(scene, spp, seed=0):
    import torch
    integ = scene.integrator()
    integ.collect_stats = True
    s, t = integ.render(scene, seed=seed, spp=spp)
    torch.cuda.synchronize()
    return np.array(s), np.array(t)


def _oracle(oracle, scene, spp, seed=0):
    sd = scene.data()
    p = scene.integrator().render_params(scene.sensors()[0].film(), seed, spp)
    t4, s4, cnt = oracle.render(sd, p, use_bvh=True)
    t3, s3 = oracle.develop(sd.film, t4, s4)
    return s3, t3, cnt


def _check(scene, got, ref):
    (s_gpu, t_gpu), (s_ref, t_ref, cnt) = got, ref
    assert t_gpu.shape == t_ref.shape and s_gpu.shape == s_ref.shape
    assert np.linalg.norm(t_ref) > 0 and np.linalg.norm(s_ref) > 0
    assert rel_l2(t_gpu, t_ref) <= TOL
    assert rel_l2(s_gpu, s_ref) <= TOL
    c = scene.integrator().last_counters
    for k in COUNTERS:
        assert c[k] == cnt[k], (k, c[k], cnt[k])


@pytest.fixture(scope="module")
def cornell_ref(oracle):
    """the oracle's render of the 48 x 40 x 64 Cornell box at 96 spp, seed 4: computed once, shared, never written to"""
    scene = make_cornell(width=W, height=H, bins=BINS, amd_mode="fused")
    s, t, cnt = _oracle(oracle, scene, SPP, seed=4)
    s.setflags(write=False); t.setflags(write=False)
    return s, t, cnt


@pytest.mark.gpu
def test_counters_across_many_tickets(cornell_ref):
    """1920 pixels over a grid of far fewer workgroups than tickets: a workgroup drains its wave counters several times"""
    scene = make_cornell(width=W, height=H, bins=BINS, amd_mode="fused")
    _check(scene, _gpu(scene, SPP, seed=4), cornell_ref)


@pytest.mark.gpu
def test_counters_with_three_bands_in_one_launch(cornell_ref):
    """the same render through the single-launch band path (n_bands = 3): every band word is published, film and counters hold"""
    import torch
    scene = make_cornell(width=W, height=H, bins=BINS, amd_mode="fused")
    integ, sens = scene.integrator(), scene.sensors()[0]
    integ.collect_stats = True
    integ.direct_develop = False
    words = torch.zeros(3, dtype=torch.int32, device="cuda")
    passes = integ.prepare(scene, sens, 4, SPP, [])
    integ.accumulate(scene, sens, passes, SPP, bands=(3, 7, words.data_ptr()))
    torch.cuda.synchronize()
    assert words.cpu().tolist() == [7, 7, 7]
    s, t = (np.array(x) for x in sens.film().develop())
    _check(scene, (s, t), cornell_ref)


@pytest.mark.gpu
def test_counters_with_a_crop_window(oracle):
    """a crop window off the film's origin: the ticket's first pixel and the flushed pixel go through the crop arithmetic"""
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=W, height=H, temporal_bins=BINS, start_opl=3.5, bin_width_opl=6.0 / BINS,
                               crop_width=37, crop_height=29, crop_offset_x=7, crop_offset_y=5)
    d["integrator"].update(amd_mode="fused")
    scene = mi.load_dict(d)
    _check(scene, _gpu(scene, SPP, seed=4), _oracle(oracle, scene, SPP, seed=4))


@pytest.mark.gpu
def test_nlos_confocal_shares_the_loop(oracle):
    scene = make_nlos(sx=16, sy=16, capture="confocal", bins=256, bin_width=0.0075)
    scene.integrator().mode = 1            # MTR_MODE_FUSED: k_fused<NLOS>
    _check(scene, _gpu(scene, 32), _oracle(oracle, scene, 32))


@pytest.mark.gpu
def test_fixed_point_rows_share_the_loop(oracle):
    scene = make_cornell(width=32, height=32, bins=64, amd_mode="fused", amd_deterministic=True)
    _check(scene, _gpu(scene, 64, seed=1), _oracle(oracle, scene, 64, seed=1))


@pytest.mark.gpu
def test_phasor_rows_share_the_loop(oracle):
    import mitransient_amd.mi as mi
    from test_phasor import phasor_cornell
    mi.set_variant("llvm_ad_mono")
    try:
        scene = phasor_cornell(mi, res=32, wl_mean=2.0, wl_sigma=10.0)
        assert len(scene.sensors()[0].film().frequencies) == 3
        scene.integrator().mode = 1        # MTR_MODE_FUSED: (Re, Im) rows in LDS
        s_gpu, p_gpu = _gpu(scene, 48, seed=2)
        sd = scene.data()
        p = scene.integrator().render_params(scene.sensors()[0].film(), 2, 48)
        raw, s4, cnt = oracle.render(sd, p, use_bvh=True)
        p_ref, s_ref = oracle.develop(sd.film, raw, s4)
        assert p_gpu.shape == (32, 32, 3, 2)
        assert rel_l2(p_gpu, p_ref) <= TOL and rel_l2(s_gpu[..., 0], s_ref[..., 0]) <= TOL
        c = scene.integrator().last_counters
        for k in COUNTERS:
            assert c[k] == cnt[k], (k, c[k], cnt[k])
    finally:
        mi.set_variant("llvm_ad_rgb")


def test_ticket_bound_of_the_wave_counters():
    """host arithmetic, no GPU: a ticket's pixels x spp x 16 contributions stay below 2^32 — for the plan's own ticket at 2^20 spp
    per chunk on any grid, and for the largest ticket that can be asked for; a ticket is never cut below one pixel (beyond that the
    kernel drains a wave that has counted 2^30 bounces on the spot)"""
    from mitransient_amd import _cabi
    lib = _cabi.load_library()
    for f in (lib.mtr_test_fused_chunk, lib.mtr_test_fused_chunk_cap):
        f.restype = C.c_uint32
    lib.mtr_test_fused_chunk.argtypes = [C.c_uint32] * 3
    lib.mtr_test_fused_chunk_cap.argtypes = [C.c_uint32] * 2
    spp = 1 << 20
    for n_pixels in (1, 1920, 1 << 20, 0xffffffff):
        for grid in (1, 256, 1024):
            chunk = lib.mtr_test_fused_chunk(n_pixels, spp, grid)
            assert chunk >= 1 and chunk * spp * 16 < 1 << 32, (n_pixels, grid, chunk)
    for spp_chunk in (1, 3, 96, 1024, 1 << 20, (1 << 28) - 1):
        chunk = lib.mtr_test_fused_chunk_cap(0xffffffff, spp_chunk)          # the largest ticket
        assert chunk >= 1 and chunk * spp_chunk * 16 < 1 << 32, (spp_chunk, chunk)
        assert (chunk + 1) * spp_chunk * 16 >= 1 << 32                        # ... and no smaller than the bound asks
        assert lib.mtr_test_fused_chunk_cap(1, spp_chunk) == 1
    assert lib.mtr_test_fused_chunk_cap(7, 1 << 30) == 1                     # one pixel already over: the kernel's own drain
    # an ordinary render keeps its ticket of about 32768 samples: 512 x 512 pixels at 1024 spp on 1024 workgroups
    assert lib.mtr_test_fused_chunk(512 * 512, 1024, 1024) == 32
