"""k_fused's lean kernels start paths from BLOCKS of 64 sample indices per wave (mtr_kernels.hip: START BLOCKS; mtr_start_blocks.h):
a wave computes the 64 path starts of its block in one full-width pass into its records of the path-start table, the lanes whose
paths end take the block's entries in lane order and read their records.  These are the smallest shapes at which that can go wrong:
fewer samples than a block, a ragged last block, blocks that span many pixels and row slots, a block that straddles two pixels with
one row slot, `carry` with blocks inside one pixel, a refill in nearly every iteration, long and short paths, passes, a crop window,
the 64-bit generator increment in the record, bands, and the context's tables in rotation.

Every case in the manner of test_gpu_fused_path_state.py: amd_mode="fused", against the CPU oracle — relative L2 <= 1e-5 on film and
steady image, the five counters exact.  About 24 x 20 pixels and 32 bins unless the case says otherwise."""
import numpy as np
import pytest

from conftest import rel_l2
from test_gpu_parity import gpu_render, oracle_render

pytestmark = pytest.mark.gpu

TOL = 1e-5   # relative L2 (BASELINE.json north_star)
COUNTERS = ("paths", "rays_closest", "rays_shadow", "splats_issued", "bounces")
W, H, BINS = 24, 20, 32


def _scene(width=W, height=H, bins=BINS, film=None, **integrator):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    from mitransient_amd import _cabi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=width, height=height, temporal_bins=bins, start_opl=0.0, bin_width_opl=12.0 / bins)
    d["sensor"]["film"].update(film or {})
    d["integrator"].update(amd_mode="fused", max_depth=6)
    d["integrator"].update(integrator)
    scene = mi.load_dict(d)
    assert scene.gpu_traits() & _cabi.MTR_TRAIT_FLAT_TOP          # the flat walk: the lean kernels
    return scene


def _check_against_oracle(oracle, scene, spp, seed):
    s_gpu, t_gpu = gpu_render(scene, spp, seed=seed)
    got = dict(scene.integrator().last_counters)
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, spp, seed=seed)
    print("rel L2 film %.3e steady %.3e" % (rel_l2(t_gpu, t_ref), rel_l2(s_gpu, s_ref)), got)
    assert rel_l2(t_gpu, t_ref) <= TOL and rel_l2(s_gpu, s_ref) <= TOL
    for k in COUNTERS:
        assert got[k] == cnt[k], k
    return s_gpu, t_gpu


def test_fewer_samples_than_one_block(oracle):
    """3 x 2 pixels x 8 spp = 48 samples: wave 0's first block is ragged, the blocks of waves 1 to 3 lie beyond the ticket's end"""
    _check_against_oracle(oracle, _scene(width=3, height=2), 8, seed=3)


def test_ragged_last_block(oracle):
    """23 x 19 pixels x 3 spp = 1311 samples, 1311 % 64 = 31 (and no ticket of whole pixels is a multiple of 64 either): the last
    block of every ticket has entries that do not exist"""
    _check_against_oracle(oracle, _scene(width=23, height=19), 3, seed=8)


@pytest.mark.parametrize("spp", [1, 3])
def test_a_block_spans_many_pixels(oracle, spp):
    """1 and 3 samples per pixel: one block holds 64 or 21 pixels, more than there are row slots"""
    _check_against_oracle(oracle, _scene(), spp, seed=7)


def test_a_block_straddles_two_pixels_with_one_row_slot(oracle):
    """4096 bins: one row slot; 96 spp is no multiple of 64, so every second block holds entries of two pixels and lanes take entries
    of a pixel that owns no row yet — the refill waits for them, the only spin is the owner's"""
    _check_against_oracle(oracle, _scene(bins=4096), 96, seed=4)


def test_carry_with_blocks_inside_one_pixel(oracle):
    """2 x 2 pixels at 1024 spp: sixteen blocks per pixel, a lane's next entry is of the same pixel and `carry` keeps p.L, except
    for the lanes that find the block used up, which deposit at once — the steady image is the check"""
    _check_against_oracle(oracle, _scene(width=2, height=2), 1024, seed=2)


@pytest.mark.parametrize("max_depth", [1, 2])
def test_a_refill_in_nearly_every_iteration(oracle, max_depth):
    """max_depth 1 and 2: every live lane ends at once or an iteration later, a block lasts one or two iterations and most lanes
    are served after the refill"""
    _check_against_oracle(oracle, _scene(max_depth=max_depth), 96, seed=5)


def test_long_and_short_paths_side_by_side(oracle):
    """rr_depth 1 with max_depth 12: a few lanes end per iteration, a block is handed out over many iterations"""
    _check_against_oracle(oracle, _scene(rr_depth=1, max_depth=12), 96, seed=6)


def test_two_passes(oracle):
    """two passes of 48 spp (spp_begin != 0 in the second) over 23 x 19 pixels: the records' sample numbers start at spp_begin; the
    passes add up to the oracle's whole render, film and counters"""
    import torch
    scene = _scene(width=23, height=19)
    integ, sens = scene.integrator(), scene.sensors()[0]
    integ.collect_stats = True
    passes = integ.prepare(scene, sens, 9, 96, [])
    total = {k: 0 for k in COUNTERS}
    for rng in [(0, 48), (48, 96)]:
        integ.accumulate(scene, sens, passes, 96, spp_range=rng)
        for k in COUNTERS:
            total[k] += integ.last_counters[k]
    s, t = sens.film().develop()
    torch.cuda.synchronize()
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, 96, seed=9)
    print("rel L2 film %.3e steady %.3e" % (rel_l2(np.array(t), t_ref), rel_l2(np.array(s), s_ref)), total)
    assert rel_l2(np.array(t), t_ref) <= TOL and rel_l2(np.array(s), s_ref) <= TOL
    for k in COUNTERS:
        assert total[k] == cnt[k], k


def test_crop_window_and_camera_unwarp(oracle):
    """a crop window with an offset: a record's ray comes from the film coordinates of the CROP pixel, which the lane rebuilds from
    its index; camera_unwarp reads the lane's first closest hit"""
    crop = dict(width=40, height=24, crop_width=17, crop_height=9, crop_offset_x=5, crop_offset_y=3)
    scene = _scene(film=crop, camera_unwarp=True)
    s_gpu, t_gpu = _check_against_oracle(oracle, scene, 96, seed=5)
    assert t_gpu.shape == (24, 40, BINS, 3)
    assert np.all(t_gpu[9:] == 0) and np.all(t_gpu[:, 17:] == 0)


@pytest.mark.parametrize("seeding", ["tea+lane", "tea64"])
def test_generator_increment_in_the_record(oracle, seeding):
    """MTR_FLAG_PCG_INITSEQ_PLUS_LANE and MTR_FLAG_PCG_TEA64: the record carries all 64 bits of the PCG32 increment"""
    scene = _scene()
    integ = scene.integrator()
    integ.pcg_initseq_plus_lane = seeding == "tea+lane"
    integ.pcg_tea64 = seeding == "tea64"
    _check_against_oracle(oracle, scene, 24, seed=1)


def test_bands_and_tables_in_rotation(oracle):
    """a banded launch (n_bands = 3), then two plain renders on the same context: three launches, three tables of the rotation;
    every band word is published and each render agrees with the oracle"""
    import torch
    scene = _scene()
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, 24, seed=4)
    integ, sens = scene.integrator(), scene.sensors()[0]
    integ.collect_stats = True
    integ.direct_develop = False
    words = torch.zeros(3, dtype=torch.int32, device="cuda")
    passes = integ.prepare(scene, sens, 4, 24, [])
    integ.accumulate(scene, sens, passes, 24, bands=(3, 7, words.data_ptr()))
    torch.cuda.synchronize()
    assert words.cpu().tolist() == [7, 7, 7]
    s, t = (np.array(x) for x in sens.film().develop())
    assert rel_l2(t, t_ref) <= TOL and rel_l2(s, s_ref) <= TOL
    for k in COUNTERS:
        assert integ.last_counters[k] == cnt[k], k
    scene2 = _scene()
    for _ in range(2):
        s_gpu, t_gpu = gpu_render(scene2, 24, seed=4)
        assert rel_l2(t_gpu, t_ref) <= TOL and rel_l2(s_gpu, s_ref) <= TOL
        for k in COUNTERS:
            assert scene2.integrator().last_counters[k] == cnt[k], k
