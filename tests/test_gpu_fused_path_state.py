"""k_fused's lean kernels keep ONE copy of the path state (mtr_kernels.hip: forget_dead; mtr_core.h: SINGLE FILLS): a lane that is not
alive lets its ray, throughput, distance, depth and generator state go, and what only a shadow ray or a continuing path reads has one
definition.  These are the smallest shapes at which a lane's state crosses one of the merges that changed: lanes that never start,
owners that churn, `carry` across the paths of a lane, waves idling on the row slot, path starts with most lanes waiting, long and
short paths in one wave, passes (spp_begin != 0) with a ragged last ticket, and the Pending fills that are read only under flags.

Every case in the manner of test_gpu_fused_round_trips.py: amd_mode="fused", against the CPU oracle — relative L2 <= 1e-5 on film and
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


def test_lanes_that_never_start(oracle):
    """3 x 2 pixels x 8 spp = 48 lanes: fewer than one wave — the other lanes of the workgroup never start a path and hold a state
    nobody ever defined, from chunk entry to the wave's exit"""
    _check_against_oracle(oracle, _scene(width=3, height=2), 8, seed=3)


@pytest.mark.parametrize("spp", [1, 3])
def test_owners_churn(oracle, spp):
    """1 and 3 samples per pixel: a lane changes pixel and row slot at every path, no path is carried, rows close all the time"""
    _check_against_oracle(oracle, _scene(), spp, seed=7)


def test_carry_keeps_the_radiance(oracle):
    """2 x 2 pixels at 1024 spp: a lane runs four paths of one pixel in a row and `carry` keeps p.L across them while everything else
    of the ended path is let go — the steady image is the check"""
    _check_against_oracle(oracle, _scene(width=2, height=2), 1024, seed=2)


def test_one_row_slot(oracle):
    """4096 bins: one row slot per workgroup, so waves sit on the idle branch (all lanes waiting, none alive) while the row of the pixel
    before is flushed — the back edge on which the whole wave's state is let go"""
    _check_against_oracle(oracle, _scene(bins=4096), 96, seed=4)


@pytest.mark.parametrize("max_depth", [1, 2])
def test_paths_that_end_at_once(oracle, max_depth):
    """max_depth 1 and 2: every live lane ends in the iteration it started in or the next, so the path start runs with most lanes
    waiting, and no path ever has active_next (1) or has it once (2)"""
    _check_against_oracle(oracle, _scene(max_depth=max_depth), 96, seed=5)


def test_long_and_short_paths_in_one_wave(oracle):
    """rr_depth 1 with max_depth 12: roulette from the first bounce on — paths of 1 to 12 vertices side by side in a wave"""
    _check_against_oracle(oracle, _scene(rr_depth=1, max_depth=12), 96, seed=6)


def test_two_passes_and_a_ragged_last_ticket(oracle):
    """two passes of 48 spp (spp_begin != 0 in the second) over 23 x 19 = 437 pixels, a count no ticket size but 19 and 23 divides: the
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


def test_fills_read_only_under_flags(oracle):
    """a crop window with an offset, camera_unwarp and discard_direct_light together: the emission of a directly seen light is never
    filled in, the unwarped distance replaces bounce 0's, and what is outside the window never reaches the film"""
    crop = dict(width=40, height=24, crop_width=17, crop_height=9, crop_offset_x=5, crop_offset_y=3)
    scene = _scene(film=crop, camera_unwarp=True, discard_direct_light=True)
    s_gpu, t_gpu = _check_against_oracle(oracle, scene, 96, seed=5)
    assert t_gpu.shape == (24, 40, BINS, 3)
    assert np.all(t_gpu[9:] == 0) and np.all(t_gpu[:, 17:] == 0)
