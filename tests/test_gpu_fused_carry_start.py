"""k_fused's lean kernels restart a lane IN ITS OWN PIXEL where it takes its entry (mtr_kernels.hip: CARRY START): when the next
sample index of a lane whose path has ended lies in the pixel it has just finished (`carry`), the lane reads its record there, sets
the constants of a fresh path, advances its lane id by the difference of the two indices and goes on accumulating in p.L — no owner
test, no index arithmetic, no turn of the loop-top start section.  These are the smallest shapes at which that can go wrong: every
restart same-pixel, blocks equal to / straddling / larger than a pixel (restarts of both kinds in one iteration), a restart beside
lanes that spin on the owner, every lane restarting in every iteration, long paths, a crop window, camera_unwarp's counted ray, a
second pass (spp_begin != 0), the lane id in the splat log, bands.

Every case in the manner of test_gpu_fused_start_blocks.py: amd_mode="fused", the Cornell box, against the CPU oracle — relative
L2 <= 1e-5 on film and steady image, the five counters exact.  About 24 x 20 pixels and 32 bins unless the case says otherwise.
The steady image is what catches a wrong `carry`: a radiance deposited twice or never.

WHICH SHAPES REACH THE RESTART.  A work ticket opens with the four waves of a workgroup holding the blocks [0, 256) and the next block
drawn at index 256, and the first refill hands all 64 entries of a wave's first block to marked lanes.  So a lane takes an entry where
its path ends — the only place `carry` can come out true — only in tickets of MORE than 256 sample indices, and tickets are whole
pixels: for films this small, a pixel must hold more than 256 samples of the launch.  The shapes the issue names that stay below
that (256, 128, 64, 65, 63, 1 and 96 spp) are kept: they run the lanes that never restart beside the new code.  Every case also runs
at a shape above it.  HOW MANY PIXELS A TICKET HOLDS is the plan's (fused_plan): on a device of hundreds of compute units a film of a few
hundred pixels gets ONE-pixel tickets above 256 samples per pixel, and sample indices are ticket-local — no block straddles two pixels
there, every lane that holds an entry restarts in its pixel, nobody waits for a row.  The cases in which a restart meets a lane that
moves on to another pixel, or one that waits for its row, therefore render on ONE compute unit (`amd_reserve_cus`, clamped: at most
four workgroups), where the same film gets tickets of up to 60 pixels; they assert that.  That the shapes take the branch was checked once with two deliberately wrong libraries (profiles/
r14_carry_start.txt, section 6): without the restart's path count every case above 256 samples per pixel that reads the counters
fails on `paths` but max_depth 1 (its docstring), and with the lane id off by one the splat-log case fails on `lane`; an
experiments-build counter (tools/occ.py --mixed) finds iterations in which a lane restarts and a lane beside it moves on to another
pixel in the one-compute-unit shapes and none in the others."""
import ctypes as C

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


def _one_cu_scene(n_pixels, spp, **kw):
    """the scene rendered by one compute unit's workgroups (amd_reserve_cus is clamped so that one renders): at most four workgroups,
    so a ticket of the film holds at least fused_chunk(n_pixels, spp, 4) pixels — more than one, or the case is not what it says"""
    from mitransient_amd import _cabi
    assert _cabi.load_library().mtr_test_fused_chunk(n_pixels, spp, 4) >= 2
    return _scene(amd_reserve_cus=100000, **kw)


def _check_against_oracle(oracle, scene, spp, seed):
    s_gpu, t_gpu = gpu_render(scene, spp, seed=seed)
    got = dict(scene.integrator().last_counters)
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, spp, seed=seed)
    print("rel L2 film %.3e steady %.3e" % (rel_l2(t_gpu, t_ref), rel_l2(s_gpu, s_ref)), got)
    assert rel_l2(t_gpu, t_ref) <= TOL and rel_l2(s_gpu, s_ref) <= TOL
    for k in COUNTERS:
        assert got[k] == cnt[k], k
    return s_gpu, t_gpu


@pytest.mark.parametrize("width,spp", [(1, 256), (2, 128), (1, 1024), (2, 1024)])
def test_every_restart_is_same_pixel(oracle, width, spp):
    """1 x 1 pixel and 2 x 1 pixels at 1024 spp: tickets of one pixel, sixteen blocks inside it — from the fifth block on every
    restart is a same-pixel one but for the lanes that find their block used up.  (1 x 1 at 256 spp and 2 x 1 at 128: the four
    first blocks alone, no restart.)"""
    _check_against_oracle(oracle, _scene(width=width, height=1), spp, seed=2)


@pytest.mark.parametrize("spp", [64, 65, 63, 1, 320, 321, 319])
def test_blocks_equal_to_straddling_and_larger_than_a_pixel(oracle, spp):
    """320, 321 and 319 spp: tickets of ONE pixel (module docstring) of five blocks, the last one full, one entry over, one short:
    every lane that holds an entry restarts in its pixel, the ragged last block runs dry.  64, 65, 63: tickets of four and two
    pixels whose blocks are, or straddle, the pixels, with at most 256 indices: nobody restarts.  1: a block holds 64 pixels."""
    _check_against_oracle(oracle, _scene(), spp, seed=7)


@pytest.mark.parametrize("spp", [320, 321, 319])
def test_restarts_beside_lanes_that_move_on_to_the_next_pixel(oracle, spp):
    """one compute unit: tickets of up to 60 pixels.  320 spp: five blocks are a pixel, every fifth block of the ticket begins a new
    one; 321 and 319: the blocks straddle the pixels at a different entry each time.  Lanes that restart in their pixel and lanes
    that take an entry of the next pixel — forget their path, start at the loop top behind the owner test — end in the same
    iteration"""
    _check_against_oracle(oracle, _one_cu_scene(W * H, spp), spp, seed=7)


@pytest.mark.parametrize("spp", [96, 352])
def test_a_restart_beside_lanes_that_spin_on_the_owner(oracle, spp):
    """4096 bins: one row slot.  One compute unit, 352 spp (five and a half blocks, every other pixel boundary inside a block), tickets
    of up to 60 pixels: lanes restart in the pixel that owns the row while others of their wave hold entries of the next pixel and
    wait for the row at the loop top; the refill waits for those.  (96 spp, all compute units: one-pixel tickets of 96 indices, no
    restart and nobody waits.)"""
    scene = _one_cu_scene(W * H, spp, bins=4096) if spp == 352 else _scene(bins=4096)
    _check_against_oracle(oracle, scene, spp, seed=4)


@pytest.mark.parametrize("max_depth", [1, 2, 12])
def test_every_lane_restarts_in_every_iteration_and_long_paths(oracle, max_depth):
    """512 spp (blocks inside a pixel).  max_depth 2: lanes end at once or an iteration later, a block lasts one or two iterations
    and about half the lanes restart where they end; max_depth 12: a few lanes restart per iteration beside long paths.  max_depth 1:
    all 64 lanes end in every iteration, so every block goes whole to marked lanes through the refill and NO lane restarts where it
    ends (the library without the restart's path count passes this case): the restart's code beside a loop that never takes it"""
    _check_against_oracle(oracle, _scene(max_depth=max_depth), 512, seed=5)


def test_crop_window(oracle):
    """a crop window with an offset, 512 spp: the restarted lane keeps its film coordinates (xy) and never recomputes them; nothing
    lands outside the window.  (The film refuses a window that leaves it — "Invalid crop window specification!" — so a pixel whose
    paths deposit nothing cannot be built through the scene loader; the lanes of such a pixel would carry p.L like any other.)"""
    crop = dict(width=40, height=24, crop_width=17, crop_height=9, crop_offset_x=5, crop_offset_y=3)
    s_gpu, t_gpu = _check_against_oracle(oracle, _scene(film=crop), 512, seed=5)
    assert t_gpu.shape == (24, 40, BINS, 3)
    assert np.all(t_gpu[9:] == 0) and np.all(t_gpu[:, 17:] == 0)


def test_camera_unwarp_counts_the_start(oracle):
    """camera_unwarp: rays_closest holds one ray per path on top of the bounces, whichever place started the path; bounce 0 of a
    restarted path reads depth 0 and distance 0"""
    _check_against_oracle(oracle, _scene(camera_unwarp=True), 512, seed=6)


def test_two_passes(oracle):
    """two passes, 64 and 512 of 576 spp (spp_begin != 0 in the second, where lanes restart) over 23 x 19 pixels: a restarted
    lane's record holds the generator of sample spp_begin + (i - q spp_chunk); the passes add up to the oracle's whole render"""
    import torch
    scene = _scene(width=23, height=19)
    integ, sens = scene.integrator(), scene.sensors()[0]
    integ.collect_stats = True
    passes = integ.prepare(scene, sens, 9, 576, [])
    total = {k: 0 for k in COUNTERS}
    for rng in [(0, 64), (64, 576)]:
        integ.accumulate(scene, sens, passes, 576, spp_range=rng)
        for k in COUNTERS:
            total[k] += integ.last_counters[k]
    s, t = sens.film().develop()
    torch.cuda.synchronize()
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, 576, seed=9)
    print("rel L2 film %.3e steady %.3e" % (rel_l2(np.array(t), t_ref), rel_l2(np.array(s), s_ref)), total)
    assert rel_l2(np.array(t), t_ref) <= TOL and rel_l2(np.array(s), s_ref) <= TOL
    for k in COUNTERS:
        assert total[k] == cnt[k], k


def test_lane_id_by_difference_in_the_splat_log(oracle):
    """the second pass alone (samples 64 .. 576 of 4 x 3 pixels) with the splat log on: a restarted lane's id is the ended path's
    plus the difference of the two sample indices, and must be pixel * spp + sample — the same (lane, depth, kind, pixel, bin)
    multiset as the oracle's, the same values bit for bit"""
    import torch
    from mitransient_amd.runtime import get_context
    scene = _scene(width=4, height=3, max_depth=3)
    integ, sens = scene.integrator(), scene.sensors()[0]
    film = sens.film()
    passes = integ.prepare(scene, sens, 3, 576, [])
    ctx = get_context()
    h = scene.gpu_handle(ctx, 0)
    cap = 1 << 17
    log = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.check(ctx.lib.mtr_debug_set_splat_log(h, C.c_void_p(log.data_ptr()), cap, C.c_void_p(n.data_ptr())))
    integ.accumulate(scene, sens, passes, 576, spp_range=(64, 576))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.mtr_debug_set_splat_log(h, None, 0, None))
    n_gpu = int(n.item())
    rec = log[:n_gpu].cpu().numpy().view(np.uint32)
    params = integ.render_params(film, 3, 576, 64, 576, 0, None)
    _, _, cnt, olog = oracle.render(scene.data(), params, use_bvh=False, log_capacity=cap)
    assert 0 < n_gpu == len(olog) == cnt["splats_issued"] < cap
    g = np.zeros(n_gpu, dtype=olog.dtype)
    g["lane"], g["depth_kind"], g["pixel"], g["bin"] = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    g["r"], g["g"], g["b"], g["opl"] = (rec[:, 4].view(np.float32), rec[:, 5].view(np.float32),
                                       rec[:, 6].view(np.float32), rec[:, 7].view(np.float32))
    order = ["lane", "depth_kind"]
    g.sort(order=order)
    olog.sort(order=order)
    for k in olog.dtype.names:
        assert np.array_equal(g[k].view(np.uint32), olog[k].view(np.uint32)), k


def test_bands(oracle):
    """a banded launch (n_bands = 3) at 512 spp: every band word is published and the render agrees with the oracle"""
    import torch
    scene = _scene()
    s_ref, t_ref, s4, t4, cnt = oracle_render(oracle, scene, 512, seed=4)
    integ, sens = scene.integrator(), scene.sensors()[0]
    integ.collect_stats = True
    integ.direct_develop = False
    words = torch.zeros(3, dtype=torch.int32, device="cuda")
    passes = integ.prepare(scene, sens, 4, 512, [])
    integ.accumulate(scene, sens, passes, 512, bands=(3, 7, words.data_ptr()))
    torch.cuda.synchronize()
    assert words.cpu().tolist() == [7, 7, 7]
    s, t = (np.array(x) for x in sens.film().develop())
    assert rel_l2(t, t_ref) <= TOL and rel_l2(s, s_ref) <= TOL
    for k in COUNTERS:
        assert integ.last_counters[k] == cnt[k], k
