import sys; import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# -DMTR_PROFILE_OCC build: how full are k_fused's persistent waves?  (wave iterations with a live lane, live lanes, lanes
# holding a sample whose row slot is not free yet)
# --starts, -DMTR_PROFILE_OCC=2 build: in how many of those iterations did the loop-top start section run, and in how many for a lane
# that is no same-pixel restart (`carry` false: another pixel, or served by a refill)?  With CARRY START the two are the same number.
# --mixed, -DMTR_PROFILE_OCC=3 build: in how many iterations did a lane restart where its path ended (CARRY START), and in how many of
# those did another lane of the wave, ending beside it, take an entry of another pixel?
# --hull, -DMTR_PROFILE_OCC=4 build: of the wave's shadow walks (SHADOW HULL, mtr_core.h flat_walk_device), how many entered the rectangle slab
# stage, ran at least one rectangle test pass, held a hull-risky live lane, held an E-risky live lane.  --margin M: amd_shadow_hull_margin
# --film W H BINS SPP [--one-cu]: the Cornell box of tests/test_gpu_fused_carry_start.py at that shape instead of config 2
# (--one-cu: amd_reserve_cus, tickets of many pixels on a small film)
import bench, torch
if '--film' in sys.argv:
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    w, h, bins, spp = (int(x) for x in sys.argv[sys.argv.index('--film') + 1:][:4])
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=w, height=h, temporal_bins=bins, start_opl=0.0, bin_width_opl=12.0 / bins)
    d["integrator"].update(amd_mode="fused", max_depth=6)
    if '--one-cu' in sys.argv: d["integrator"].update(amd_reserve_cus=100000)
    scene = mi.load_dict(d)
else:
    scene, spp = bench.build_scene(512,512,1024), 1024
integ = scene.integrator(); integ.collect_stats=True
if '--margin' in sys.argv: integ.shadow_hull_margin = int(sys.argv[sys.argv.index('--margin') + 1])
s,t = integ.render(scene, spp=spp)
c = integ.last_counters
it, alive, wait = c['splats_overflow'], c['reserved'][0], c['reserved'][1]
if '--hull' in sys.argv:
    walks, slabs, tests, rh, re_, iters = alive >> 32, alive & 0xffffffff, wait >> 32, wait & 0xffffffff, it >> 32, it & 0xffffffff
    print('wave iterations %d  shadow walks %d (%.3f)  entered the slab stage %d (%.3f of walks)  ran a rectangle test pass %d (%.3f)  hull-risky lane %d (%.5f)  E-risky lane %d (%.3f)'
          % (iters, walks, walks / iters, slabs, slabs / walks, tests, tests / walks, rh, rh / walks, re_, re_ / walks))
elif '--starts' in sys.argv:
    print('wave iterations %d  start section ran in %d (%.3f)  for more than same-pixel restarts in %d (%.3f)' % (it, alive, alive/it, wait, wait/it))
elif '--mixed' in sys.argv:
    print('wave iterations %d  with a restart where a path ended %d (%.3f)  with a lane beside it that moved on to another pixel %d (%.3f)' % (it, alive, alive/it, wait, wait/it))
else:
    print('wave iterations %d  alive lanes/iteration %.1f  waiting lanes/iteration %.1f  (bounces %d, ideal iterations %d)' % (it, alive/it, wait/it, c['bounces'], c['bounces']//64))
