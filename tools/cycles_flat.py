"""wave-clock sections of k_fused's flat walk on config 2 (-DMTR_PROFILE_CYCLES=2 build: MITRANSIENT_AMD_LIB=ab/libs/lib_prof_CYC2.so)
--shadow: a -DMTR_PROFILE_CYCLES=4 build — the four stages of the SHADOW walk alone, the closest-hit walk's in "everything else"; the
closest-hit walk's stages are the difference of the two runs.  --margin M: amd_shadow_hull_margin (0: the rectangle stage in every wave)"""
import sys; import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, torch
scene = bench.build_scene(512, 512, 1024)
integ = scene.integrator(); integ.collect_stats = True
if '--margin' in sys.argv: integ.shadow_hull_margin = int(sys.argv[sys.argv.index('--margin') + 1])
shadow = '--shadow' in sys.argv
for _ in range(2):
    s, t = integ.render(scene, spp=1024)
c = integ.last_counters; tm = integ.last_times
print(tm)
v = [c['splats_overflow'], c['reserved'][0], c['reserved'][1]]
sec = []
for x in v: sec += [x >> 32, x & 0xffffffff]
tot = sum(sec)
names = ['box selection (both walks)', 'shading (A + B)', 'rectangle slab tests', 'everything else (path start, bookkeeping, flush, idle)', 'rectangle tests', 'box face tests']
if shadow: names = ['shadow walk: box selection', 'shading (A + B)', 'shadow walk: rectangle slab tests (and the hull guard)', 'everything else (closest-hit walk, path start, bookkeeping, flush, idle)', 'shadow walk: rectangle tests', 'shadow walk: box face tests']
for n, x in zip(names, sec): print('%-56s %5.1f%%' % (n, 100.0 * x / tot))
