"""tools/cycles_rt.py — the price of ONE round trip inside the running config-2 kernel (4 waves per SIMD): needs the experiments
library built with EXTRA=-DMTR_PROFILE_CYCLES=3 (MITRANSIENT_AMD_LIB=.../libmitransient_amd_exp.so).  Wave clocks (s_memtime) per
bracket in k_fused's `refresh`.  Every bracket is: clock read, awaited; its content, awaited; the next clock read.  The contents: nothing,
a kernarg_copy<Film, true> (14 dwords, three s_load_*), one ds_read_b64 of the staged scene (through an LDS-address-space pointer: check
the assembly for ds_read_b64, a generic pointer gives a flat_load).  A content's price is its bracket minus the empty one."""
import sys; import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, torch
scene = bench.build_scene(512, 512, 1024)
integ = scene.integrator(); integ.collect_stats = True
for _ in range(2):
    s, t = integ.render(scene, spp=1024)
c = integ.last_counters
print(integ.last_times)
scal, lds, packed = c['splats_overflow'], c['reserved'][0], c['reserved'][1]
n, empty = packed >> 32, (packed & 0xffffffff) << 6          # (the kernel keeps the empty brackets' clocks in units of 64, per wave)
print('brackets %d' % n)
print('empty bracket (clock read, awaited, clock read)                          %.1f clocks' % (empty / n))
print('scalar bracket (+ 14 dwords of the kernarg segment, awaited at once)     %.1f clocks: the loads %.1f' % (scal / n, (scal - empty) / n))
print('LDS bracket (+ one ds_read_b64, awaited at once)                         %.1f clocks: the read  %.1f' % (lds / n, (lds - empty) / n))
