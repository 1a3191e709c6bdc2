#!/usr/bin/env python3
"""tools/round_trips.py <kernel.s> — the WAIT POINTS of the persistent loop of the k_fused instantiation config 2 runs.

Reads the device assembly tools/isa_c2.sh leaves in /tmp/isa_<tag>/ (mtr_kernels-hip-amdgcn-amd-amdhsa-gfx950.s) and prints, for every
s_waitcnt of the loop that has requests outstanding: its position (instruction index from the loop's head), the requests it waits for
(scalar-load dwords, LDS operations, vector-memory operations) and the number of instructions issued between the last request and the
wait — 0 is a round trip with nothing to hide it.  Then the totals DESIGN.md section 6 quotes.

A straight-line model: the instructions are read in layout order, a wait retires what its counters say (lgkmcnt(n) leaves the n newest
LDS operations outstanding when no scalar load is in flight — scalar loads return out of order, so with one in flight only
lgkmcnt(0) retires anything; vmcnt(n) likewise, in order), and a label does not reset anything: what is outstanding at a join is what
the fall-through path left.  Only load / LDS / wait mnemonics are parsed; everything else is counted as one instruction."""
import re
import sys

KERNEL = '_ZN3mtr7k_fusedILb1ELb1ELb0ELi4ELb0ELb0ELb0ELj15EEEvNS_9FusedArgsE:'
DWORDS = {'dword': 1, 'dwordx2': 2, 'dwordx3': 3, 'dwordx4': 4, 'dwordx8': 8, 'dwordx16': 16}


def kernel_instructions(path):
    on = False
    ins, labels = [], {}
    for l in open(path):
        l = l.rstrip('\n')
        if l.startswith(KERNEL):
            on = True
            continue
        if not on:
            continue
        if 's_endpgm' in l:
            break
        m = re.match(r'^(\.LBB\d+_\d+):', l)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = l.strip()
        if not t or t[0] in ';.':
            continue
        ins.append(t.split(';')[0].strip())
    if not ins:
        sys.exit('no %s in %s' % (KERNEL, path))
    return ins, labels


def persistent_loop(ins, labels):
    loops = []
    for i, t in enumerate(ins):
        m = re.match(r'(s_cbranch\w+|s_branch)\s+(\.LBB\d+_\d+)', t)
        if m and m.group(2) in labels and labels[m.group(2)] <= i:
            loops.append((labels[m.group(2)], i))
    # the longest backward branch, as tools/isa_c2.sh takes it: the chunk loop, i.e. the persistent loop with its ticket draw and drain
    return min(loops, key=lambda ab: ab[0] - ab[1])


def wait_points(seg):
    """-> list of (position, scalar dwords, LDS ops, vector-memory ops, instructions since the last request)"""
    smem, lds, vmem = [], [], []          # outstanding: dwords per scalar load; positions of LDS / vector-memory operations
    last_req = None
    out = []
    for pos, t in enumerate(seg):
        op = t.split()[0]
        if op.startswith('s_load_') or op.startswith('s_buffer_load_'):
            smem.append(DWORDS.get(op.rsplit('_', 1)[1], 1)); last_req = pos
        elif op.startswith('ds_'):
            lds.append(pos); last_req = pos
        elif re.match(r'(global|flat|buffer|scratch)_(load|atomic)', op):
            vmem.append(pos); last_req = pos
        elif op == 's_waitcnt':
            lg = re.search(r'lgkmcnt\((\d+)\)', t)
            vm = re.search(r'vmcnt\((\d+)\)', t)
            if re.fullmatch(r's_waitcnt\s+(0|0x0)', t):
                lg_n = vm_n = 0
            else:
                lg_n = int(lg.group(1)) if lg else None
                vm_n = int(vm.group(1)) if vm else None
            w_s = w_l = w_v = 0
            if lg_n is not None:
                if smem:
                    if lg_n == 0:
                        w_s, w_l = sum(smem), len(lds); smem, lds = [], []
                elif len(lds) > lg_n:
                    w_l = len(lds) - lg_n; lds = lds[len(lds) - lg_n:] if lg_n else []
            if vm_n is not None and len(vmem) > vm_n:
                w_v = len(vmem) - vm_n; vmem = vmem[len(vmem) - vm_n:] if vm_n else []
            if w_s or w_l or w_v:
                out.append((pos, w_s, w_l, w_v, pos - last_req - 1))
    return out


def main():
    args = sys.argv[1:]
    if len(args) != 1:
        sys.exit(__doc__)
    ins, labels = kernel_instructions(args[0])
    a, b = persistent_loop(ins, labels)
    seg = ins[a:b + 1]
    pts = wait_points(seg)
    n_wait = sum(1 for t in seg if t.startswith('s_waitcnt'))
    print('persistent loop: %d instructions, %d s_load_*, %d ds_*, %d s_waitcnt, %d with requests outstanding'
          % (len(seg), sum(1 for t in seg if t.startswith('s_load_')), sum(1 for t in seg if t.startswith('ds_')), n_wait, len(pts)))
    print('%6s %8s %5s %5s %6s' % ('pos', 's_dwords', 'lds', 'vmem', 'after'))
    for pos, s, l, v, gap in pts:
        print('%6d %8d %5d %5d %6d' % (pos, s, l, v, gap))
    with_s = [p for p in pts if p[1]]
    print('waits with scalar loads among the requests: %d (%d dwords); LDS / vector memory only: %d'
          % (len(with_s), sum(p[1] for p in with_s), len(pts) - len(with_s)))
    print('waits with no instruction after the last request: %d; with at most 7: %d'
          % (sum(1 for p in pts if p[4] == 0), sum(1 for p in pts if p[4] <= 7)))


if __name__ == '__main__':
    main()
