"""tools/loop_moves.py <dir of tools/asm_funcs.sh output> [kernel symbol substring] — the register moves of one kernel (default: the
k_fused instantiation config 2 runs): v_mov counts by source class (register, zero, other constant, scalar) over the whole function and
over the loops around its s_sleep (chunk loop, persistent loop, idle spin), every run of at least 4 consecutive moves with its line number in
mtr_kernels.s, its classes and the two register sets involved, the v_readlane / v_writelane / s_nop counts, and the resource remarks
of mtr_kernels.remarks.  It counts moves; it looks for nothing else."""
import re, sys, collections

d = sys.argv[1]
sym = sys.argv[2] if len(sys.argv) > 2 else 'k_fusedILb1ELb1ELb0ELi4ELb0ELb0ELb0ELj15E'
RUN = 4

lines = open(d + '/mtr_kernels.s').read().split('\n')
ins = []            # (line number in the file, text)
labels = {}
name = None
for n, l in enumerate(lines, 1):
    if name is None:
        m = re.match(r'^(_ZN3mtr\w+):', l)
        if m and sym in m.group(1): name = m.group(1)
        continue
    if l.startswith('.Lfunc_end'): break
    m = re.match(r'^(\.LBB\d+_\d+):', l)
    if m: labels[m.group(1)] = len(ins); continue
    t = l.split(';')[0].strip()
    if not t or t[0] == '.': continue
    ins.append((n, t))
if name is None: sys.exit('no kernel matching %s in %s/mtr_kernels.s' % (sym, d))

def regs(op):
    """v7 -> [7]; v[4:5] -> [4, 5]; anything else -> None"""
    m = re.fullmatch(r'v(\d+)', op)
    if m: return [int(m.group(1))]
    m = re.fullmatch(r'v\[(\d+):(\d+)\]', op)
    if m: return list(range(int(m.group(1)), int(m.group(2)) + 1))
    return None

def move(t):
    """(class, destination registers, source registers) of a v_mov_b32 / v_mov_b64, else None"""
    m = re.match(r'(v_mov_b32|v_mov_b64)\w*\s+([^,]+),\s*(\S+)', t)
    if not m: return None
    dst, src = regs(m.group(2).strip()), m.group(3).strip()
    if regs(src) is not None: return 'reg', dst, regs(src)
    if re.match(r'(s\d+|s\[\d+:\d+\]|vcc|exec|ttmp|m0)', src): return 'scalar', dst, []
    if src in ('0', '0x0'): return 'zero', dst, []
    return 'const', dst, []

def spans(rs):
    """[3, 8, 9, 10, 12] -> 'v3 v8-10 v12'"""
    rs = sorted(set(rs)); out = []; i = 0
    while i < len(rs):
        j = i
        while j + 1 < len(rs) and rs[j + 1] == rs[j] + 1: j += 1
        out.append('v%d' % rs[i] if i == j else 'v%d-%d' % (rs[i], rs[j])); i = j + 1
    return ' '.join(out) if out else '-'

def count(a, b):
    c = collections.Counter(); op = collections.Counter()
    for _, t in ins[a:b + 1]:
        k = t.split()[0]
        op[k] += 1
        mv = move(t)
        if mv: c[('b64 ' if k.startswith('v_mov_b64') else '') + mv[0]] += 1
    valu = sum(v for k, v in op.items() if k.startswith('v_'))
    b32 = sum(v for k, v in op.items() if k.startswith('v_mov_b32'))
    b64 = sum(v for k, v in op.items() if k.startswith('v_mov_b64'))
    return ('instructions %d  VALU %d  v_mov_b32 %d (register %d, zero %d, other constant %d, scalar %d)  v_mov_b64 %d (register %d, constant %d)  '
            'v_readlane %d  v_writelane %d  s_nop %d' % (b - a + 1, valu, b32, c['reg'], c['zero'], c['const'], c['scalar'], b64, c['b64 reg'],
            c['b64 zero'] + c['b64 const'] + c['b64 scalar'], op['v_readlane_b32'], op['v_writelane_b32'], op['s_nop']))

# the loops (header label .. last backward branch to it) that hold the s_sleep, outermost first: the chunk loop (the one the 2219 VALU
# of DESIGN.md section 8 count), the persistent loop, and whatever the compiler makes of the back edges inside it
ends = {}
for i, (_, t) in enumerate(ins):
    m = re.match(r'(s_cbranch\w+|s_branch)\s+(\.LBB\d+_\d+)', t)
    if m and m.group(2) in labels and labels[m.group(2)] <= i: ends[labels[m.group(2)]] = i
sleep = [i for i, (_, t) in enumerate(ins) if t.startswith('s_sleep')]
held = sorted((a, b) for a, b in ends.items() if sleep and a <= sleep[0] <= b)
loop = held[0] if held else None          # runs are marked against the outermost one

print('kernel  ', name)
print('function', count(0, len(ins) - 1))
for k, (a, b) in enumerate(held): print('loop %d   lines %d-%d%s  ' % (k, ins[a][0], ins[b][0], ' (chunk loop)' if k == 0 else '') + count(a, b))
if not held: print('loop     (no s_sleep: no persistent loop found)')

print('\nruns of >= %d consecutive moves (line, length, in the loop, classes, destination set <- source set)' % RUN)
i = 0; n_runs = 0; in_runs = 0
while i < len(ins):
    j = i; cl = collections.Counter(); dst = []; src = []
    while j < len(ins) and move(ins[j][1]):
        c, dd, ss = move(ins[j][1]); cl[c] += 1; dst += dd or []; src += ss; j += 1
    if j - i >= RUN:
        n_runs += 1; in_runs += j - i
        where = 'loop' if loop and loop[0] <= i <= loop[1] else '    '
        print('%6d  %3d  %s  %-40s %s <- %s' % (ins[i][0], j - i, where, ' '.join('%s %d' % kv for kv in sorted(cl.items())), spans(dst), spans(src)))
    i = max(j, i + 1)
print('%d runs, %d moves in them' % (n_runs, in_runs))

print('\nresource remarks')
try:
    on = False
    for l in open(d + '/mtr_kernels.remarks'):
        if 'Function Name:' in l: on = name in l
        elif on and 'remark:' in l: print('  ' + l.split('remark:')[1].split('[-R')[0].strip())
except OSError:
    print('  (no mtr_kernels.remarks in %s)' % d)
