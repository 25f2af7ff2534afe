#!/usr/bin/env python3
"""DEV TOOL: instruction counts per source line of one file of the quantization search (innermost frame of the inline chain that lies in
the k_quant_*.h family): VALU, SGPR spill traffic (v_readlane / v_writelane), SALU (without s_waitcnt / s_nop), waits+nops, LDS, VMEM.
usage: isa_lines.py <g_quant listing with .loc comments> <file, e.g. k_quant_amp.h> <first line> <last line>"""
import re, collections, sys
import quant_src
lines = open(sys.argv[1]).read().split('\n')
name, a, b = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
cur = None
cnt = collections.defaultdict(collections.Counter)
for l in lines:
    m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+).*?;\s*(.*)$', l)
    if m:
        cur = quant_src.innermost(m.group(3)) or cur
        continue
    m = re.match(r'\s+([a-z][a-z0-9_]+)', l)
    if m and cur:
        op = m.group(1)
        if op.startswith(('v_readlane', 'v_writelane')): k = 'spill'
        elif op.startswith('v_'): k = 'valu'
        elif op in ('s_waitcnt', 's_nop'): k = 'wait'
        elif op.startswith('s_'): k = 'salu'
        elif op.startswith('ds_'): k = 'lds'
        elif op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')): k = 'vmem'
        else: k = 'other'
        cnt[cur][k] += 1
src = quant_src.source(name)
tot = collections.Counter()
print("file:line  valu spill salu wait lds vmem")
for ln in range(a, b + 1):
    c = cnt.get((name, ln))
    if c:
        tot.update(c)
        print(f"{name}:{ln:<5d} {c['valu']:4d} {c['spill']:4d} {c['salu']:5d} {c['wait']:4d} {c['lds']:3d} {c['vmem']:3d}  {src[ln - 1].strip()[:100]}")
print('total', dict(tot))
