#!/usr/bin/env python3
"""DEV TOOL: a kernel's ISA as a readable flow -- one instruction per line, prefixed with the innermost source line of its inline chain
that lies in the quantization search (file:line of a k_quant_*.h file), and the inlined helper's file:line when the instruction comes
from lhip_wave.h / lhip_math.h.
usage: isa_flow.py <listing.s> <kernel symbol> [file first last]   (only instructions attributed to that range of that file)"""
import re, sys
import quant_src
path, kern = sys.argv[1], sys.argv[2]
only, lo, hi = (sys.argv[3], int(sys.argv[4]), int(sys.argv[5])) if len(sys.argv) > 5 else (None, 0, 1 << 30)
inside = False; cur = ("", 0); inner = ""
def wanted(): return (only is None or cur[0] == only) and lo <= cur[1] <= hi
for l in open(path):
    if not inside:
        if l.startswith(kern + ":"): inside = True
        continue
    if l.startswith(".Lfunc_end"): break
    m = re.match(r'\s*\.loc\s+\d+\s+\d+.*?;\s*(.*)$', l)
    if m:
        chain = m.group(1)
        cur = quant_src.innermost(chain) or cur
        first = re.match(r'\S*?/?(\w+\.(?:h|cpp)):(\d+)', chain)
        inner = "" if not first or first.group(1) in quant_src.FAMILY else f"{first.group(1)[:-2]}:{first.group(2)}"
        continue
    if re.match(r'^\.L\w+:', l):
        if wanted(): print(f"      {l.strip()}")
        continue
    m = re.match(r'\s+([a-z][a-z0-9_]+.*)', l)
    if m and wanted() and not m.group(1).startswith(('.', ';')):
        print(f"{cur[0] + ':' + str(cur[1]):24s} {inner:14s} {m.group(1).split(';')[0].rstrip()}")
