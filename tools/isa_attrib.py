#!/usr/bin/env python3
"""DEV TOOL: static attribution of g_quant's ISA to the source functions of the quantization search (the k_quant*.h
family).

Build the listing first (tools/isa_build.sh):
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -x hip --cuda-device-only -gline-tables-only -S lamejs_amd/csrc/lhip_api.cpp -o kg.s
usage: isa_attrib.py kg.s [kernel-symbol-substring [anything: also the top lines]]
Every instruction is attributed to the last `.loc` that pointed into one of those files (helpers inlined from lhip_wave.h /
lhip_math.h are charged to their call site).  Prints VALU / SGPR-spill (v_readlane/v_writelane) / SALU / LDS / VMEM counts
per source function (by line range) -- static counts, to be weighted with the phase call counts of phase_prof.py.
"""
import re, sys, collections
import quant_src
path = sys.argv[1]
kern = sys.argv[2] if len(sys.argv) > 2 else "g_quant"
funcs = quant_src.functions()
def func_of(loc):
    name = "?"
    for s, n in funcs[loc[0]] if loc else ():
        if s <= loc[1]: name = n
        else: break
    return name
lines = open(path).read().split("\n")
fileno = {}
for l in lines:
    m = re.match(r'\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"(?:[^"]*/)?(k_quant(?:_\w+)?\.h)"', l)      # (with or without a directory string)
    if m and m.group(2) in funcs: fileno[m.group(1)] = m.group(2)
inside = False
cur = None
stat = collections.defaultdict(lambda: collections.Counter())
perline = collections.defaultdict(lambda: collections.Counter())
for l in lines:
    if not inside:
        if re.match(r"^_Z\w*%s\w*:" % kern, l): inside = True
        continue
    if l.startswith("\t.end_amdhsa_kernel") or l.startswith(".Lfunc_end"):
        break
    m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        if m.group(1) in fileno: cur = (fileno[m.group(1)], int(m.group(2)))
        continue
    m = re.match(r"\s+([a-z][a-z0-9_]+)", l)
    if not m: continue
    op = m.group(1)
    if op.startswith("v_readlane") or op.startswith("v_writelane"): k = "spill"
    elif op.startswith("v_"): k = "valu"
    elif op.startswith("s_"): k = "salu"
    elif op.startswith("ds_"): k = "lds"
    elif op.startswith(("global_", "flat_", "scratch_", "buffer_")): k = "vmem"
    else: continue
    stat[func_of(cur)][k] += 1
    perline[cur][k] += 1
tot = collections.Counter()
print("%-28s %6s %6s %6s %5s %5s" % ("function", "valu", "spill", "salu", "lds", "vmem"))
for f, c in sorted(stat.items(), key=lambda kv: -(kv[1]["valu"] + kv[1]["spill"])):
    print("%-28s %6d %6d %6d %5d %5d" % (f, c["valu"], c["spill"], c["salu"], c["lds"], c["vmem"]))
    tot.update(c)
print("%-28s %6d %6d %6d %5d %5d" % ("TOTAL", tot["valu"], tot["spill"], tot["salu"], tot["lds"], tot["vmem"]))
if len(sys.argv) > 3:
    print("\nper line (top 60 by valu+spill):")
    for loc, c in sorted(((k, v) for k, v in perline.items() if k), key=lambda kv: -(kv[1]["valu"] + kv[1]["spill"]))[:60]:
        src = quant_src.source(loc[0])
        print("%-24s %5d %5d %5d  %s" % ("%s:%d" % loc, c["valu"], c["spill"], c["salu"], src[loc[1] - 1].strip()[:110] if 0 < loc[1] <= len(src) else ""))
