#!/usr/bin/env python3
"""Per loop of a kernel listing (fused0.s, the one tools/isa.sh cuts out of the device assembly): the instruction mix of all its blocks -- the header and
the blocks the compiler annotates with "in Loop: Header=" -- VALU, SALU, branches, vector-memory instructions, and how the
running best is kept (v_min_f64 / 64-bit compares / selects); lane moves between scalar and vector registers (v_readlane / v_writelane:
scalar spills reloaded inside the loop), 32-bit integer multiplies (v_mul_lo_u32, quarter rate), vector compares (v_cmp) and LDS reads.
usage: isa_loops.py file.s"""
import re
import sys

lines = open(sys.argv[1]).read().split("\n")
loops = {}
order = []
cur = None
for l in lines:
    m = re.match(r"^(\.LBB\w+):\s*(;.*)?$", l)
    if m:
        c = m.group(2) or ""
        h = re.search(r"Header=(BB\w+)", c)
        if "Loop Header" in c:
            cur = m.group(1)[2:]
        elif h:
            cur = h.group(1)
        else:
            cur = None
        if cur and cur not in loops:
            loops[cur] = dict(valu=0, salu=0, vmem=0, br=0, brexec=0, min64=0, cmp64=0, cnd=0, lane=0, mul32=0, cmp=0, ds=0); order.append(cur)
        continue
    m2 = re.match(r"^; %bb\.\d+:\s*(;.*)?$", l)
    if m2:
        h = re.search(r"Header=(BB\w+)", m2.group(1) or "")
        cur = h.group(1) if h else None
        continue
    s = l.strip()
    if not cur or not s or s[0] in ";.":
        continue
    op = s.split()[0]; d = loops[cur]
    if op.startswith("v_"): d["valu"] += 1
    elif op.startswith("s_"):
        d["salu"] += 1
        if "branch" in op: d["br"] += 1
        if "cbranch_exec" in op: d["brexec"] += 1
    elif op.startswith(("buffer_", "global_")): d["vmem"] += 1
    if op.startswith("v_min_f64"): d["min64"] += 1
    if "_u64" in op and op.startswith("v_cmp"): d["cmp64"] += 1
    if op.startswith("v_cndmask"): d["cnd"] += 1
    if op.startswith(("v_readlane", "v_writelane")): d["lane"] += 1
    if op.startswith("v_mul_lo_u32"): d["mul32"] += 1
    if op.startswith("v_cmp"): d["cmp"] += 1
    if op.startswith("ds_"): d["ds"] += 1
for k in order:
    d = loops[k]
    print("%-10s valu %3d (v_min_f64 %d, v_cmp_*_u64 %d, v_cndmask %2d)  salu %3d  branches %2d (s_cbranch_exec* %2d)  vmem %d  v_readlane/v_writelane %2d  v_mul_lo_u32 %d  v_cmp %2d  ds %d" % (k, d["valu"], d["min64"], d["cmp64"], d["cnd"], d["salu"], d["br"], d["brexec"], d["vmem"], d["lane"], d["mul32"], d["cmp"], d["ds"]))
