#!/usr/bin/env python3
"""Diagnostic: instruction counts of every k-loop of a kernel (all basic blocks of the loop; the split kernels unroll by two,
so a loop is TWO steps) from the ISA (`hipcc -S --cuda-device-only`, the Makefile's flags): MFMAs, the other vector
instructions by kind, s_waitcnt.  Loops with fewer than 24 MFMAs are skipped.
    python tools/kloop_counts.py build/isa/gemm_split.s '<kernel name fragment>'      (profiles/r08_gemm_sign_loops.txt)"""
import re, sys, collections
path, frag = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
st = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and frag in l)
end = next(i for i in range(st, len(lines)) if lines[i].strip().startswith("s_endpgm"))
loops = collections.OrderedDict(); cur = None
for l in lines[st:end]:
    m = re.match(r"^(\.LBB\S+):\s*;\s*=>This Inner Loop Header", l.strip())
    if m: loops[m.group(1)[2:]] = []
for l in lines[st:end]:
    s = l.strip()
    m = re.match(r"^(\.LBB\S+):\s*;\s*=>This Inner Loop Header", s)
    if m: cur = m.group(1)[2:]; continue
    m2 = re.match(r"^(\.LBB\S+:|; %bb\.\d+:)\s*(;\s*in Loop: Header=(\S+))?", s)
    if m2 and (s.startswith(".LBB") or s.startswith("; %bb")):
        cur = m2.group(3) if m2.group(3) in loops else None
        continue
    if cur and s and not s.startswith((";", ".")): loops[cur].append(s.split()[0])
print(lines[st].split(":")[0][:100])
for k, ops in loops.items():
    c = collections.Counter(ops)
    mf = sum(v for o, v in c.items() if o.startswith("v_mfma"))
    if mf < 24: continue
    vec = sum(v for o, v in c.items() if o.startswith("v_") and not o.startswith("v_mfma"))
    g = lambda *p: sum(v for o, v in c.items() if o.startswith(p))
    print("  loop %-10s per 2 steps: mfma %d, other vector %d (without v_mov %d): sub %d cvt %d shift/mask %d xor %d add_f32 %d lshl_add_u64 %d cndmask %d mov %d other %d | s_waitcnt %d, all %d" % (
        k, mf, vec, vec - g("v_mov"), g("v_sub_f32"), g("v_cvt_pk_bf16"), g("v_lshlrev_b32", "v_and_b32"), g("v_xor"), g("v_add_f32"), g("v_lshl_add_u64"),
        g("v_cndmask"), g("v_mov"), vec - g("v_sub_f32", "v_cvt_pk_bf16", "v_lshlrev_b32", "v_and_b32", "v_xor", "v_add_f32", "v_lshl_add_u64", "v_cndmask", "v_mov"),
        c["s_waitcnt"], len(ops)))
