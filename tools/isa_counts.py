#!/usr/bin/env python3
"""tools/isa_counts.py [pattern] [source root]: compile ezrt_launch.hip for gfx950 to assembly (device only, the Makefile's flags) and
print, for the kernels whose demangled name contains `pattern` (default: traceq4_kernel<7), what tools/regs.py prints -- VGPRs, SGPRs,
scratch, occupancy -- plus the static VALU / SALU instruction counts and, inside the kernel's MAIN LOOP (the longest span closed by a
backward branch), the lane-spill moves (v_readlane / v_writelane: SGPRs kept in VGPR lanes), s_nop and scratch loads / stores.
`source root` (default: this checkout) lets the same script read another checkout, e.g. the parent commit's, for a before / after."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pat = sys.argv[1] if len(sys.argv) > 1 else "traceq4_kernel<7"
root = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT
with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, "launch.s")
    cmd = "/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero " \
          "-fno-slp-vectorize -Iinclude -Iezrt_amd/csrc/hip --offload-device-only -S ezrt_amd/csrc/hip/ezrt_launch.hip -o " + out
    subprocess.run(cmd.split(), cwd=root, check=True, capture_output=True)
    txt = open(out).read()
for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^; Occupancy: \d+", txt, re.S | re.M):
    name, body = m.group(1), m.group(2)
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    if pat not in dem or ".amdhsa_kernel" not in body:
        continue
    code = body.split("s_endpgm")[0].split("\n")
    g = lambda k: (re.search(k + r":?\s+(\d+)", body) or [None, "?"])[1]
    ins = [(i, l.split()[0], l) for i, l in enumerate(code) if l.startswith("\t") and l.strip() and not l.startswith("\t.") and not l.startswith("\t;")]
    labels = {re.match(r"^(\.?\w+):", l).group(1): i for i, l in enumerate(code) if re.match(r"^\.?\w+:", l)}
    span = (0, 0)
    for i, op, l in ins:
        if op.startswith("s_cbranch") or op == "s_branch":
            t = labels.get(l.split()[-1])
            if t is not None and t < i and i - t > span[1] - span[0]:
                span = (t, i)
    loop = [(op, l) for i, op, l in ins if span[0] <= i <= span[1]]
    cnt = lambda seq, f: sum(1 for op, _ in seq if f(op))
    allops = [(op, l) for _, op, l in ins]
    print(dem)
    print("  VGPR %s SGPR %s scratch %s B/lane occupancy %s" % (g(r"; NumVgprs"), g(r"; TotalNumSgprs"), g(r"; ScratchSize"),
                                                              m.group(0).rsplit(" ", 1)[1]))
    lanemove = lambda o: o in ("v_readlane_b32", "v_writelane_b32")
    print("  static: VALU %d SALU %d, lane-spill moves %d, s_nop %d, scratch ops %d" % (
        cnt(allops, lambda o: o.startswith("v_") and "lane" not in o), cnt(allops, lambda o: o.startswith("s_") and o != "s_nop"),
        cnt(allops, lanemove), cnt(allops, lambda o: o == "s_nop"), cnt(allops, lambda o: o.startswith("scratch_"))))
    print("  main loop: %d instructions, VALU %d, lane-spill moves %d, s_nop %d, scratch ops %d" % (
        len(loop), cnt(loop, lambda o: o.startswith("v_") and "lane" not in o), cnt(loop, lanemove),
        cnt(loop, lambda o: o == "s_nop"), cnt(loop, lambda o: o.startswith("scratch_"))))
