#!/usr/bin/env python3
"""Register / spill / occupancy table of the conv kernels' instantiations (hipcc -Rpass-analysis=kernel-resource-usage).
  python tools/kernel_regs.py [precision]      the generic kernel; precision: 0 f32, 1 bf16, 2 f16x2 (default: all)
  python tools/kernel_regs.py rows [csrc dir]  the row-step 3x3 kernel (conv3x3_rows.hip), of this tree or of another source
                                               directory (a copy of an older revision's csrc, two levels below its include/)
Columns: template arguments <PREC, WM, WN, MT, NT, S, STEM, VAR, BIGW> (rows: <WN, NT, SB, OR>), VGPRs, AGPRs, spilled VGPRs,
scratch bytes per lane, waves per SIMD; rows also: v_mfma and v_pk_mul_f16 instructions in the file's device assembly."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuralbarkcalculator_amd", "csrc")
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-x", "hip"]
ROWS = len(sys.argv) > 1 and sys.argv[1] == "rows"
if ROWS:
    src = os.path.join(sys.argv[2] if len(sys.argv) > 2 else CSRC, "conv3x3_rows.hip")
    name_re, head, want = r"conv3x3_rowstep_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE", "WN NT SB OR", None
    extra = []
else:
    src = os.path.join(CSRC, "conv_igemm_dma.hip")
    name_re, head = r"conv_dma_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d+)ELb(\d)E", "PREC WM WN MT NT S STEM VAR BIGW"
    want = sys.argv[1] if len(sys.argv) > 1 else None
    extra = sys.argv[2:]
cmd = HIPCC + ["-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"] + extra
out = subprocess.run(cmd, capture_output=True, text=True).stderr
cur, rows = None, []
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        t = re.search(name_re, m.group(1))
        cur = dict(args=tuple(int(v) for v in t.groups())) if t else None
        if cur:
            rows.append(cur)
        continue
    if cur is None:
        continue
    for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("sgpr", r" SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
        m = re.search(pat, line)
        if m:
            cur[key] = int(m.group(1))
if "error" in out:
    print(out[-3000:])
print(head + " | VGPR AGPR spill scratch occ")
for r in sorted(rows, key=lambda r: r["args"]):
    if want is not None and str(r["args"][0]) != want:
        continue
    print(" ".join("%*d" % (len(h), v) for h, v in zip(head.split(), r["args"])) +
          " | %4d %4d %5d %7d %3d" % (r.get("vgpr", -1), r.get("agpr", -1), r.get("spill", -1), r.get("scratch", -1), r.get("occ", -1)))
if ROWS:
    asm = subprocess.run(HIPCC + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True).stdout
    code = [line.split()[0] for line in asm.splitlines() if line.startswith("\t") and not line.startswith("\t.")]
    print("device assembly of %s: v_mfma %d, v_pk_mul_f16 %d" % (os.path.relpath(src, ROOT), sum(c.startswith("v_mfma") for c in code), code.count("v_pk_mul_f16")))
