#!/usr/bin/env python3
"""Resource table and ISA digest of every gfx950 kernel of some csrc/*.hip files, to compare two revisions of them without a GPU.
  python tools/codegen_table.py CSRC_DIR file.hip ... > table.txt        one revision
  python tools/codegen_table.py --diff OLD.txt NEW.txt                   both side by side; exit status 1 when a kernel's
                                                                         scratch, occupancy or LDS got worse
                                                                         or a kernel is new (a removed one is listed)
Per kernel (hipcc -O3 -Rpass-analysis=kernel-resource-usage --save-temps): VGPRs, AGPRs, SGPRs, scratch bytes per lane,
occupancy in waves per SIMD, LDS bytes per block, and the SHA-1 of its ISA with comments, directives and label numbers taken
out.  Equal digests mean equal machine code.  A compile is not a run."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r" AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def isa_digests(asm):
    """{symbol: sha1 of the function's instructions}"""
    out, cur, body = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"(\w+):\s*(;.*)?$", line)
        if cur is None:
            if m and not line.startswith(".L"):
                cur, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = hashlib.sha1("\n".join(body).encode()).hexdigest()[:12]
            cur = None
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith((".loc", ".file", ".cfi", ".p2align")):
            continue
        body.append(re.sub(r"\.L(BB|tmp)\d+_?", r".L\1", text))
    return out


def table(csrc, files):
    rows = []
    for f in files:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-x", "hip", "-c",
                   os.path.abspath(os.path.join(csrc, f)), "-o", "x.o", "-Rpass-analysis=kernel-resource-usage", "--save-temps"]
            err = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, check=True).stderr
            asm = [n for n in os.listdir(tmp) if n.endswith("gfx950.s")]
            digests = isa_digests(open(os.path.join(tmp, asm[0])).read())
        cur = None
        for line in err.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = dict(file=f, sym=m.group(1), isa=digests.get(m.group(1), "?"))
                rows.append(cur)
            for key, pat in FIELDS:
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    names = subprocess.run(["c++filt"], input="\n".join(r["sym"] for r in rows), capture_output=True, text=True, check=True).stdout.split("\n")
    for r, n in zip(rows, names):
        n = re.sub(r"\(anonymous namespace\)::|nbc::", "", n)
        print("%s %s vgpr=%d agpr=%d sgpr=%d scratch=%d occ=%d lds=%d isa=%s" % (
            r["file"], re.sub(r"\s+", "", re.sub(r"^void |\(.*$", "", n)), r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"], r["isa"]))


def diff(old, new):
    def read(path):
        d = {}
        for line in open(path):
            if line.startswith("#") or not line.strip():
                continue
            f, k, *kv = line.split()
            d[(f, k)] = dict(x.split("=") for x in kv)
        return d
    a, b = read(old), read(new)
    bad = 0
    print("%-18s %-44s %-26s %-26s %s" % ("file", "kernel", "parent vgpr/scr/occ/lds", "new vgpr/scr/occ/lds", "ISA"))
    for key in sorted(set(a) | set(b)):
        x, y = a.get(key), b.get(key)
        fmt = lambda r: "%s/%s/%s/%s" % (r["vgpr"], r["scratch"], r["occ"], r["lds"]) if r else "-"
        worse = x and y and (int(y["scratch"]) > int(x["scratch"]) or int(y["occ"]) < int(x["occ"]) or int(y["lds"]) > int(x["lds"]))
        bad += bool(worse) or not x                      # a kernel the new revision no longer has is not worse; one it adds has no parent row
        print("%-18s %-44s %-26s %-26s %s%s" % (key[0], key[1], fmt(x), fmt(y),
                                                "removed" if not y else "identical" if x and x["isa"] == y["isa"] else "CHANGED", "  WORSE" if worse else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    table(sys.argv[1], sys.argv[2:])
