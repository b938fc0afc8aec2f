"""Are the kernels of two source trees the same device code?  (no GPU: hipcc --cuda-device-only -S)
    python scripts/same_kernels.py OTHER_CSRC [THIS_CSRC] [--files NAME.hip ...]
Compiles the named files (default: the convolution kernels, conv_igemm_dma.hip and conv3x3_rows.hip) of both directories with
build.py's flags and compares, kernel by kernel, the
text between the kernel's label and its .Lfunc_end without `;` comments and without the function number inside local labels
(.LBB27_89 / .LBB33_89): all that a changed order of instantiation changes.  Exit status 1 when a kernel is missing or differs."""
import os, re, subprocess, sys, tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-x", "hip", "--cuda-device-only", "-S"]


def kernels(csrc, name):
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(csrc, name), "-o", os.path.join(d, "k.s")], check=True)
        text = open(os.path.join(d, "k.s")).read()
    out = {}
    for sym in re.findall(r"^\s*\.name:\s+(\S+)$", text, re.M):
        body = text[text.index("\n" + sym + ":"):]
        body = body[:body.index(".Lfunc_end")]
        out[sym] = re.sub(r"(\.L[A-Za-z]+)\d+_", r"\1_", re.sub(r"\s*;.*", "", body))
    return out


argv, files = sys.argv[1:], ["conv_igemm_dma.hip", "conv3x3_rows.hip"]
if "--files" in argv:
    argv, files = argv[:argv.index("--files")], argv[argv.index("--files") + 1:]
other, this = argv[0], (argv[1:] + [os.path.join(os.path.dirname(__file__), "..", "neuralbarkcalculator_amd", "csrc")])[0]
bad = 0
for name in files:
    a, b = kernels(other, name), kernels(this, name)
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f"{name}: {len(a)} / {len(b)} kernels, {len(differ)} missing or different")
    for k in differ:
        print("  ", "differs" if k in a and k in b else "only in " + (other if k in a else this), k)
    bad += len(differ)
sys.exit(1 if bad else 0)
