"""Register / scratch / LDS use of the kernels of one csrc file, from hipcc's own report: compiles the file's device
code with rn/build.py's flags plus -Rpass-analysis=kernel-resource-usage and prints one line per kernel whose name
matches a pattern. How the dgrad1x1_stream_kernel table of DESIGN.md is made (and re-made after a compiler upgrade):

python tools/kernel_resources.py rn_conv.hip dgrad1x1_stream_kernel
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "resnet.mxnet_amd")]

FIELDS = ["VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]


def main(src, pattern):
    from rn import build as b
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [b.HIPCC] + b.CXXFLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                        os.path.join(b.CSRC, src), "-o", os.path.join(tmp, "dev.o")]
        print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr[-4000:])
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")  # (without one the names stay mangled)
    text = subprocess.run([filt], input=r.stderr, capture_output=True, text=True).stdout if filt else r.stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (.*?) \[-Rpass-analysis", line)
        if m:
            cur = {} if re.search(pattern, m.group(1)) else None
            if cur is not None:
                rows.append((m.group(1), cur))
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    print("  ".join(FIELDS) + "  kernel")
    for name, f in sorted(rows):
        name = re.sub(r"\(anonymous namespace\)::|\(.*", "", name).replace("void ", "")
        ints = re.findall(r"Li(\d+)E", name)  # (a mangled name: its integer template arguments, in order)
        name += "  <%s>" % ", ".join(ints) if name.startswith("_Z") and ints else ""
        print("  ".join("%*s" % (len(k), f.get(k, "?")) for k in FIELDS) + "  " + name)
    bad = [n for n, f in rows if f.get("ScratchSize [bytes/lane]") != "0" or f.get("VGPRs Spill") != "0"]
    print("%d kernels, %d with scratch or spilled VGPRs" % (len(rows), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "."))
