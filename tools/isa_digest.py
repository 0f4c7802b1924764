#!/usr/bin/env python3
"""One line per device symbol of a built library (or object): digest of its instruction text, instruction count, name -- sorted by name.
    python tools/isa_digest.py [libquadrace.so] > a.txt ; python tools/isa_digest.py other.so > b.txt ; diff a.txt b.txt
"The device code did not move" as a command, without a GPU: equal output = the same kernels with the same instructions.  The digest is
the sha256 of the disassembly with addresses, encodings and comments stripped, so it does not depend on where a symbol was placed."""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optimal_quad_control_rl_amd import isa_lint


def digest(path):
    """{symbol: (sha256 hex, instruction count)} over every AMDGPU code object in `path`."""
    objdump = os.path.join(isa_lint.llvm_bin(), "llvm-objdump")
    out = {}
    for blob in isa_lint.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            txt = subprocess.run([objdump, "-d", "--mcpu=gfx950", f.name], check=True, capture_output=True, text=True).stdout
        cur = None
        for ln in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.*)>:", ln)
            if m:
                if m.group(1) in out:
                    raise RuntimeError("isa_digest: symbol %s occurs in two code objects of %s" % (m.group(1), path))
                cur = out[m.group(1)] = [hashlib.sha256(), 0]
            elif cur and re.match(r"^\s+(?:[sv]_|ds_|global_|buffer_|flat_|scratch_)", ln):   # (the lines isa_lint counts)
                cur[0].update(" ".join(ln.split("//")[0].split()).encode() + b"\n")
                cur[1] += 1
    return {s: (h.hexdigest(), n) for s, (h, n) in out.items()}


if __name__ == "__main__":
    for lib in sys.argv[1:] or [os.path.join(ROOT, "optimal_quad_control_rl_amd", "libquadrace.so")]:
        d = digest(lib)
        for s in sorted(d):
            print("%s %6d %s" % (d[s][0], d[s][1], s))
        print("%s: %d symbols, %d instructions" % (os.path.basename(lib), len(d), sum(n for _, n in d.values())), file=sys.stderr)
