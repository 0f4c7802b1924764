#!/usr/bin/env python3
"""One line per device symbol of a built library (or object): digest of its instruction text, instruction count, name -- sorted by name.
    python tools/isa_digest.py [libquadrace.so] > a.txt ; python tools/isa_digest.py other.so > b.txt ; diff a.txt b.txt
"The device code did not move" as a command, without a GPU: equal output = the same kernels with the same instructions.  The digest is
the sha256 of the disassembly with addresses, encodings and comments stripped, so it does not depend on where a symbol was placed.

--mask-kernarg: for a kernel whose PARAMETER LIST changed and whose code should not have (a variant added to a pinned kernel as a
template mode).  The digest is then blind to where an argument sits in the kernel-argument segment and to nothing else:
the offset of every scalar load from the kernel-argument pointer and the immediate of the s_add_u32 that forms the implicit-argument
pointer from it are masked; so are branch distances (an offset that stops fitting an inline constant takes a literal dword, and every
branch across it grows by one) and what the disassembler makes of the padding behind the last s_endpgm.  Each line also carries the
kernel's resources from the code object's metadata -- vgpr agpr sgpr lds scratch sgpr_spills vgpr_spills -- so that "the same code"
includes "no new scratch, no new spill".  Rename the symbols with sed before diffing."""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optimal_quad_control_rl_amd import isa_lint

RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count",
             "vgpr_spill_count")


def _mask_kernarg(lines):
    """`lines` of one kernel with the kernel-argument immediates, branch distances and trailing padding masked (see the module text)."""
    ends = [i for i, ln in enumerate(lines) if ln.startswith("s_endpgm")]
    lines = lines[:ends[-1] + 1] if ends else lines
    first = next((re.match(r"s_load_\w+ \S+ (s\[\d+:\d+\]),", ln) for ln in lines if ln.startswith("s_load_")), None)
    if not first:
        return lines
    base = first.group(1)                              # the kernel-argument pointer: the base of the kernel's first scalar load
    lo = re.match(r"s\[(\d+):", base).group(1)
    out = []
    for ln in lines:
        if re.match(r"s_load_\w+ \S+ %s, " % re.escape(base), ln):
            ln = ln[:ln.rindex(",")] + ", KERNARG"
        elif re.match(r"s_add_u32 s\d+, s%s, \w+$" % lo, ln):
            ln = ln[:ln.rindex(",")] + ", KERNARG"
        elif re.match(r"s_c?branch\w* ", ln):
            ln = ln.split()[0] + " TARGET"
        out.append(ln)
    return out


def _resources(objfile):
    """{kernel symbol: [the RESOURCES values]} from the code object's metadata note."""
    readelf = os.path.join(isa_lint.llvm_bin(), "llvm-readelf")
    txt = subprocess.run([readelf, "--notes", objfile], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n(?=\s+- \.agpr_count:)", txt):   # one list item per kernel; its first key is .agpr_count
        sym = re.search(r"^\s+\.symbol:\s+'?([^'\s]+?)(?:\.kd)?'?\s*$", block, re.M)
        if sym:
            vals = [re.search(r"^\s+(?:- )?\.%s:\s+(\d+)" % k, block, re.M) for k in RESOURCES]
            out[sym.group(1)] = [int(v.group(1)) if v else 0 for v in vals]
    return out


def digest(path, mask_kernarg=False):
    """{symbol: (sha256 hex, instruction count)} over every AMDGPU code object in `path`; with mask_kernarg a third entry, the
    kernel's RESOURCES values (None for a symbol that is no kernel)."""
    objdump = os.path.join(isa_lint.llvm_bin(), "llvm-objdump")
    out, res = {}, {}
    for blob in isa_lint.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            txt = subprocess.run([objdump, "-d", "--mcpu=gfx950", f.name], check=True, capture_output=True, text=True).stdout
            if mask_kernarg:
                res.update(_resources(f.name))
        cur = None
        for ln in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.*)>:", ln)
            if m:
                if m.group(1) in out:
                    raise RuntimeError("isa_digest: symbol %s occurs in two code objects of %s" % (m.group(1), path))
                cur = out[m.group(1)] = []
            elif cur is not None and re.match(r"^\s+(?:[sv]_|ds_|global_|buffer_|flat_|scratch_)", ln):   # (the lines isa_lint counts)
                cur.append(" ".join(ln.split("//")[0].split()))
    if mask_kernarg:
        out = {s: _mask_kernarg(lines) for s, lines in out.items()}
        return {s: (hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest(), len(lines), res.get(s)) for s, lines in out.items()}
    return {s: (hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest(), len(lines)) for s, lines in out.items()}


if __name__ == "__main__":
    mask = "--mask-kernarg" in sys.argv[1:]
    for lib in [a for a in sys.argv[1:] if a != "--mask-kernarg"] or [os.path.join(ROOT, "optimal_quad_control_rl_amd", "libquadrace.so")]:
        d = digest(lib, mask)
        for s in sorted(d):
            extra = (" " + " ".join("%d" % v for v in d[s][2]) if d[s][2] else " -") if mask else ""
            print("%s %6d%s %s" % (d[s][0], d[s][1], extra, s))
        print("%s: %d symbols, %d instructions" % (os.path.basename(lib), len(d), sum(v[1] for v in d.values())), file=sys.stderr)
