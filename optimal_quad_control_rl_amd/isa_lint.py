"""Build-time ISA lint for libquadrace.so: no kernel of the library may contain an instruction form that MI355X executes wrongly.

Rule 1 (root cause of the "two waves per SIMD" corruption of rounds 4-5, reproducer tools/ubench/mfma_pk_hazard.hip):

    A packed-f32 VALU instruction (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) whose SECOND source takes its HIGH dword for the LOW
    half of the result (op_sel bit 1 set) loses that low-half result in lanes 48-63 when another wave of the same SIMD -- of this
    kernel, of another kernel of this process, or of another process -- issues an f16 / bf16 matrix (XDL MFMA) instruction at the
    wrong moment.  The other operand positions, the high-half selectors (op_sel_hi) and v_pk_mov_b32 are not affected.

Rule 2 (store_data_hazards below): a VALU write of the data registers of a > 8-byte vector-memory store within two wait states.

hipcc (SLP vectoriser + instruction selection) produces the form of rule 1 freely; `build.py` therefore compiles through assembly and rewrites
every occurrence into an equivalent safe form (`fix_asm_text`), and this module re-checks the FINAL code objects by disassembly, so a
library that loads is a library without the form -- whatever the compiler did.

    python -m optimal_quad_control_rl_amd.isa_lint [library.so ...]      exit status 1 and a listing if anything is found
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

_LLVM_BIN = None


def llvm_bin(hipcc=None):
    """Directory of the LLVM tools (clang, lld, clang-offload-bundler, llvm-objdump) that belong to the hipcc in use: asked of hipcc
    itself (`--print-prog-name`), so a second ROCm installation on PATH cannot give a mixed toolchain; /opt/rocm/lib/llvm/bin as the
    fallback.  Raises with a clear message when a tool is missing."""
    global _LLVM_BIN
    if _LLVM_BIN:
        return _LLVM_BIN
    import shutil
    cands = []
    hipcc = hipcc or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    try:
        out = subprocess.run([hipcc, "--print-prog-name=clang"], capture_output=True, text=True, timeout=60).stdout.strip().splitlines()
        if out and os.path.isabs(out[-1]):
            cands.append(os.path.dirname(os.path.realpath(out[-1])))
    except Exception:  # noqa: BLE001
        pass
    cands += [os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin"), "/opt/rocm/lib/llvm/bin"]
    need = ("clang", "lld", "clang-offload-bundler", "llvm-objdump")
    for d in cands:
        if all(os.path.exists(os.path.join(d, t)) for t in need):
            _LLVM_BIN = d
            return d
    raise RuntimeError("LLVM tools %s not found next to %s (looked in %s): libquadrace.so is built through device assembly and needs them" % (need, hipcc, cands))

_PK = r"v_pk_(?:fma|mul|add)_f32"
# op_sel:[a,b] or op_sel:[a,b,c] -- position 1 is the second source
_OPSEL = re.compile(r"\bop_sel:\[([01]),([01])(?:,([01]))?\]")
_OPSEL_HI = re.compile(r"\bop_sel_hi:\[([01]),([01])(?:,([01]))?\]")
_INSTR = re.compile(r"^\s*(" + _PK + r")\s+(.*)$")


def is_hazardous(line):
    """True for a packed-f32 arithmetic instruction whose src1 feeds its HIGH dword to the low result half."""
    m = _INSTR.match(line.split("//")[0].split(";")[0])
    if not m:
        return False
    sel = _OPSEL.search(m.group(2))
    return bool(sel and sel.group(2) == "1")


def _split_operands(rest):
    """'v[4:5], v[6:7], s[0:1], v[4:5] op_sel:[0,1,0] neg_lo:[...]' -> (['v[4:5]', ...], ' op_sel:[0,1,0] neg_lo:[...]')"""
    ops, depth, cur, i = [], 0, "", 0
    while i < len(rest):
        c = rest[i]
        if c == "[":
            depth += 1
        elif c == "]":
            depth -= 1
        if c == "," and depth == 0:
            ops.append(cur.strip()); cur = ""
        elif c == " " and depth == 0 and cur.strip() and re.match(r"\s*(op_sel|op_sel_hi|neg_lo|neg_hi|clamp)\b", rest[i:]):
            ops.append(cur.strip())
            return ops, rest[i:]
        else:
            cur += c
        i += 1
    ops.append(cur.strip())
    return ops, ""


def _swap01(mods, rx, nsrc, default):
    m = rx.search(mods)
    bits = [m.group(1), m.group(2)] + ([m.group(3)] if m and m.group(3) is not None else []) if m else [default] * nsrc
    bits[0], bits[1] = bits[1], bits[0]
    return m, bits


def fix_asm_line(line):
    """Rewrite a hazardous instruction into an equivalent safe one by exchanging its two commutative sources (a*b = b*a, a+b = b+a)
    together with their op_sel / op_sel_hi / neg bits: the high-dword selection moves to source 0, where the hardware handles it.
    Returns the line unchanged if it is not hazardous.  When BOTH commutative sources select the high dword for the low half
    (op_sel:[1,1,*] -- hi * hi products; the exchange cannot help) the instruction is split into its two scalar halves instead
    (split_packed_line); only if that is impossible either (the destination pair overlaps sources both ways) does it raise."""
    if not is_hazardous(line):
        return line
    body, sep, comment = line.partition(";")
    m = _INSTR.match(body)
    indent = body[: len(body) - len(body.lstrip())]
    ops, mods = _split_operands(m.group(2).rstrip())
    nsrc = len(ops) - 1
    sel = _OPSEL.search(mods)
    if sel.group(1) == "1":
        return split_packed_line(line)
    ops[1], ops[2] = ops[2], ops[1]
    out_mods = mods
    for name, rx, default in (("op_sel", _OPSEL, "0"), ("op_sel_hi", _OPSEL_HI, "1"), ("neg_lo", re.compile(r"\bneg_lo:\[([01]),([01])(?:,([01]))?\]"), "0"),
                              ("neg_hi", re.compile(r"\bneg_hi:\[([01]),([01])(?:,([01]))?\]"), "0")):
        mm, bits = _swap01(out_mods, rx, nsrc, default)
        if mm:
            out_mods = out_mods[: mm.start()] + "%s:[%s]" % (name, ",".join(bits)) + out_mods[mm.end():]
    fixed = "%s%s %s%s" % (indent, m.group(1), ", ".join(ops), out_mods)
    assert not is_hazardous(fixed), fixed
    return fixed + (" " + sep + comment if sep else "") + ("" if comment.endswith("\n") or not line.endswith("\n") else "\n")


_PAIR = re.compile(r"^([vs])\[(\d+):(\d+)\]$")


def _half(op, hi):
    """The 32-bit operand that is the low / high dword of a 64-bit packed operand (register pair; a scalar constant or a 32-bit
    literal is broadcast to both halves by the hardware)."""
    m = _PAIR.match(op)
    if not m:
        return op
    return "%s%d" % (m.group(1), int(m.group(2)) + (1 if hi else 0))


def split_packed_line(line):
    """v_pk_{mul,add,fma}_f32 D, A, B[, C] with arbitrary op_sel / op_sel_hi / neg_lo / neg_hi -> the two scalar VOP3 instructions
    that compute the same two IEEE results (D.lo = f(A[op_sel0], B[op_sel1][, C[op_sel2]]), D.hi likewise with op_sel_hi), ordered so
    that no half is overwritten before it is read.  `clamp` is carried over.  Raises when both orders would clobber a source."""
    body, sep, comment = line.partition(";")
    m = _INSTR.match(body)
    indent = body[: len(body) - len(body.lstrip())]
    ops, mods = _split_operands(m.group(2).rstrip())
    nsrc = len(ops) - 1
    def bits(rx, default):
        mm = rx.search(mods)
        return [int(x) for x in ([mm.group(1), mm.group(2)] + ([mm.group(3)] if mm.group(3) is not None else []))] if mm else [default] * nsrc
    sel, sel_hi = bits(_OPSEL, 0), bits(_OPSEL_HI, 1)
    neg_lo = bits(re.compile(r"\bneg_lo:\[([01]),([01])(?:,([01]))?\]"), 0)
    neg_hi = bits(re.compile(r"\bneg_hi:\[([01]),([01])(?:,([01]))?\]"), 0)
    for lst in (sel, sel_hi, neg_lo, neg_hi):
        lst += [lst[-1] * 0 + (1 if lst is sel_hi else 0)] * (nsrc - len(lst))
    opc = {"v_pk_mul_f32": "v_mul_f32_e64", "v_pk_add_f32": "v_add_f32_e64", "v_pk_fma_f32": "v_fma_f32"}[m.group(1)]
    clamp = " clamp" if re.search(r"\bclamp\b", mods) else ""
    def one(hi):
        srcs = [("-" if (neg_hi if hi else neg_lo)[k] else "") + _half(ops[1 + k], (sel_hi if hi else sel)[k]) for k in range(nsrc)]
        return _half(ops[0], hi), srcs
    (dlo, slo), (dhi, shi) = one(False), one(True)
    reads = lambda srcs: {x.lstrip("-") for x in srcs}   # noqa: E731
    if dlo not in reads(shi):
        order = [(dlo, slo), (dhi, shi)]
    elif dhi not in reads(slo):
        order = [(dhi, shi), (dlo, slo)]
    else:
        raise ValueError("packed-f32 instruction with op_sel:[1,1] whose destination overlaps its sources both ways: cannot be rewritten "
                         "(compile that translation unit with -fno-slp-vectorize, build.py PER_SOURCE_FLAGS, or change the source): " + line.strip())
    out = ["%s%s %s, %s%s" % (indent, opc, d, ", ".join(srcs), clamp) for d, srcs in order]
    return "\n".join(out) + (" " + sep + comment if sep else "")


def fix_asm_text(text):
    """Apply fix_asm_line to every line of a device assembly file; returns (new text, number of rewritten instructions).  An
    instruction that cannot be rewritten is reported with the kernel it belongs to and its line number."""
    out, n, sym = [], 0, "?"
    for no, ln in enumerate(text.split("\n"), 1):
        lab = re.match(r"^([A-Za-z_][\w.$]*):", ln)
        if lab and not lab.group(1).startswith(".L"):
            sym = lab.group(1)
        try:
            new = fix_asm_line(ln)
        except ValueError as ex:
            raise ValueError("%s (kernel %s, assembly line %d)" % (ex, sym, no)) from None
        n += new != ln
        out.append(new)
    return "\n".join(out), n


# ---- rule 2: a vector-memory store of more than 8 bytes followed too closely by a VALU write of its data registers ------------------
# Such a store reads its data registers after it has been issued; the gfx940 family needs two wait states before a VALU instruction
# may overwrite them.  The compiler's hazard recogniser pads the stores it schedules itself but does not look inside inline asm
# (round 5: the f32-partial path of the PPO gradient kernel stored through `asm volatile("global_store_dwordx4 ... sc1")`; once the
# EXEC-mask sequences between consecutive stores were gone, the next tile's first v_pk_mul_f32 overwrote the data of the store in
# flight).  Checked on the final disassembly, linearly (a branch target in between only makes the check stricter).
_STORE = re.compile(r"^\s*((?:global|flat|scratch)_store_dwordx[34]|buffer_store_dwordx[34]|buffer_store_format_\w*xyzw?)\s+(.*)$")
_VREG = re.compile(r"\bv(?:\[(\d+):(\d+)\]|(\d+))")
_SNOP = re.compile(r"^\s*s_nop\s+(\d+)")
_VALU = re.compile(r"^\s*(v_\w+)\s+(.*)$")
STORE_DATA_WAIT_STATES = 2


def _vregs(operand):
    m = _VREG.search(operand)
    if not m:
        return set()
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) is not None else {int(m.group(3))}


def _clean(line):
    """An instruction line of `llvm-objdump -d` or of compiler assembly without its comment / encoding."""
    return line.split("//")[0].split(";")[0].rstrip()


def store_data_hazards(lines):
    """[(store instruction, VALU instruction)] where the VALU instruction writes data registers of a > 8-byte vector-memory store
    fewer than STORE_DATA_WAIT_STATES wait states after it (every instruction in between is one wait state, `s_nop N` is N + 1)."""
    bad, pending = [], []   # pending: [store text, data registers, wait states elapsed]
    for raw in lines:
        ln = _clean(raw)
        if not ln.strip() or ln.lstrip().startswith((".", "#")) or ln.rstrip().endswith(":") or re.match(r"^[0-9a-f]+ <.*>:", ln):
            continue
        mv = _VALU.match(ln)
        if mv and pending and not mv.group(1).startswith(("v_cmp", "v_readlane", "v_readfirstlane")):
            dst = _vregs(_split_operands(mv.group(2))[0][0])
            for st, regs, waited in pending:
                if waited < STORE_DATA_WAIT_STATES and dst & regs:
                    bad.append((st.strip(), ln.strip()))
        nop = _SNOP.match(ln)
        step = int(nop.group(1)) + 1 if nop else 1
        pending = [[st, regs, waited + step] for st, regs, waited in pending if waited + step < STORE_DATA_WAIT_STATES]
        ms = _STORE.match(ln)
        if ms:
            ops, _ = _split_operands(ms.group(2))
            data = ops[0] if ms.group(1).startswith("buffer") else (ops[1] if len(ops) > 1 else "")
            pending.append([ln, _vregs(data), 0])
    return bad


def code_objects(path):
    """Every AMDGPU ELF embedded in a host object / shared library (the .hip_fatbin bundles), or the file itself if it is one."""
    data = open(path, "rb").read()
    found, pos = [], 0
    while True:
        i = data.find(b"\x7fELF", pos)
        if i < 0:
            break
        pos = i + 4
        if len(data) < i + 64 or data[i + 4] != 2:   # ELF64 only
            continue
        e_machine = struct.unpack_from("<H", data, i + 18)[0]
        if e_machine != 224:   # EM_AMDGPU
            continue
        e_shoff, = struct.unpack_from("<Q", data, i + 40)
        e_shentsize, e_shnum = struct.unpack_from("<HH", data, i + 58)
        found.append(data[i: i + e_shoff + e_shentsize * e_shnum])
    return found


def lint_library(path, stats=None):
    """[(kernel symbol, instruction text)] for every hazardous instruction in the device code of `path`.  Fails CLOSED: a
    library in which no AMDGPU code object, no kernel symbol or no instruction could be found (a compressed offload bundle, another
    bundler layout, a truncated section table) raises instead of being reported clean.  `stats` (a dict) receives the counts."""
    bad = []
    objdump = os.path.join(llvm_bin(), "llvm-objdump")
    blobs = code_objects(path)
    n_sym = n_ins = n_pk = 0
    for blob in blobs:
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            txt = subprocess.run([objdump, "-d", "--mcpu=gfx950", f.name], check=True, capture_output=True, text=True).stdout
        sym, body = "?", []
        for ln in txt.split("\n") + ["0 <end>:"]:
            m = re.match(r"^[0-9a-f]+ <(.*)>:", ln)
            if m:
                bad += [(sym, "%s  <-  %s" % (st, wr)) for st, wr in store_data_hazards(body)]
                sym, body = m.group(1), []
                n_sym += m.group(1) != "end"
            else:
                body.append(ln)
                n_ins += bool(re.match(r"^\s+(?:[sv]_|ds_|global_|buffer_|flat_|scratch_)", ln))
                n_pk += bool(_INSTR.match(ln.split("//")[0]))
                if is_hazardous(ln):
                    bad.append((sym, ln.split("//")[0].strip()))
    if stats is not None:
        stats.update(code_objects=len(blobs), symbols=n_sym, instructions=n_ins, packed_f32=n_pk)
    if not blobs or n_sym == 0 or n_ins == 0:
        raise RuntimeError("isa_lint: nothing to lint in %s (%d AMDGPU code objects, %d symbols, %d instructions): the check cannot vouch for "
                           "this library" % (path, len(blobs), n_sym, n_ins))
    return bad


def main(argv):
    libs = argv or [os.path.join(os.path.dirname(os.path.abspath(__file__)), "libquadrace.so")]
    rc = 0
    for lib in libs:
        bad = lint_library(lib)
        print("%s: %d hazardous instruction(s) (packed-f32 form / store-data overwrite)" % (lib, len(bad)))
        for sym, ins in bad[:40]:
            print("   %s: %s" % (sym, ins))
        rc |= bool(bad)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
