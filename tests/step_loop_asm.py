"""Control flow of hipcc device assembly, read from LLVM's own annotations: which blocks a K-step rollout kernel's step loop runs on
EVERY step, and which vector-memory waits (`s_waitcnt ... vmcnt(N)`) sit in them.

A wait there stalls the wave once per step until the counted loads AND stores have returned (loads and stores share `vmcnt`).
In a kernel that runs one wave per SIMD nothing covers that stall: the observation stores the step has just issued drain before
the dynamics go on.

Blocks start at `.LBB<f>_<n>:` labels and at `; %bb.<n>:` comments.  The comment on a label says which loop the block belongs to
(`in Loop: Header=BB<f>_<h> Depth=d`) or that it heads one (`Loop Header: Depth=d`, its parents listed as `Parent Loop ...`).
A block of loop L runs on every iteration that goes round again iff it dominates every latch of L (every block of L with an edge
back to L's header), dominance taken over L's own blocks and edges from L's header.

    python tests/step_loop_asm.py FILE.s [kernel substring ...]     prints each loop of each kernel with its waits
"""
import os
import re
import subprocess
import sys

_LABEL = re.compile(r"^\.LBB(\d+_\d+):(.*)$")
_BBCOMMENT = re.compile(r"^; %bb\.(\d+):(.*)$")
_FUNC = re.compile(r"^(_Z[A-Za-z0-9_]+):")
_IN_LOOP = re.compile(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)")
_HEADER = re.compile(r"Loop Header: Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop BB(\d+_\d+) Depth=(\d+)")
_VMCNT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(\d+\)")


class Block:
    def __init__(self, name):
        self.name = name
        self.insts = []          # instruction lines (mnemonic first)
        self.loop = None         # innermost loop (header block name) or None
        self.succ = []


class Function:
    def __init__(self, name):
        self.name = name
        self.blocks = []
        self.loop_parent = {}    # header -> parent header (None at depth 1)
        self.loop_depth = {}     # header -> depth

    def loop_blocks(self, header):
        """Blocks of loop `header`, nested loops included."""
        out = []
        for b in self.blocks:
            h = b.loop
            while h is not None and h != header:
                h = self.loop_parent.get(h)
            if h == header:
                out.append(b)
        return out

    def loops_at(self, depth):
        return [h for h, d in self.loop_depth.items() if d == depth]

    def every_iteration_blocks(self, header):
        """Blocks of loop `header` that run on every iteration that reaches a back edge (they dominate all latches)."""
        blocks = self.loop_blocks(header)
        names = {b.name for b in blocks}
        by_name = {b.name: b for b in blocks}
        pred = {n: [] for n in names}
        for b in blocks:
            for s in b.succ:
                if s in names and s != header:
                    pred[s].append(b.name)
        latches = [b.name for b in blocks if header in b.succ]
        dom = {n: set(names) for n in names}
        dom[header] = {header}
        changed = True
        while changed:
            changed = False
            for b in blocks:
                n = b.name
                if n == header:
                    continue
                ps = [dom[p] for p in pred[n]]
                new = (set.intersection(*ps) if ps else set()) | {n}
                if new != dom[n]:
                    dom[n] = new
                    changed = True
        if not latches:
            return []
        keep = set.intersection(*(dom[l] for l in latches))
        return [by_name[b.name] for b in blocks if b.name in keep]


def parse(text):
    """Device assembly text -> {mangled kernel name: Function}."""
    funcs = {}
    f = None
    cur = None
    pending_comment = None   # the block whose loop annotation may continue on the following comment-only lines

    def annotate(block, comment):
        m = _IN_LOOP.search(comment)
        if m:
            block.loop = "BB" + m.group(1)
        m = _HEADER.search(comment)
        if m:
            block.loop = block.name
            f.loop_depth[block.name] = int(m.group(1))
        for m in _PARENT.finditer(comment):
            block.parent_hint = "BB" + m.group(1)

    def start(name, comment):
        nonlocal cur
        b = Block(name)
        b.parent_hint = None
        f.blocks.append(b)
        cur = b
        annotate(b, comment)
        return b

    for line in text.splitlines():
        m = _FUNC.match(line)
        if m:
            f = Function(m.group(1))
            funcs[f.name] = f
            cur = None
            pending_comment = None
            continue
        if f is None:
            continue
        if line.startswith(".Lfunc_end"):
            f = None
            continue
        m = _LABEL.match(line) or _BBCOMMENT.match(line)
        if m:
            name = ("BB" if line.startswith(".LBB") else "%bb.") + m.group(1)
            pending_comment = start(name, m.group(2))
            continue
        s = line.strip()
        if s.startswith(";"):
            if pending_comment is not None:
                annotate(pending_comment, s)
            continue
        pending_comment = None
        if not s or s.startswith(".") or cur is None:
            continue
        cur.insts.append(s)

    for f in funcs.values():
        for b in f.blocks:
            if b.loop == b.name:
                f.loop_parent[b.name] = b.parent_hint
        names = [b.name for b in f.blocks]
        for k, b in enumerate(f.blocks):
            last = b.insts[-1].split() if b.insts else []
            op = last[0] if last else ""
            fall = names[k + 1] if k + 1 < len(names) else None
            target = last[1].lstrip(".").replace("LBB", "BB") if len(last) > 1 else None
            if op == "s_branch":
                b.succ = [target]
            elif op.startswith("s_cbranch"):
                b.succ = [target] + ([fall] if fall else [])
            elif op in ("s_endpgm", "s_setpc_b64"):
                b.succ = []
            else:
                b.succ = [fall] if fall else []
    return funcs


def step_loops(func, depth, min_insts=150):
    """The step loops of a rollout kernel: loops at `depth` with at least `min_insts` instructions (the prologue's copy loops and the
    reset paths' inner loops are a few dozen)."""
    out = []
    for h in func.loops_at(depth):
        n = sum(len(b.insts) for b in func.loop_blocks(h))
        if n >= min_insts:
            out.append(h)
    return sorted(out, key=lambda h: [b.name for b in func.blocks].index(h))


def per_step_waits(func, header):
    """(instruction count of the every-step blocks, [(block, wait instruction)] of vmcnt waits among them)."""
    blocks = func.every_iteration_blocks(header)
    waits = [(b.name, i) for b in blocks for i in b.insts if _VMCNT.match(i)]
    return sum(len(b.insts) for b in blocks), waits


def compile_to_asm(src, out):
    """One env translation unit -> device assembly, with build.py's own flags (the library's, minus -shared, plus that source's)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from optimal_quad_control_rl_amd import build as B
    flags = [f for f in B.FLAGS if f != "-shared"]
    flags = [f for f in flags if not (src in B.NO_VGPR_FORM and f in ("-mllvm", "-amdgpu-mfma-vgpr-form"))]
    cmd = [B._hipcc(), *flags, *B.PER_SOURCE_FLAGS.get(src, []), "--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", out]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as fh:
        return fh.read()


if __name__ == "__main__":
    with open(sys.argv[1]) as fh:
        fs = parse(fh.read())
    pats = sys.argv[2:]
    for name, fn in fs.items():
        if pats and not any(p in name for p in pats):
            continue
        print(name)
        for h in sorted(fn.loop_depth, key=lambda h: [b.name for b in fn.blocks].index(h)):
            n, waits = per_step_waits(fn, h)
            total = sum(len(b.insts) for b in fn.loop_blocks(h))
            print("  loop %-8s depth %d: %5d instructions, %4d on every iteration, vmcnt waits there: %s"
                  % (h, fn.loop_depth[h], total, n, [w for _, w in waits] or "none"))
