"""The one-wave fused rollout kernels do not drain their stores on every step.

Each listed kernel's env translation unit is compiled to device assembly with build.py's own flags, each step loop is found from
LLVM's loop annotations, and no block that the step loop runs on EVERY step may hold an `s_waitcnt` with a `vmcnt` field.  Waits
stay allowed where they run once per action chunk (the chunk loop around the step loop) or outside the loops.

Why: loads and stores share vmcnt, so with the previous step's observation, reward and done stores outstanding a wait for any
load is `vmcnt(0)`: the wave stalls until its whole store queue has reached memory.  Such a wait sat in the step loop of the
full-grid copy of rollout_fast_mlp_kernel / rollout_fast_kernel (for the prologue's last state load, dB), and with one wave per
SIMD nothing covered it.  See step_loop_asm.py for how blocks, loops and "every step" are read from the assembly.

rollout_fast_kernel (E2E without the MLPs) is not listed: its full-grid copy has the same per-step wait, and taking it out the same
way made that kernel 4 % slower on MI355X (see the comment in rollout_fast_body_impl).  rollout_stash_kernel and the f16-operand
rollout_policy_kernel never had one; they are listed so that they keep it that way.

rollout_policy_kernel<V, GA, true> (the reference-precision closed loop) is not listed: policy_forward_f32class reads the low-piece
weight image from global memory inside every step by design, so its step has load waits of its own.
"""
import os
import tempfile

import pytest

import step_loop_asm as A

# kernel template -> (translation unit, depth of its step loop, step loops per instantiation: full-grid copy + general copy)
KERNELS = {
    "rollout_fast_mlp_kernel": ("quadrace_kernels_mlp.hip", 2, 2),
    "rollout_stash_kernel": ("quadrace_kernels.hip", 2, 2),
    "rollout_policy_kernel": ("quadrace_kernels.hip", 1, 1),
}


def _hipcc_available():
    try:
        from optimal_quad_control_rl_amd import build as B
        B._hipcc()
        return True
    except Exception:
        return False


@pytest.fixture(scope="module")
def asm():
    if not _hipcc_available():
        pytest.fail("hipcc is needed to compile the env units to assembly (build() needs it too)")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for src in sorted({s for s, _, _ in KERNELS.values()}):
            out[src] = A.parse(A.compile_to_asm(src, os.path.join(d, src + ".s")))
    return out


def _instantiations(funcs, template):
    tag = "%d%s" % (len(template), template)   # Itanium mangling: qr::<len><name>
    names = [n for n in funcs if n.startswith("_ZN2qr" + tag + "I")]
    if template == "rollout_policy_kernel":   # the f16-operand form only (see the module docstring)
        names = [n for n in names if "ELb0EEEv" in n]
    return names


@pytest.mark.parametrize("template", sorted(KERNELS))
def test_no_vmcnt_wait_in_every_step_blocks(asm, template):
    src, depth, per_inst = KERNELS[template]
    funcs = asm[src]
    names = _instantiations(funcs, template)
    assert len(names) >= 5, (template, len(names))   # every gates_ahead (and both variants where there are two)
    bad = []
    for name in names:
        f = funcs[name]
        loops = A.step_loops(f, depth)
        assert len(loops) == per_inst, (name, loops)   # found the step loop(s), so the check below is not vacuous
        for h in loops:
            n, waits = A.per_step_waits(f, h)
            print("%s loop %s: %d every-step instructions, vmcnt waits %s" % (name, h, n, [w for _, w in waits]))
            assert n > 50, (name, h, n)   # a real step body (the smallest, INDI stash form, has ~75)
            if waits:
                bad.append((name, h, waits))
    assert not bad, bad
