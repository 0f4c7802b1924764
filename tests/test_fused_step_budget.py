"""Instruction budget of the one-wave fused E2E + residual-MLP rollout's step loop.

rollout_fast_mlp_kernel runs one wave per SIMD, and that wave's time is the number of instructions it issues: about 5.3 cycles
each, vector, packed, scalar or s_nop alike (profiles/r08_fused_issue_count.txt).  This test compiles the kernels'
translation unit to device assembly the way build.py does (same flags, same packed-f32 rewrite), finds the two step loops of every
instantiation with step_loop_asm.py and counts the instructions of the blocks that run on EVERY step; the counts of gates_ahead = 1,
the benchmark's kernel, may not exceed what the build that introduced the packed step reached.

Which copy is which: the full-grid copy (every launch whose env count is a multiple of the workgroup size, the benchmark's among
them) stores each observation block once, behind the dynamics; the general copy has a second, masked set of the same stores for
ragged waves.  So the step loop with FEWER 16-byte global stores is the full-grid one.  (In the general copy fewer instructions run
on EVERY step, because its stores sit in blocks that a ragged wave skips; that is why its count is the lower one.)

                                 every-step instructions, gates_ahead = 1
                                 full-grid copy      general copy
    before the packed step            565                531
    this build                        497                480
"""
import os
import re
import tempfile

import pytest

import step_loop_asm as A

SRC = "quadrace_kernels_mlp.hip"
CEILING_FULL_GA1 = 497      # was 565
CEILING_GENERAL_GA1 = 480   # was 531


@pytest.fixture(scope="module")
def funcs():
    try:
        from optimal_quad_control_rl_amd import build as B, isa_lint
        B._hipcc()
    except Exception:
        pytest.fail("hipcc is needed to compile the env unit to assembly (build() needs it too)")
    with tempfile.TemporaryDirectory() as d:
        text = A.compile_to_asm(SRC, os.path.join(d, SRC + ".s"))
    text, _ = isa_lint.fix_asm_text(text)   # what build.py assembles
    return A.parse(text)


def _counts(f):
    """(every-step instructions of the full-grid copy, of the general copy) of one instantiation."""
    loops = A.step_loops(f, 2)
    assert len(loops) == 2, loops
    stores = [sum(i.startswith("global_store_dwordx4") for b in f.loop_blocks(h) for i in b.insts) for h in loops]
    assert stores[0] != stores[1], stores
    full, general = (loops[0], loops[1]) if stores[0] < stores[1] else (loops[1], loops[0])
    return A.per_step_waits(f, full)[0], A.per_step_waits(f, general)[0]


def test_step_loop_instruction_budget(funcs):
    by_ga = {}
    for name, f in funcs.items():
        m = re.match(r"_ZN2qr23rollout_fast_mlp_kernelILi0ELi(\d)EEE", name)
        if m:
            by_ga[int(m.group(1))] = _counts(f)
    assert sorted(by_ga) == [0, 1, 2, 3, 4], sorted(by_ga)
    for ga, (full, general) in sorted(by_ga.items()):
        print("rollout_fast_mlp_kernel<0, %d>: every-step instructions full-grid %d, general %d" % (ga, full, general))
    full, general = by_ga[1]
    assert full <= CEILING_FULL_GA1, (full, CEILING_FULL_GA1)
    assert general <= CEILING_GENERAL_GA1, (general, CEILING_GENERAL_GA1)
