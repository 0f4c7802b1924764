"""CPU-side checks of the dynamics-grid feature (no GPU needed): the qr_dynamics_* / qr_evaluate_policy_dynamics_grid entry points against
include/quadrace.h and optimal_quad_control_rl_amd/_lib.py in the manner of tests/abi_table.py, what they refuse without a device, the
nominal table against SURVEY Appendix A (tests/golden/dynamics_nominal.json), the physical-to-table folding of dynamics.py against the
nominal table and against tests/dynamics_spec.py, and the float64 restatement tests/dynamics_spec.py (which
tests/test_gpu_dynamics_grid.py holds the kernel against) against the C oracle's one step at nominal coefficients.

Measured here (256 injected states per variant, dynamics_spec.injected_states, seed 20; parity.rel_err of the new world state, float32 C
oracle against the float64 restatement): E2E max 5.272e-07 (in p: its derivative holds the difference of four squared rotor speeds of 1e8),
INDI max 1.198e-07.  The project's teacher-forced one-step bound is 1e-6; the E2E maximum exceeds a quarter of it, so the GPU
test uses four times the measured value there, 2.112e-6, and 1e-6 for INDI (dynamics_spec.ORACLE_ERR / tolerance).
from_physical(reference values) against nominal(): 0 ulp in every entry of both variants, so equality is asserted."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import abi_decl
import dynamics_spec as D
import parity
import test_abi_host
from abi_table import f32p, i32, i32p, row, vp, vpp  # noqa: F401
from optimal_quad_control_rl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "quadrace_eval_dynamics.hip"
CONTRACT = ("typedef struct qr_dynamics_bank qr_dynamics_bank",
            ["CONTRACT", "bit for bit", "Refused before anything is launched", "scalar registers", "NOT modelled", "residual", "observation",
             "GROUP-LOCAL RESET STREAM", "R:81, 124", "R:74, 144", "R:89, 131, 146", "I:69-70, 94", "I:58, 63-64, 101", "22 entries", "12 entries", "128 bytes"])
_OUT22 = (C.c_float * 22)()
ROWS = [
    row("qr_dynamics_count", ["variant"], types=["int32_t"], bound=[i32], optional=True, in_version_comment="qr_dynamics_*", source=SRC,
        default_flags=True, vgpr_form=True, defines={"QR_ABI_VERSION": 3}, contract=CONTRACT,
        patterns=[r"typedef\s+struct\s+qr_dynamics_bank\s+qr_dynamics_bank\s*;"], null_call=((7,), _lib.QR_E_INVALID, b"qr_dynamics_count")),
    row("qr_dynamics_nominal", ["variant", "out", "count"], types=["int32_t", "float *", "int32_t"], bound=[i32, f32p, i32], optional=True,
        null_call=((0, None, 22), _lib.QR_E_INVALID, b"qr_dynamics_nominal")),
    row("qr_dynamics_bank_create", ["variant", "device", "capacity", "out"], types=["int32_t", "int32_t", "int32_t", "qr_dynamics_bank * *"],
        bound=[i32, i32, i32, vpp], optional=True, same_as=[((0, None), "qr_condition_bank_create", (0, None))],
        null_call=((0, 0, 1, None), _lib.QR_E_INVALID, b"qr_dynamics_bank_create")),
    row("qr_dynamics_bank_destroy", ["bank"], types=["qr_dynamics_bank *"], bound=[vp], optional=True),
    row("qr_dynamics_bank_capacity", ["bank"], types=["const qr_dynamics_bank *"], bound=[vp], optional=True,
        null_call=((None,), _lib.QR_E_INVALID, b"qr_dynamics_bank_capacity")),
    row("qr_dynamics_bank_set", ["bank", "slot", "coeffs", "count"], types=["qr_dynamics_bank *", "int32_t", "const float *", "int32_t"],
        bound=[vp, i32, f32p, i32], optional=True, null_call=((None, 0, None, 22), _lib.QR_E_INVALID, b"qr_dynamics_bank_set")),
    row("qr_dynamics_bank_read", ["bank", "slot", "out", "count"], types=["const qr_dynamics_bank *", "int32_t", "float *", "int32_t"],
        bound=[vp, i32, f32p, i32], optional=True, null_call=((None, 0, _OUT22, 22), _lib.QR_E_INVALID, b"qr_dynamics_bank_read")),
    row("qr_evaluate_policy_dynamics_grid",
        ["env", "policies", "conditions", "dynamics", "num_groups", "envs_per_group", "policy_of_group", "condition_of_group", "dynamics_of_group",
         "num_steps", "flags", "rec_dev", "recf_dev", "stream"],
        types={1: "qr_policy_bank *", 2: "qr_condition_bank *", 3: "qr_dynamics_bank *", 6: "const int32_t *", 7: "const int32_t *", 8: "const int32_t *"},
        bound={3: vp, 6: i32p, 7: i32p, 8: i32p, 9: i32, 10: i32}, optional=True, in_version_comment="qr_evaluate_policy_dynamics_grid",
        in_exports="qr_*", same_as=[((0, 3), "qr_evaluate_policy_grid", (0, 3)), ((4, 8), "qr_evaluate_policy_grid", (3, 7)),
                                    ((9, None), "qr_evaluate_policy_grid", (7, None))],
        null_call=((None,) * 4 + (1, 256) + (None,) * 3 + (1, 0) + (None,) * 3, _lib.QR_E_INVALID, None)),
]


# ---- header <-> _lib ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ROWS, ids=lambda r: r["name"])
def test_dynamics_entry_points_are_pinned(r):
    test_abi_host.test_pinned_entry_points(r)
    assert r["name"] in _lib.SIGNATURES and r["name"] in _lib.OPTIONAL_SYMBOLS


def test_every_declared_dynamics_function_has_a_row():
    code = abi_decl.header()[1]
    declared = sorted(f[0] for f in abi_decl.functions(code, "qr_dynamics_")) + ["qr_evaluate_policy_dynamics_grid"]
    assert abi_decl.declaration(code, "qr_evaluate_policy_dynamics_grid")
    assert declared == sorted(r["name"] for r in ROWS) and len(declared) == 8


@pytest.mark.parametrize("r", [r for r in ROWS if "null_call" in r], ids=lambda r: r["name"])
def test_null_calls_are_refused(r):
    test_abi_host.test_null_handles_are_refused_without_a_device(r)


def test_count_and_nominal_check_their_arguments():
    L = _lib.load()
    assert L.qr_dynamics_count(0) == 22 and L.qr_dynamics_count(1) == 12
    out = (C.c_float * 32)(*([7.0] * 32))
    for variant, count in ((0, 12), (0, 21), (0, 23), (1, 22), (1, 0), (2, 22), (-1, 12)):
        assert L.qr_dynamics_nominal(variant, out, count) == _lib.QR_E_INVALID, (variant, count)
        assert b"qr_dynamics_nominal" in L.qr_last_error() and all(x == 7.0 for x in out)
    assert L.qr_dynamics_nominal(1, out, 12) == _lib.QR_OK and all(x == 7.0 for x in out[12:])     # writes `count` values and no more
    assert L.qr_dynamics_bank_destroy(None) == _lib.QR_OK


def test_bank_create_checks_its_arguments_before_it_asks_for_a_device():
    L = _lib.load()
    h = C.c_void_p()
    for variant, capacity in ((2, 1), (-1, 1), (0, 0), (1, -4)):
        assert L.qr_dynamics_bank_create(variant, 0, capacity, C.byref(h)) == _lib.QR_E_INVALID and not h.value
        assert b"qr_dynamics_bank_create" in L.qr_last_error()


def test_bank_create_without_a_device_is_no_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.load()
    h = C.c_void_p()
    assert L.qr_dynamics_bank_create(0, 0, 4, C.byref(h)) == _lib.QR_E_NO_DEVICE
    assert b"no HIP device" in L.qr_last_error() and not h.value


# ---- the nominal table ---------------------------------------------------------------------------------------------------------------------
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "dynamics_nominal.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("variant,key", [(0, "e2e"), (1, "indi")])
def test_nominal_is_exactly_the_float32_values_of_appendix_a(variant, key):
    from optimal_quad_control_rl_amd.dynamics import ENTRIES, DynamicsParams

    want = np.asarray(_golden()[key], np.float64).astype(np.float32)
    got = DynamicsParams.nominal(variant)
    assert got.coeffs.dtype == np.float32 and got.coeffs.shape == want.shape == (D.COUNT[variant],) == (len(ENTRIES[variant]),)
    assert np.array_equal(got.coeffs.view(np.int32), want.view(np.int32))
    assert not got.coeffs.flags.writeable and got.variant == variant


def test_importing_dynamics_needs_no_torch():
    import subprocess

    code = "import sys; import optimal_quad_control_rl_amd.dynamics as d; d.DynamicsParams.nominal(0); assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ---- the folding -----------------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("variant", [0, 1])
def test_from_physical_reference_values_is_the_nominal_table(variant):
    from optimal_quad_control_rl_amd import dynamics as M

    nominal = M.DynamicsParams.nominal(variant)
    folded = M.DynamicsParams.from_physical(variant, **M.PHYSICAL[variant])
    spec = (D.fold_e2e if variant == 0 else D.fold_indi)(**M.PHYSICAL[variant]).astype(np.float32)
    print("variant", variant, "ulps from_physical vs nominal", _ulps(folded.coeffs, nominal.coeffs).tolist(), "spec vs nominal", _ulps(spec, nominal.coeffs).tolist())
    assert np.array_equal(folded.coeffs.view(np.int32), nominal.coeffs.view(np.int32))      # measured: 0 ulp everywhere
    assert np.array_equal(spec.view(np.int32), nominal.coeffs.view(np.int32))


def test_from_physical_refuses_what_the_table_cannot_hold():
    from optimal_quad_control_rl_amd import dynamics as M

    for variant, extra in ((1, dict(T_min=1.0)), (1, dict(p_min=-2.0)), (0, dict(k_zz=1.0))):
        with pytest.raises(ValueError):
            M.DynamicsParams.from_physical(variant, **{**M.PHYSICAL[variant], **extra})
    for variant in (0, 1):
        short = dict(M.PHYSICAL[variant])
        short.pop("g")
        with pytest.raises(ValueError):
            M.DynamicsParams.from_physical(variant, **short)
    with pytest.raises(ValueError):
        M.DynamicsParams.from_physical(0, **{**M.PHYSICAL[0], "Ixx": 0.0})       # 1 / 0: not finite
    with pytest.raises(ValueError):
        M.DynamicsParams(0, np.zeros(12))
    with pytest.raises(ValueError):
        M.DynamicsParams(3, np.zeros(12))


@pytest.mark.parametrize("variant", [0, 1])
def test_physical_sweep_moves_exactly_the_entries_the_folding_says(variant):
    from optimal_quad_control_rl_amd import dynamics as M

    assert sorted(D.MOVES[variant]) == sorted(M.PHYSICAL[variant])
    for name, moved in D.MOVES[variant].items():
        base, up, down = M.physical_sweep(variant, name, [1.0, 1.15, 0.7])
        assert (base.name, up.name) == (name + "*1", name + "*1.15") and base.variant == variant
        assert np.array_equal(base.coeffs, M.DynamicsParams.nominal(variant).coeffs)
        for other in (up, down):
            assert np.nonzero(other.coeffs != base.coeffs)[0].tolist() == moved, (name, other.name)
        # and by the factor the folding says, against the float64 restatement
        phys = dict(M.PHYSICAL[variant])
        phys[name] *= 1.15
        want = (D.fold_e2e if variant == 0 else D.fold_indi)(**phys).astype(np.float32)
        assert np.array_equal(up.coeffs.view(np.int32), want.view(np.int32)), name
    assert D.MOVES[0]["Izz"] == [9, 13, 16, 17, 18, 19, 20] and D.MOVES[0]["tau"] == [19, 20, 21]     # why the sweep is physical
    with pytest.raises(ValueError):
        M.physical_sweep(variant, "mass", [1.0])


def test_scaled_works_by_entry_name_and_refuses_unknown_names():
    from optimal_quad_control_rl_amd import dynamics as M

    n = M.DynamicsParams.nominal(0)
    s = n.scaled(neg_k_w=1.15, motor_lag=0.5)
    changed = np.nonzero(s.coeffs != n.coeffs)[0].tolist()
    assert changed == [M.E2E_ENTRIES.index("neg_k_w"), M.E2E_ENTRIES.index("motor_lag")] == [4, 21]
    assert s.coeffs[4] == np.float32(n.coeffs[4]) * np.float32(1.15) and s.coeffs[21] == np.float32(n.coeffs[21]) * np.float32(0.5)
    assert np.array_equal(n.scaled().coeffs, n.coeffs)
    for bad in (dict(k_w=1.1), dict(thrust_gain=1.1), dict(Izz=1.1)):
        with pytest.raises(ValueError):
            n.scaled(**bad)
    assert M.DynamicsParams.nominal(1).scaled(thrust_gain=2.0).coeffs[2] == -16.0
    with pytest.raises(Exception):
        n.coeffs[0] = 1.0            # frozen


def test_plan_dynamics_batches():
    from optimal_quad_control_rl_amd.evaluation import plan_dynamics_batches

    plan = plan_dynamics_batches(2, 1, 3, 4)
    assert plan == [([(0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 0, 0)], 4), ([(1, 0, 1), (1, 0, 2), (1, 0, 2), (1, 0, 2)], 2)]
    cells = [c for batch, kept in plan_dynamics_batches(2, 3, 5, 7) for c in batch[:kept]]
    assert cells == [(p, c, d) for p in range(2) for c in range(3) for d in range(5)]
    for bad in ((0, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4), (1, 1, 1, 0)):
        with pytest.raises(ValueError):
            plan_dynamics_batches(*bad)


def test_reality_gap_sweep_arguments_and_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reality_gap_sweep as T

    assert T.parse_factors("0.7, 1,1.3") == [0.7, 1.0, 1.3]
    for bad in ("", "0", "-1,1", "1,1", "a", "inf"):
        with pytest.raises(SystemExit):
            T.parse_factors(bad)
    assert T.parse_parameters("k_w,tau,Izz", "e2e") == ["k_w", "tau", "Izz"] and T.parse_parameters("", "indi")[0] == "k_x"
    for bad, variant in (("k_w", "indi"), ("mass", "e2e"), ("tau,tau", "e2e")):
        with pytest.raises(SystemExit):
            T.parse_parameters(bad, variant)
    cell = lambda c, lap: dict(window=dict(crashes_per_window=c, gates_per_window=10.0), total=dict(flying_lap_seconds=lap))
    lines = T.format_table("m.zip", "k_w", [0.7, 1.0], [cell(0.5, None), cell(0.0, 2.75)]).split("\n")
    assert lines[0] == "m.zip  k_w" and lines[2].startswith("  x0.7") and "-" in lines[2] and lines[3].startswith("* x1") and "2.750" in lines[3]


# ---- the restatement against the C oracle, and the honesty conditions of the GPU test ----------------------------------------------------------
def _oracle_step(variant, world, dist, action):
    from oracle import oracle as O
    import eval_spec

    n = world.shape[0]
    env = O.OracleEnv(O.E2E if variant == 0 else O.INDI, n, *eval_spec.scenario_track(), 1)
    env.set_residual(None)
    env.set_limits(10 ** 6, 0.01)
    env.seed(1)
    env.reset()
    env.world_states[:] = world
    if dist is not None:
        env.disturbances[:] = dist
    env.target_gates[:] = 0
    env.step_counts[:] = 0
    _, _, done, _ = env.step(np.tile(np.asarray(action, np.float32), (n, 1)))
    return env.world_states.copy(), done


@pytest.mark.parametrize("variant", [0, 1])
def test_restatement_equals_the_oracle_step_at_nominal_coefficients(variant):
    from optimal_quad_control_rl_amd.dynamics import DynamicsParams

    world, dist = D.injected_states(variant)
    new, done = _oracle_step(variant, world, dist, D.ACTION[variant])
    assert int(done.sum()) == 0                                  # no injected state ends its episode within the step
    want = D.step(variant, DynamicsParams.nominal(variant).coeffs, world, D.ACTION[variant], dist)
    err = parity.rel_err(new, want)
    print("variant", variant, "oracle vs restatement: max rel_err %.3e (column %d)" % (err.max(), int(err.max(axis=0).argmax())))
    assert err.max() <= D.ORACLE_ERR[variant]                    # the measurement the GPU tolerance is derived from (dynamics_spec.tolerance)
    assert D.tolerance(0) == 4 * 5.28e-7 and D.tolerance(1) == 1e-6


@pytest.mark.parametrize("variant", [0, 1])
def test_every_perturbed_entry_is_visible_from_the_injected_states(variant):
    """The second honesty condition of the GPU test, re-checked for the exact seed: under the restatement each table with one entry
    x 1.25 moves at least three quarters of the 256 envs by >= 1e-4 (parity.rel_err) away from the nominal step."""
    from optimal_quad_control_rl_amd.dynamics import ENTRIES, DynamicsParams

    world, dist = D.injected_states(variant)
    assert world.shape == (256, 16 if variant == 0 else 13) and world.dtype == np.float32
    assert np.all(np.abs(world[:, 0]) < 9.9) and np.all(np.abs(world[:, 1]) < 9.9) and np.all(world[:, 2] <= -1.0)
    tables = D.perturbed_tables(DynamicsParams.nominal(variant).coeffs)
    assert len(tables) == D.COUNT[variant] + 1
    base = D.step(variant, tables[0], world, D.ACTION[variant], dist)
    for k, t in enumerate(tables[1:]):
        moved = parity.rel_err(D.step(variant, t, world, D.ACTION[variant], dist), base).max(axis=1) >= 1e-4
        print("variant", variant, "entry %2d %-14s moves %5.1f %% of the envs" % (k, ENTRIES[variant][k], 100.0 * moved.mean()))
        assert moved.mean() >= 0.75, (k, ENTRIES[variant][k], moved.mean())
