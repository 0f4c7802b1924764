"""GPU: the dynamics-grid evaluator (qr_evaluate_policy_dynamics_grid, eval_policy_dynamics_grid_kernel<V, GA, kF32>).

1. With every slot nominal it IS the grid evaluator (qr_evaluate_policy_grid, which tests/test_gpu_eval_grid.py pins to the single-policy
   evaluator and that to tests/eval_spec.py): records, float records, state and observation buffer bit-equal -- the runtime form of the
   equations of motion reproduces the literals.
2. Every coefficient sits in its term: one group per table entry with that entry x 1.25, one step from injected states, against the
   float64 restatement tests/dynamics_spec.py under the group's table.  Tolerance (parity.rel_err of the new world state):
   dynamics_spec.tolerance -- the project's teacher-forced one-step bound of 1e-6 for INDI; for E2E four times the C oracle's own error
   against the restatement, 4 x 5.28e-7 = 2.112e-6, because that error (measured in tests/test_dynamics_host.py) exceeds a quarter of
   1e-6.  Measured here (one run): E2E max 6.61e-07 over the 23 groups (the motor_gain group), INDI max 1.18e-07 over the 13.
3. The loop carries them: K steps in one launch equal K launches of one step under three non-nominal vehicles, bit for bit.
4. A cell depends on its (policy, condition, dynamics) triple only.   5. Refusals touch nothing.   6. Its time, printed."""
import ctypes as C
import statistics

import numpy as np
import pytest
import torch

import dynamics_spec as D
import eval_spec as S
import parity
from eval_helpers import SENTINEL, _constant_layers, _policy_bank, _ptr, _records
from test_gpu_eval_grid import _condition_bank, _conditions, _twin, _two_policies

pytestmark = pytest.mark.gpu

SC = S.SCENARIO
VAR = {"e2e": 0, "indi": 1}
MIXED_POL, MIXED_COG = [1, 0, 1, 1, 0, 1, 0], [2, 0, 2, 1, 1, 0, 2]      # test_gpu_eval_grid's arbitrary group map


def _dynamics_bank(variant, params, capacity=None):
    """params: DynamicsParams, a raw float32 table, or None (the NULL form of qr_dynamics_bank_set) per slot"""
    from optimal_quad_control_rl_amd.dynamics import DynamicsBank, DynamicsParams

    bank = DynamicsBank(VAR[variant], capacity or len(params))
    for slot, p in enumerate(params):
        bank.set(slot, p if p is None or isinstance(p, DynamicsParams) else DynamicsParams(VAR[variant], p))
    return bank


def _raw(env, pbank, cbank, dbank, E, pol, cog, dog, K, rec, recf, flags=0):
    """the C entry point itself: no observation refresh between calls"""
    i32p = C.POINTER(C.c_int32)
    arr = [None if m is None else np.asarray(m, np.int32) for m in (pol, cog, dog)]
    ptr = [None if a is None else a.ctypes.data_as(i32p) for a in arr]
    n = next((len(a) for a in arr if a is not None), 0)
    return env._L.qr_evaluate_policy_dynamics_grid(env._h, pbank._h if pbank is not None else None, cbank._h if cbank is not None else None,
                                                   dbank._h if dbank is not None else None, n, E, ptr[0], ptr[1], ptr[2], K, flags, _ptr(rec),
                                                   _ptr(recf), env._stream())


def _same_state(a, b, what):
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), a.get_state_tensors(), b.get_state_tensors()):
        assert x is None or torch.equal(x, y), (what, name)


# ---- 1. nominal slots: the grid evaluator, bit for bit ------------------------------------------------------------------------------------------
_NOMINAL = [(v, g, p, SC["steps"]) for v in ("e2e", "indi") for g in (0, 1) for p in ("f16-operands", "f32")]
_NOMINAL += [(v, g, p, 64) for v in ("e2e", "indi") for g in (2, 3, 4) for p in ("f16-operands", "f32")]


@pytest.mark.parametrize("variant,gates_ahead,precision,K", _NOMINAL, ids=["%s-ga%d-%s-K%d" % c for c in _NOMINAL])
def test_nominal_slots_equal_the_grid_evaluator(variant, gates_ahead, precision, K):
    from optimal_quad_control_rl_amd.dynamics import DynamicsParams

    E, pol, cog = 256, MIXED_POL, MIXED_COG
    dog = [0, 1, 0, 1, 1, 0, 1]                  # slot 0: set from NULL; slot 1: the table qr_dynamics_nominal returns, read back
    conds = _conditions(variant)
    a, b = (_twin(variant, len(pol) * E, gates_ahead, conds[0].replace(max_steps=97)) for _ in range(2))
    sets = _two_policies(variant, a.state_len)
    pbank, cbank = _policy_bank(a.state_len, sets), _condition_bank(variant, conds)
    nominal = DynamicsParams.nominal(VAR[variant])
    dbank = _dynamics_bank(variant, [None, nominal], capacity=3)
    assert np.array_equal(dbank.read(0).view(np.int32), nominal.coeffs.view(np.int32)) and np.array_equal(dbank.read(1), dbank.read(0))
    a.condition_starts(conds, cog, E); b.condition_starts(conds, cog, E)
    start = a.get_state_tensors()[0].clone()
    _same_state(a, b, "starts")
    ra, rfa = _records(a)
    rb, rfb = _records(b)
    a.evaluate_grid_device(pbank, cbank, pol, cog, E, K, ra, rfa, precision=precision)
    b.evaluate_dynamics_grid_device(pbank, cbank, dbank, pol, cog, dog, E, K, rb, rfb, precision=precision)
    # non-vacuity, on the grid launch's own records
    r = ra.cpu().numpy()
    assert bool((ra[:, 5] == K).all()) and not torch.equal(a.get_state_tensors()[0], start)
    passes, ends = int(r[:, 0].sum()), int(r[:, 1].sum() + r[:, 2].sum())
    print(variant, gates_ahead, precision, K, "passes", passes, "ends", ends)
    if K == SC["steps"]:
        for g in range(len(pol)):
            rg = r[g * E:(g + 1) * E]
            assert int(rg[:, 0].sum()) > 0 and int(rg[:, 1].sum() + rg[:, 2].sum()) > 0, g
    assert torch.equal(ra, rb), ("integer records", int((ra != rb).any(dim=1).sum()))
    assert torch.equal(rfa.view(torch.int32), rfb.view(torch.int32)), "float records"
    _same_state(a, b, "after")
    assert torch.equal(a.states_tensor, b.states_tensor), "observation buffer"
    a.close(); b.close(); pbank.close(); cbank.close(); dbank.close()


# ---- 2. every coefficient lands in its term ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_every_coefficient_lands_in_its_term(variant):
    from optimal_quad_control_rl_amd import Quadcopter3DGates, Quadcopter3DGatesINDI
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.dynamics import ENTRIES, DynamicsParams

    v, E = VAR[variant], 256
    tables = D.perturbed_tables(DynamicsParams.nominal(v).coeffs)          # [nominal] + one per entry x 1.25
    G = len(tables)
    assert G == (23 if v == 0 else 13)
    cls = Quadcopter3DGates if v == 0 else Quadcopter3DGatesINDI
    env = cls(G * E, *S.scenario_track(), gates_ahead=1, seed=SC["seed"], residual=None, infos_mode="none")
    env.max_steps = 10 ** 6
    env.reset_device()
    world, dist = D.injected_states(v)
    env.set_state_tensors(world=np.tile(world, (G, 1)), dist=None if dist is None else np.tile(dist, (G, 1)),
                          target=np.zeros(G * E, np.int32), steps=np.zeros(G * E, np.int32))
    pbank = _policy_bank(env.state_len, [_constant_layers(env.state_len, D.ACTION[v])])
    cbank = _condition_bank(variant, [Condition.from_env(env)])
    dbank = _dynamics_bank(variant, tables)
    rec, recf = _records(env)
    env.evaluate_dynamics_grid_device(pbank, cbank, dbank, [0] * G, [0] * G, list(range(G)), E, 1, rec, recf)
    new = env.get_state_tensors()[0].cpu().numpy()
    ended = (rec[:, 1] + rec[:, 2]).cpu().numpy() != 0
    tol = D.tolerance(v)
    base = D.step(v, tables[0], world, D.ACTION[v], dist)
    worst = 0.0
    for g in range(G):
        keep = ~ended[g * E:(g + 1) * E]
        assert (~keep).mean() <= 0.05, (g, (~keep).mean())                                    # at most 5 % left out as ended
        want = D.step(v, tables[g], world, D.ACTION[v], dist)
        if g:
            moved = parity.rel_err(want, base).max(axis=1) >= 1e-4
            assert moved.mean() >= 0.75, (g, moved.mean())                                    # the perturbation is visible from these states
        err = parity.rel_err(new[g * E:(g + 1) * E][keep], want[keep])
        worst = max(worst, float(err.max()))
        print(variant, "group %2d %-14s max rel_err %.3e (tolerance %.3e), ended %d" % (g, "nominal" if g == 0 else ENTRIES[v][g - 1], err.max(), tol,
                                                                                         int((~keep).sum())))
        assert err.max() <= tol, (g, float(err.max()), tol)
    print(variant, "max over the groups %.3e" % worst)
    env.close(); pbank.close(); cbank.close(); dbank.close()


# ---- 3. K steps equal K launches of one step -------------------------------------------------------------------------------------------------------
def _vehicles(variant, count=3, seed=11):
    """`count` vehicles, every physical parameter with its own factor in 0.8 .. 1.2"""
    from optimal_quad_control_rl_amd import dynamics as M

    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        phys = {name: x * float(rng.uniform(0.8, 1.2)) for name, x in M.PHYSICAL[VAR[variant]].items()}
        out.append(M.DynamicsParams.from_physical(VAR[variant], name="vehicle %d" % k, **phys))
    return out


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_k_steps_equal_k_launches_of_one_step(variant):
    from optimal_quad_control_rl_amd import _lib

    K, E, pol, cog, dog = 48, 256, [1, 0, 1], [0, 1, 2], [0, 1, 2]
    conds = _conditions(variant)
    vehicles = _vehicles(variant)
    assert len({v.coeffs.tobytes() for v in vehicles}) == 3
    envs = [_twin(variant, 3 * E, 1, conds[0]) for _ in range(3)]       # E2E: the residual MLPs are on (the default)
    a, b, c = envs
    pbank, cbank = _policy_bank(a.state_len, _two_policies(variant, a.state_len)), _condition_bank(variant, conds)
    dbank = _dynamics_bank(variant, vehicles + [None])
    recs = []
    for env in envs:
        env.condition_starts(conds, cog, E)
        recs.append(_records(env))
    assert _raw(a, pbank, cbank, dbank, E, pol, cog, dog, K, *recs[0]) == _lib.QR_OK
    for _ in range(K):
        assert _raw(b, pbank, cbank, dbank, E, pol, cog, dog, 1, *recs[1]) == _lib.QR_OK
    assert _raw(c, pbank, cbank, dbank, E, pol, cog, [3, 3, 3], K, *recs[2]) == _lib.QR_OK     # the nominal vehicle
    torch.cuda.synchronize()
    assert bool((recs[0][0][:, 5] == K).all())
    assert torch.equal(recs[0][0], recs[1][0]) and torch.equal(recs[0][1].view(torch.int32), recs[1][1].view(torch.int32))
    _same_state(a, b, "K launches")
    # non-vacuity: every perturbed group's records differ from the nominal ones
    for g in range(3):
        lo, hi = g * E, (g + 1) * E
        same = torch.equal(recs[0][0][lo:hi], recs[2][0][lo:hi]) and torch.equal(recs[0][1][lo:hi].view(torch.int32), recs[2][1][lo:hi].view(torch.int32))
        assert not same, g
    for env in envs:
        env.close()
    pbank.close(); cbank.close(); dbank.close()


# ---- 4. a cell depends on its triple only ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_a_cell_depends_on_its_triple_only(variant):
    from optimal_quad_control_rl_amd import _lib

    K, E = 300, 256
    conds, vehicles = _conditions(variant), _vehicles(variant)
    cells = [(0, 0, 0), (1, 1, 1), (0, 2, 2), (1, 0, 1)]                           # (policy, condition, dynamics) of groups 0..3
    order = [2, 0, 3, 1]                                                          # launch B: group j flies cell order[j] ...
    pperm, cperm, dperm = [1, 0], [2, 0, 1], [3, 1, 4]                            # ... out of other slots of each bank
    a, b = _twin(variant, 4 * E, 1, conds[0]), _twin(variant, 4 * E, 1, conds[0])
    sets = _two_policies(variant, a.state_len)
    pa, ca, da = _policy_bank(a.state_len, sets), _condition_bank(variant, conds), _dynamics_bank(variant, vehicles)
    pb = _policy_bank(a.state_len, [sets[pperm.index(s)] for s in range(2)])
    cb = _condition_bank(variant, [conds[cperm.index(s)] for s in range(3)])
    db = _dynamics_bank(variant, [vehicles[dperm.index(s)] if s in dperm else None for s in range(5)])
    a.condition_starts(conds, [c for _, c, _ in cells], E)
    state = a.get_state_tensors()
    rows = torch.cat([torch.arange(order[j] * E, (order[j] + 1) * E) for j in range(4)]).to(a.device)
    b.set_state_tensors(*[None if t is None else t[rows] for t in state])        # the same group-local starts
    ra, rfa = _records(a)
    rb, rfb = _records(b)
    assert _raw(a, pa, ca, da, E, [p for p, _, _ in cells], [c for _, c, _ in cells], [d for _, _, d in cells], K, ra, rfa) == _lib.QR_OK
    assert _raw(b, pb, cb, db, E, [pperm[cells[o][0]] for o in order], [cperm[cells[o][1]] for o in order], [dperm[cells[o][2]] for o in order],
                K, rb, rfb) == _lib.QR_OK
    torch.cuda.synchronize()
    assert int(ra[:, 0].sum()) > 0 and int(ra[:, 1].sum() + ra[:, 2].sum()) > 0
    assert torch.equal(ra[rows], rb) and torch.equal(rfa[rows].view(torch.int32), rfb.view(torch.int32))
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), a.get_state_tensors(), b.get_state_tensors()):
        assert x is None or torch.equal(x[rows], y), name
    assert not torch.equal(ra[:E], ra[3 * E:])                                     # cells 0 and 3 differ in policy and vehicle: so do their records
    a.close(); b.close()
    for bank in (pa, ca, da, pb, cb, db):
        bank.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_dynamics_grid_refusals_launch_nothing():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.dynamics import DynamicsBank, DynamicsParams

    G, E, K = 2, 256, 8
    n = G * E
    conds = _conditions("indi")
    env = _twin("indi", n, 1, conds[0])
    L = env._L
    pbank = _policy_bank(env.state_len, _two_policies("indi", env.state_len), capacity=3)
    cbank = _condition_bank("indi", conds[:2], capacity=3)
    dbank = _dynamics_bank("indi", _vehicles("indi", 2), capacity=3)            # slots 0, 1 set, slot 2 never set
    assert L.qr_dynamics_bank_capacity(dbank._h) == 3
    rec = torch.full((n, S.REC_INTS), 7, dtype=torch.int32, device=env.device)
    recf = torch.full((n, S.REC_FLOATS), SENTINEL, dtype=torch.float32, device=env.device)
    before = env.get_state_tensors()

    def refused(code, message, pb=pbank, cb=cbank, db=dbank, epg=E, pol=(0, 1), cog=(1, 0), dog=(1, 0), k=K, flags=0, r=rec):
        rc = _raw(env, pb, cb, db, epg, pol, cog, dog, k, r, recf, flags)
        assert rc == code, (message, rc, L.qr_last_error())
        assert b"qr_evaluate_policy_dynamics_grid" in L.qr_last_error() and message in L.qr_last_error(), L.qr_last_error()
        torch.cuda.synchronize()
        assert bool((rec == 7).all()) and bool((recf == SENTINEL).all())
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    # what qr_evaluate_policy_grid refuses, in its order: a missing condition bank is named before a missing dynamics bank, ...
    refused(_lib.QR_E_INVALID, b"policy bank", pb=None, cb=None, db=None)
    refused(_lib.QR_E_INVALID, b"condition bank", cb=None, db=None)
    refused(_lib.QR_E_INVALID, b"rec_dev", r=None)
    refused(_lib.QR_E_INVALID, b"num_steps", k=0)
    refused(_lib.QR_E_INVALID, b"flags", flags=1)
    refused(_lib.QR_E_INVALID, b"multiple of 256", epg=128, pol=(0, 1, 0, 1), cog=(0, 1, 0, 1), dog=(0, 1, 0, 1))
    refused(_lib.QR_E_INVALID, b"must equal the env count", pol=(0,), cog=(0,), dog=(0,))
    refused(_lib.QR_E_INVALID, b"policy_of_group[1]", pol=(0, 3), dog=(0, 5))       # ... and a bad policy index before a bad dynamics index
    refused(_lib.QR_E_STATE, b"condition bank was never set", cog=(2, 0), dog=(2, 0))
    # the dynamics bank's own
    refused(_lib.QR_E_INVALID, b"null dynamics bank", db=None)
    refused(_lib.QR_E_INVALID, b"three group maps", dog=None)
    refused(_lib.QR_E_INVALID, b"three group maps", pol=None)
    other = _dynamics_bank("e2e", [None, None])
    refused(_lib.QR_E_INVALID, b"dynamics bank of another variant", db=other)
    other.close()
    refused(_lib.QR_E_INVALID, b"dynamics_of_group[0] is outside the dynamics bank", dog=(3, 0))
    refused(_lib.QR_E_INVALID, b"dynamics_of_group[1] is outside the dynamics bank", dog=(0, -1))
    refused(_lib.QR_E_INVALID, b"dynamics_of_group[1] is outside the dynamics bank", dog=(0, 2 ** 31 - 1))
    refused(_lib.QR_E_STATE, b"slot 2 of the dynamics bank was never set", dog=(2, 0))
    if torch.cuda.device_count() > 1:
        far = DynamicsBank(1, 2, device=1)
        far.set(0); far.set(1)
        torch.cuda.set_device(0)
        refused(_lib.QR_E_INVALID, b"dynamics bank on another GPU", db=far)
        far.close()
    # qr_dynamics_bank_set / _read
    f32p = C.POINTER(C.c_float)
    good = DynamicsParams.nominal(1).coeffs.copy()
    p = lambda x: x.ctypes.data_as(f32p)
    out = np.full(12, 7.0, np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        t = good.copy()
        t[5] = bad
        assert L.qr_dynamics_bank_set(dbank._h, 2, p(t), 12) == _lib.QR_E_INVALID and b"coefficient 5 is not finite" in L.qr_last_error()
    assert L.qr_dynamics_bank_set(dbank._h, 2, p(good), 22) == _lib.QR_E_INVALID and b"count" in L.qr_last_error()
    assert L.qr_dynamics_bank_set(dbank._h, 3, p(good), 12) == _lib.QR_E_INVALID and L.qr_dynamics_bank_set(dbank._h, -1, p(good), 12) == _lib.QR_E_INVALID
    assert L.qr_dynamics_bank_read(dbank._h, 2, p(out), 12) == _lib.QR_E_STATE and b"never set" in L.qr_last_error()
    assert L.qr_dynamics_bank_read(dbank._h, 0, p(out), 22) == _lib.QR_E_INVALID and L.qr_dynamics_bank_read(dbank._h, 3, p(out), 12) == _lib.QR_E_INVALID
    assert bool((out == 7.0).all())
    refused(_lib.QR_E_STATE, b"slot 2 of the dynamics bank was never set", dog=(2, 0))     # none of the refused sets filled slot 2
    assert np.array_equal(dbank.read(1), dbank.params[1].coeffs)
    # ... and a valid call runs and reports its time
    dbank.set(2)
    rec.zero_(); recf.zero_()
    assert _raw(env, pbank, cbank, dbank, E, (0, 1), (1, 0), (2, 0), K, rec, recf) == _lib.QR_OK
    assert _raw(env, pbank, cbank, dbank, E, (0, 1), (1, 0), (2, 0), K, rec, None, flags=2) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((rec[:, 5] == 2 * K).all()) and env.last_rollout_ms() > 0.0
    env.close(); pbank.close(); cbank.close(); dbank.close()


def test_python_evaluate_dynamics_grid_nominal_column_is_evaluate_grid():
    """1 policy x 2 conditions x 3 vehicles on a 4-group env (two launches, the second padded): the nominal vehicle's column equals
    evaluate_grid dict for dict, and a vehicle with 30 % less thrust coefficient flies differently."""
    from optimal_quad_control_rl_amd import evaluate_dynamics_grid, evaluate_grid, physical_sweep
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(5)
    net = ActorCritic(24, 4)
    with torch.no_grad():
        net.pi[-1].bias.copy_(torch.tensor([0.4, 0.4, 0.4, 0.4]))
    E, K, W, seed = 256, 400, 250, 99
    conds = _conditions("e2e")[:2]
    ev = _twin("e2e", 4 * E, 1, conds[0], seed=1)
    vehicles = physical_sweep(0, "k_w", [0.7, 1.0, 1.3])
    res = evaluate_dynamics_grid([net.pi], conds, vehicles, ev, envs_per_cell=E, n_eval_steps=K, window_steps=W, seed=seed)
    want = evaluate_grid([net.pi], conds, ev, envs_per_cell=E, n_eval_steps=K, window_steps=W, seed=seed)
    assert len(res) == 1 and len(res[0]) == 2 and all(len(r) == 3 for r in res[0])
    for c in range(2):
        assert res[0][c][1] == want[0][c], c
        assert res[0][c][0] != res[0][c][1] and res[0][c][2] != res[0][c][1]
    ev.close()


# ---- 6. time, printed ----------------------------------------------------------------------------------------------------------------------------
def test_dynamics_grid_time_is_printed():
    """Median us per step of qr_evaluate_policy_dynamics_grid with all-nominal slots and of qr_evaluate_policy_grid on the same handle:
    N = 65 536 = 256 groups x 256 envs, K = 200, E2E + residual MLPs + training disturbances, square track, one seeded network in every
    slot, every group on the condition that equals the handle's configuration; alternating launches, one warm-up pair, medians of 5,
    times from qr_last_step_many_ms (the protocol of test_gpu_eval_grid.test_grid_not_slower_than_the_bank).  NO bound is asserted.
    Measured (one run of this test, us per step, dynamics grid vs grid): f16 5.725 vs 5.635, ratio 1.016; f32 26.52 vs 26.67, ratio 0.995."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    n, K, E = 65536, 200, 256
    P = n // E
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=99)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = 10 ** 6
    torch.manual_seed(0)
    pi = ActorCritic(env.state_len, 4).pi
    layers = [(m.weight, m.bias) for m in pi if isinstance(m, torch.nn.Linear)]
    pbank = _policy_bank(env.state_len, [layers] * P)
    cbank = _condition_bank("e2e", [Condition.from_env(env)])
    dbank = _dynamics_bank("e2e", [None] * P)
    rec, recf = _records(env)
    pol, zero = list(range(P)), [0] * P
    for precision in ("f16-operands", "f32"):
        t_dyn, t_grid = [], []
        for rep in range(6):
            env.seed(99); env.reset_device(); rec.zero_(); recf.zero_()
            env.evaluate_dynamics_grid_device(pbank, cbank, dbank, pol, zero, pol, E, K, rec, recf, precision=precision)
            ms_d = env.last_rollout_ms()
            env.seed(99); env.reset_device(); rec.zero_(); recf.zero_()
            env.evaluate_grid_device(pbank, cbank, pol, zero, E, K, rec, recf, precision=precision)
            ms_g = env.last_rollout_ms()
            if rep:
                t_dyn.append(ms_d * 1e3 / K); t_grid.append(ms_g * 1e3 / K)
        md, mg = statistics.median(t_dyn), statistics.median(t_grid)
        print("%s: qr_evaluate_policy_dynamics_grid %s -> median %.4f us/step; qr_evaluate_policy_grid %s -> median %.4f us/step; ratio %.4f"
              % (precision, ["%.4f" % t for t in t_dyn], md, ["%.4f" % t for t in t_grid], mg, md / mg))
        assert md > 0.0 and mg > 0.0
    env.close(); pbank.close(); cbank.close(); dbank.close()
