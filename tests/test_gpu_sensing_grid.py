"""GPU: the sensing-grid evaluator (qr_evaluate_policy_sensing_grid, eval_policy_sensing_grid_kernel<V, GA, kF32>) and its noise dump
(qr_sensing_noise, sensing_noise_kernel<V, GA>), csrc/quadrace_eval_sensing.hip.  Model: include/quadrace.h, restated in
tests/sensing_spec.py.

1. Ideal slots ARE the dynamics-grid evaluator (which tests/test_gpu_dynamics_grid.py pins to the grid evaluator, that to the single-policy
   evaluator and that to tests/eval_spec.py): records, float records, state and observation bit-equal, pending all zero.
2. The dumped noise equals the restatement (the bounds of tests/test_gpu_action_noise.py: the float32 operations are the action noise's)
   and is rejected against its neighbours; each sigma lands on its group only.
3. The closed loop with noise and delay equals a per-step loop on a twin handle, bit for bit:
       K x [ states_tensor + dumped noise[k] -> qr_policy_forward -> clamp -> torch-side queue with clear-on-done -> qr_step ]
   with the records from eval_spec.run.  No tolerance.
4. K steps in one call equal K calls of one step, d = 3, across episode ends.   5. A group depends on its quadruple only.
6. Refusals touch nothing.   7. Python: the ideal column of evaluate_sensing_grid is evaluate_dynamics_grid.   8. Its time, printed."""
import ctypes as C
import statistics

import numpy as np
import pytest
import torch

import action_noise as N
import eval_spec as S
import sensing_spec as SS
from eval_helpers import SENTINEL, _closed_loop_layers, _policy_bank, _ptr, _records
from test_gpu_dynamics_grid import _dynamics_bank, _same_state
from test_gpu_eval_grid import _condition_bank, _conditions, _twin, _two_policies
from test_gpu_evaluate import _target

pytestmark = pytest.mark.gpu

SC = S.SCENARIO
VAR = {"e2e": 0, "indi": 1}
NOISY = (0.05, 0.1, 0.02, 0.2, 0.05, 0.05, 0.02, 0.1)          # one non-zero sigma per group
BASE = 2 ** 32 - 300                                            # env_id_base: the low word of the env id wraps inside a 512-env group


def _sensing_bank(params, capacity=None):
    """params: SensingParams or None (the NULL form of qr_sensing_bank_set) per slot"""
    from optimal_quad_control_rl_amd.sensing import SensingBank

    bank = SensingBank(capacity or len(params))
    for slot, p in enumerate(params):
        bank.set(slot, p)
    return bank


def _sensor(sigma8=(0,) * 8, delay=0):
    from optimal_quad_control_rl_amd.sensing import SensingParams

    return SensingParams.from_sigma(sigma8, delay)


def _pending(env, fill=0.0):
    return torch.full((env.num_envs, 16), fill, dtype=torch.float32, device=env.device)


def _raw(env, pbank, cbank, dbank, sbank, E, pol, cog, dog, sog, K, pending, rec, recf, flags=0, seed=0, first=0):
    """the C entry point itself: no observation refresh between calls"""
    i32p = C.POINTER(C.c_int32)
    arr = [None if m is None else np.asarray(m, np.int32) for m in (pol, cog, dog, sog)]
    ptr = [None if a is None else a.ctypes.data_as(i32p) for a in arr]
    n = next((len(a) for a in arr if a is not None), 0)
    h = lambda b: b._h if b is not None else None
    return env._L.qr_evaluate_policy_sensing_grid(env._h, h(pbank), h(cbank), h(dbank), h(sbank), n, E, *ptr, K, flags, seed, first,
                                                  pending if isinstance(pending, C.c_void_p) else _ptr(pending), _ptr(rec), _ptr(recf), env._stream())


def _based_twin(variant, n, gates_ahead, cond, env_id_base, seed=SC["seed"]):
    """test_gpu_eval_grid._twin with an env_id_base"""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, Quadcopter3DGatesINDI

    trk = (cond.gate_pos, cond.gate_yaw, cond.start_pos)
    if variant == "e2e":
        env = Quadcopter3DGates(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none", env_id_base=env_id_base)
        env.disturbance_ranges = cond.disturbance_ranges
        env.disturbance_scale = cond.disturbance_scale
    else:
        env = Quadcopter3DGatesINDI(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none", env_id_base=env_id_base)
    env.max_steps = cond.max_steps
    env.reset_device()
    return env


def _bits(t):
    return t.view(torch.int32)


# ---- 1. ideal slots: the dynamics-grid evaluator, bit for bit -----------------------------------------------------------------------------------
_IDEAL = [(v, g, p) for v in ("e2e", "indi") for g in range(5) for p in ("f16-operands", "f32")]


@pytest.mark.parametrize("variant,gates_ahead,precision", _IDEAL, ids=["%s-ga%d-%s" % c for c in _IDEAL])
def test_ideal_slots_equal_the_dynamics_grid(variant, gates_ahead, precision):
    E, K, pol, cog, dog, sog = 256, 40, [1, 0, 1, 1], [2, 0, 1, 2], [0, 0, 0, 0], [0, 1, 1, 0]
    conds = [c.replace(max_steps=21 + 4 * k) for k, c in enumerate(_conditions(variant))]      # time limits inside the 40 steps
    a, b = (_twin(variant, len(pol) * E, gates_ahead, conds[0].replace(max_steps=97)) for _ in range(2))
    pbank, cbank = _policy_bank(a.state_len, _two_policies(variant, a.state_len)), _condition_bank(variant, conds)
    dbank = _dynamics_bank(variant, [None])
    sbank = _sensing_bank([None, _sensor()], capacity=3)          # slot 0: set from NULL; slot 1: zero sigmas, zero delay
    for slot in (0, 1):
        sigma, delay = sbank.read(slot)
        assert not sigma.view(np.int32).any() and delay == 0
    a.condition_starts(conds, cog, E); b.condition_starts(conds, cog, E)
    start = a.get_state_tensors()[0].clone()
    _same_state(a, b, "starts")
    ra, rfa = _records(a)
    rb, rfb = _records(b)
    pend = _pending(b)
    a.evaluate_dynamics_grid_device(pbank, cbank, dbank, pol, cog, dog, E, K, ra, rfa, precision=precision)
    b.evaluate_sensing_grid_device(pbank, cbank, dbank, sbank, pol, cog, dog, sog, E, K, pend, rb, rfb, precision=precision, noise_seed=0xC0FFEE,
                                   first_step=2 ** 32 - 7)
    r = ra.cpu().numpy()
    ends = int(r[:, 1].sum() + r[:, 2].sum())
    print(variant, gates_ahead, precision, "passes", int(r[:, 0].sum()), "ends", ends)
    assert bool((ra[:, 5] == K).all()) and not torch.equal(a.get_state_tensors()[0], start) and ends >= len(pol) * E   # every env's episode ended
    assert torch.equal(ra, rb), ("integer records", int((ra != rb).any(dim=1).sum()))
    assert torch.equal(_bits(rfa), _bits(rfb)), "float records"
    _same_state(a, b, "after")
    assert torch.equal(_bits(a.states_tensor), _bits(b.states_tensor)), "observation buffer"
    assert not bool(_bits(pend).any()), "pending"
    a.close(); b.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close()


# ---- 2. the noise ---------------------------------------------------------------------------------------------------------------------------------
def _noise_env(variant, gates_ahead, n=256):
    cond = _conditions(variant)[0]
    return _based_twin(variant, n, gates_ahead, cond, BASE)


@pytest.mark.parametrize("variant,gates_ahead,E", [("indi", 0, 256), ("indi", 0, 512), ("e2e", 4, 256), ("e2e", 4, 512)])
def test_noise_matches_the_restatement_and_rejects_its_neighbours(variant, gates_ahead, E):
    """L = 13: the last block is partial; L = 36: nine blocks.  sigma = 0.5 in every group, so dump / 0.5 is eps exactly.  The restated
    values stand in for the three entries of the partial block that no observation entry takes."""
    from test_gpu_action_noise import CEILING, EPS_TOL, assert_eps

    K, seed, first = 8, 0xC0FFEE + (0x5EED << 32), (5 << 32) + 2 ** 32 - 3          # the step's low word wraps at k = 3
    env = _noise_env(variant, gates_ahead)
    L = env.state_len
    assert L == SS.obs_len(VAR[variant], gates_ahead) == (13 if variant == "indi" else 36)
    Q = SS.num_blocks(L)
    sbank = _sensing_bank([_sensor((0.5,) * 8, 2), None])
    out = torch.full((K, E, L), SENTINEL, dtype=torch.float32, device=env.device)
    env.sensing_noise_device(sbank, 0, E, K, noise_seed=seed, first_step=first, out=out)
    dump = out.cpu().numpy()
    assert np.isfinite(dump).all() and not (dump == SENTINEL).any()
    eps64, u = SS.noise(L, E, K, seed, env_id_base=BASE, first_step=first)
    eps = eps64.copy()
    eps[:, :, :L] = dump.astype(np.float64) / 0.5
    shape = (K, E * Q, 4)
    rel = assert_eps(eps.reshape(shape), eps64.reshape(shape), tuple(x.reshape(K, E * Q) for x in u), "qr_sensing_noise %s L=%d E=%d" % (variant, L, E))
    print("qr_sensing_noise: measured max |eps - eps64| / max(1, |eps|) = %.3e (tolerance %.1e)" % (rel, EPS_TOL))
    wrong = {
        "swapped pairs": SS.noise(L, E, K, seed, BASE, first, swap_pairs=True)[0],
        "q in the step's low word": SS.noise(L, E, K, seed, BASE, first, q_word=2)[0],
        "q in the env id's high word": SS.noise(L, E, K, seed, BASE, first, q_word=1)[0],
        "the action-noise key": SS.noise(L, E, K, seed, BASE, first, key=N.noise_key(seed))[0],
        "env_id_base 0": SS.noise(L, E, K, seed, 0, first)[0],
        "first_step without its high word": SS.noise(L, E, K, seed, BASE, first % 2 ** 32)[0],
        "first_step + 1": SS.noise(L, E, K, seed, BASE, first + 1)[0],
        "seed ^ 2^63": SS.noise(L, E, K, seed ^ (1 << 63), BASE, first)[0],
    }
    for name, w in wrong.items():
        lo = 4 if name.startswith("q in") else 0                                     # block 0 carries q = 0 in any word
        d = np.abs(eps[:, :, lo:L] - w[:, :, lo:L])
        frac = float((d > 0.1).mean())
        assert frac > 0.8 and d.max() > 1.0, (name, frac)
        assert (d / np.maximum(1.0, np.abs(w[:, :, lo:L]))).max() > 100 * EPS_TOL and d.max() > 100 * CEILING, name
    # the ideal slot writes +0.0f
    env.sensing_noise_device(sbank, 1, E, K, noise_seed=seed, first_step=first, out=out.fill_(SENTINEL))
    assert not bool(_bits(out).any())
    # the dump does not depend on the delay, and a smaller E is a prefix
    small = env.sensing_noise_device(sbank, 0, 100, K, noise_seed=seed, first_step=first)
    assert torch.equal(_bits(small), _bits(env.sensing_noise_device(sbank, 0, E, K, noise_seed=seed, first_step=first)[:, :100]))
    env.close(); sbank.close()


@pytest.mark.parametrize("variant,gates_ahead", [("indi", 0), ("e2e", 4), ("e2e", 1), ("indi", 3)])
def test_each_sigma_lands_on_its_group_only(variant, gates_ahead):
    K, E, seed, first = 4, 256, 77, 9
    env = _noise_env(variant, gates_ahead)
    groups = SS.GROUPS[(VAR[variant], gates_ahead)]
    sigmas = [tuple(0.25 if g == k else 0.0 for g in range(8)) for k in range(8)]
    sbank = _sensing_bank([_sensor((0.25,) * 8)] + [_sensor(s) for s in sigmas])
    full = env.sensing_noise_device(sbank, 0, E, K, noise_seed=seed, first_step=first).cpu().numpy()
    assert (full != 0).mean() > 0.999
    for k in range(8):
        one = env.sensing_noise_device(sbank, 1 + k, E, K, noise_seed=seed, first_step=first).cpu().numpy()
        mine = groups == k
        assert np.array_equal(one[..., mine].view(np.int32), full[..., mine].view(np.int32)), k
        assert not one[..., ~mine].any(), k
    env.close(); sbank.close()


# ---- 3. the closed loop, bit for bit ------------------------------------------------------------------------------------------------------------
def _loop(twin, pol, noise, d, K, precision):
    """K x [obs + noise[k] -> forward -> clamp -> queue -> step]; returns eval_spec.run's sequences and the queue in canonical order"""
    n, dev = twin.num_envs, twin.device
    tb = torch.empty((K, n), dtype=torch.int32, device=dev)
    ta = torch.empty((K, n), dtype=torch.int32, device=dev)
    dn = torch.empty((K, n), dtype=torch.uint8, device=dev)
    tr = torch.empty((K, n), dtype=torch.uint8, device=dev)
    rw = torch.empty((K, n), dtype=torch.float32, device=dev)
    prev = torch.empty(n, dtype=torch.int32, device=dev)
    _target(twin, prev)
    queue = torch.zeros((n, 16), dtype=torch.float32, device=dev)
    obs = twin.states_tensor
    for k in range(K):
        seen = obs if noise is None else obs + noise[k]
        act = pol.forward(seen.contiguous(), precision=precision).clamp(-1, 1).contiguous()
        if d > 0:
            fly = queue[:, 4 * (d - 1):4 * d].clone()
            queue[:, 4:4 * d] = queue[:, :4 * (d - 1)].clone()
            queue[:, :4] = act
        else:
            fly = act
        obs, r, dd, t = twin.step_device(fly.contiguous())
        queue[dd.bool()] = 0.0
        rw[k].copy_(r); dn[k].copy_(dd); tr[k].copy_(t)
        tb[k].copy_(prev)
        _target(twin, ta[k])
        prev = ta[k]
    return [x.cpu().numpy() for x in (tb, ta, dn, tr, rw)], queue


_LOOP = [(v, p, d, E) for v in ("e2e", "indi") for p in ("f16-operands", "f32") for d in (0, 1, 4) for E in (256, 512)]


@pytest.mark.parametrize("variant,precision,d,E", _LOOP, ids=["%s-%s-d%d-E%d" % c for c in _LOOP])
def test_closed_loop_equals_the_per_step_loop(variant, precision, d, E):
    """group 1 of four flies (noise, delay d) and is held against the loop; groups 0, 2, 3 fly ideal, noise alone and delay alone (d, or 1
    where d = 0) from the same start, and their records must differ from one another where the sensors differ."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    K, gpl, ga, seed, first = SC["steps"], SC[variant + "_gates_per_lap"], 1, 0xFACE + (3 << 32), 2 ** 32 - 250
    cond = _conditions(variant)[0]
    env = _based_twin(variant, 4 * E, ga, cond.replace(max_steps=97), BASE)
    twin = _based_twin(variant, E, ga, cond, BASE)
    layers = _closed_loop_layers(env.state_len, SC[variant + "_action"], seed=3)
    pbank, cbank, dbank = _policy_bank(env.state_len, [layers]), _condition_bank(variant, [cond]), _dynamics_bank(variant, [None])
    pol = MfmaPolicy(env.state_len).set_weights(layers)
    sbank = _sensing_bank([None, _sensor(NOISY, d), _sensor(NOISY, 0), _sensor(delay=d or 1)])
    env.condition_starts([cond], [0] * 4, E)
    state = env.get_state_tensors()
    twin.set_state_tensors(*[None if t is None else t[E:2 * E] for t in state])
    twin.update_states()
    rec, recf = _records(env)
    pend = _pending(env)
    assert _raw(env, pbank, cbank, dbank, sbank, E, [0] * 4, [0] * 4, [0] * 4, [0, 1, 2, 3], K, pend, rec, recf, 2 if precision == "f32" else 0,
                seed, first) == 0
    noise = env.sensing_noise_device(sbank, 1, E, K, noise_seed=seed, first_step=first)
    seq, queue = _loop(twin, pol, noise, d, K, precision)
    srec, srecf = S.run(*S.new_records(E), *seq, gates_per_lap=gpl)
    ends, passes = int(srec[:, 1].sum() + srec[:, 2].sum()), int(srec[:, 0].sum())
    print(variant, precision, "d", d, "E", E, "passes", passes, "crashes", int(srec[:, 1].sum()), "time limits", int(srec[:, 2].sum()))
    assert ends >= E and bool((srec[:, 5] == K).all())                          # non-vacuity: every env's episode ended inside the window
    lo, hi = E, 2 * E
    got, gotf = rec[lo:hi].cpu().numpy(), recf[lo:hi].cpu().numpy()
    bad = np.nonzero((got != srec).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:2]], srec[bad[:2]])
    assert np.array_equal(gotf.view(np.uint32), srecf.view(np.uint32)), "float records"
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), env.get_state_tensors(), twin.get_state_tensors()):
        assert x is None or torch.equal(x[lo:hi], y), name
    assert torch.equal(_bits(pend[lo:hi]), _bits(queue)), "pending"
    assert d == 0 or bool(pend[lo:hi, :4 * d].any())
    assert not bool(_bits(pend[:E]).any()) and not bool(_bits(pend[2 * E:3 * E]).any()) and not bool(_bits(pend[:, 4 * max(d, 1):]).any())
    # the sensors matter: ideal / noise alone / delay alone / both give different records
    cells = [(rec[g * E:(g + 1) * E], _bits(recf[g * E:(g + 1) * E])) for g in range(4)]
    same = lambda i, j: torch.equal(cells[i][0], cells[j][0]) and torch.equal(cells[i][1], cells[j][1])
    assert not same(0, 2), "noise alone"
    assert not same(0, 3), "delay alone"
    assert d == 0 or not same(1, 2)
    env.close(); twin.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close(); pol.close() if hasattr(pol, "close") else None


# ---- 4. continuation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_k_steps_equal_k_launches_of_one_step(variant):
    K, E, d, seed, first = 64, 256, 3, 1234567, 2 ** 32 - 20
    pol, cog, dog, sog = [1, 0, 1], [0, 1, 2], [0, 0, 0], [0, 1, 0]
    conds = [c.replace(max_steps=19 + 6 * k) for k, c in enumerate(_conditions(variant))]     # several episode ends inside the 64 steps
    a, b = (_twin(variant, 3 * E, 1, conds[0]) for _ in range(2))
    pbank, cbank = _policy_bank(a.state_len, _two_policies(variant, a.state_len)), _condition_bank(variant, conds)
    dbank = _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(NOISY, d), _sensor(delay=d)])
    out = []
    for env in (a, b):
        env.condition_starts(conds, cog, E)
        out.append((_pending(env),) + _records(env))
    assert _raw(a, pbank, cbank, dbank, sbank, E, pol, cog, dog, sog, K, *out[0], seed=seed, first=first) == 0
    for k in range(K):
        assert _raw(b, pbank, cbank, dbank, sbank, E, pol, cog, dog, sog, 1, *out[1], seed=seed, first=first + k) == 0
    torch.cuda.synchronize()
    (pa, ra, rfa), (pb, rb, rfb) = out
    ends = (ra[:, 1] + ra[:, 2]).cpu().numpy()
    assert bool((ra[:, 5] == K).all()) and int(ends.min()) >= 1 and bool(pa[:, :4 * d].any()) and not bool(_bits(pa[:, 4 * d:]).any())
    assert torch.equal(ra, rb) and torch.equal(_bits(rfa), _bits(rfb))
    _same_state(a, b, "K launches")
    assert torch.equal(_bits(pa), _bits(pb)), "pending"
    # first_step matters: the same K calls without advancing it fly differently under the noisy slot
    c = _twin(variant, 3 * E, 1, conds[0])
    c.condition_starts(conds, cog, E)
    pc, rc, rfc = (_pending(c),) + _records(c)
    for k in range(K):
        assert _raw(c, pbank, cbank, dbank, sbank, E, pol, cog, dog, sog, 1, pc, rc, rfc, seed=seed, first=first) == 0
    torch.cuda.synchronize()
    assert not torch.equal(_bits(rfa[:E]), _bits(rfc[:E])) and torch.equal(_bits(rfa[E:2 * E]), _bits(rfc[E:2 * E]))
    a.close(); b.close(); c.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close()


# ---- 5. a group depends on its quadruple only ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_a_group_depends_on_its_quadruple_only(variant):
    from test_gpu_dynamics_grid import _vehicles

    K, E, seed, first = 300, 256, 42, 5
    conds, vehicles = _conditions(variant), _vehicles(variant, 2)
    sensors = [_sensor(NOISY, 2), _sensor(delay=4), _sensor(tuple(2 * s for s in NOISY), 0)]
    cells = [(0, 0, 0, 0), (1, 1, 1, 1), (0, 2, 1, 2), (1, 0, 0, 1)]                 # (policy, condition, dynamics, sensing) of groups 0..3
    order = [2, 0, 3, 1]                                                            # launch B: group j flies cell order[j] ...
    pperm, cperm, dperm, sperm = [1, 0], [2, 0, 1], [2, 0], [3, 1, 4]               # ... out of other slots of each bank
    a, b = _twin(variant, 4 * E, 1, conds[0]), _twin(variant, 4 * E, 1, conds[0])
    sets = _two_policies(variant, a.state_len)
    pa, ca, da, sa = _policy_bank(a.state_len, sets), _condition_bank(variant, conds), _dynamics_bank(variant, vehicles), _sensing_bank(sensors)
    pb = _policy_bank(a.state_len, [sets[pperm.index(s)] for s in range(2)])
    cb = _condition_bank(variant, [conds[cperm.index(s)] for s in range(3)])
    db = _dynamics_bank(variant, [vehicles[dperm.index(s)] if s in dperm else None for s in range(3)])
    sb = _sensing_bank([sensors[sperm.index(s)] if s in sperm else None for s in range(5)])
    a.condition_starts(conds, [c[1] for c in cells], E)
    state = a.get_state_tensors()
    rows = torch.cat([torch.arange(order[j] * E, (order[j] + 1) * E) for j in range(4)]).to(a.device)
    b.set_state_tensors(*[None if t is None else t[rows] for t in state])          # the same group-local starts
    qa, ra, rfa = (_pending(a),) + _records(a)
    qb, rb, rfb = (_pending(b),) + _records(b)
    col = lambda k: [c[k] for c in cells]
    assert _raw(a, pa, ca, da, sa, E, col(0), col(1), col(2), col(3), K, qa, ra, rfa, seed=seed, first=first) == 0
    assert _raw(b, pb, cb, db, sb, E, [pperm[cells[o][0]] for o in order], [cperm[cells[o][1]] for o in order], [dperm[cells[o][2]] for o in order],
                [sperm[cells[o][3]] for o in order], K, qb, rb, rfb, seed=seed, first=first) == 0
    torch.cuda.synchronize()
    assert int(ra[:, 0].sum()) > 0 and int(ra[:, 1].sum() + ra[:, 2].sum()) > 0
    assert torch.equal(ra[rows], rb) and torch.equal(_bits(rfa[rows]), _bits(rfb)) and torch.equal(_bits(qa[rows]), _bits(qb))
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), a.get_state_tensors(), b.get_state_tensors()):
        assert x is None or torch.equal(x[rows], y), name
    assert not torch.equal(ra[:E], ra[3 * E:]) and bool(qa[E:2 * E].any())
    a.close(); b.close()
    for bank in (pa, ca, da, sa, pb, cb, db, sb):
        bank.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_sensing_grid_refusals_launch_nothing():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.sensing import SensingBank
    from test_gpu_dynamics_grid import _vehicles

    G, E, K = 2, 256, 8
    n = G * E
    conds = _conditions("indi")
    env = _twin("indi", n, 1, conds[0])
    L = env._L
    pbank = _policy_bank(env.state_len, _two_policies("indi", env.state_len), capacity=3)
    cbank = _condition_bank("indi", conds[:2], capacity=3)
    dbank = _dynamics_bank("indi", _vehicles("indi", 2), capacity=3)           # slots 0, 1 set, slot 2 never set
    sbank = _sensing_bank([_sensor(NOISY, 2), None], capacity=3)               # slots 0, 1 set, slot 2 never set
    assert L.qr_sensing_bank_capacity(sbank._h) == 3
    rec = torch.full((n, S.REC_INTS), 7, dtype=torch.int32, device=env.device)
    recf = torch.full((n, S.REC_FLOATS), SENTINEL, dtype=torch.float32, device=env.device)
    pend = _pending(env, SENTINEL)
    before = env.get_state_tensors()
    LIMIT = 2 ** 56

    def untouched():
        torch.cuda.synchronize()
        assert bool((rec == 7).all()) and bool((recf == SENTINEL).all()) and bool((pend == SENTINEL).all())
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    def refused(code, message, pb=pbank, cb=cbank, db=dbank, sb=sbank, epg=E, pol=(0, 1), cog=(1, 0), dog=(1, 0), sog=(0, 1), k=K, flags=0, r=rec,
                q=pend, first=0):
        rc = _raw(env, pb, cb, db, sb, epg, pol, cog, dog, sog, k, q, r, recf, flags, 5, first)
        assert rc == code, (message, rc, L.qr_last_error())
        assert b"qr_evaluate_policy_sensing_grid" in L.qr_last_error() and message in L.qr_last_error(), L.qr_last_error()
        untouched()

    # everything qr_evaluate_policy_dynamics_grid refuses, in its order, ahead of anything about the sensing bank
    refused(_lib.QR_E_INVALID, b"policy bank", pb=None, cb=None, db=None, sb=None)
    refused(_lib.QR_E_INVALID, b"condition bank", cb=None, db=None, sb=None)
    refused(_lib.QR_E_INVALID, b"null dynamics bank", db=None, sb=None)
    refused(_lib.QR_E_INVALID, b"three group maps", dog=None, sog=None)
    refused(_lib.QR_E_INVALID, b"rec_dev", r=None, q=None)
    refused(_lib.QR_E_INVALID, b"num_steps", k=0, sb=None)
    refused(_lib.QR_E_INVALID, b"flags", flags=1, sog=None)
    refused(_lib.QR_E_INVALID, b"multiple of 256", epg=128, pol=(0, 1, 0, 1), cog=(0, 1, 0, 1), dog=(0, 1, 0, 1), sog=(0, 1, 0, 9))
    refused(_lib.QR_E_INVALID, b"must equal the env count", pol=(0,), cog=(0,), dog=(0,), sog=(9,))
    refused(_lib.QR_E_INVALID, b"policy_of_group[1]", pol=(0, 3), sog=(0, 5))
    refused(_lib.QR_E_STATE, b"condition bank was never set", cog=(2, 0), sog=(2, 0))
    refused(_lib.QR_E_INVALID, b"dynamics_of_group[0] is outside the dynamics bank", dog=(3, 0), sog=(3, 0))
    refused(_lib.QR_E_STATE, b"slot 2 of the dynamics bank was never set", dog=(2, 0), sb=None)
    # the sensing bank's own
    refused(_lib.QR_E_INVALID, b"null sensing bank", sb=None)
    refused(_lib.QR_E_INVALID, b"sensing_of_group is required", sog=None)
    refused(_lib.QR_E_INVALID, b"pending_dev is required", q=None)
    refused(_lib.QR_E_INVALID, b"pending_dev must be 16-byte aligned", q=C.c_void_p(pend.data_ptr() + 4))
    refused(_lib.QR_E_INVALID, b"sensing_of_group[0] is outside the sensing bank", sog=(3, 0))
    refused(_lib.QR_E_INVALID, b"sensing_of_group[1] is outside the sensing bank", sog=(0, -1))
    refused(_lib.QR_E_INVALID, b"sensing_of_group[1] is outside the sensing bank", sog=(0, 2 ** 31 - 1))
    refused(_lib.QR_E_INVALID, b"must not exceed 2^56", first=LIMIT - K + 1)
    refused(_lib.QR_E_INVALID, b"must not exceed 2^56", first=2 ** 64 - 1)
    refused(_lib.QR_E_INVALID, b"must not exceed 2^56", first=LIMIT - K + 1, sog=(2, 0))      # ... ahead of the unset slot
    refused(_lib.QR_E_STATE, b"slot 2 of the sensing bank was never set", sog=(2, 0))
    if torch.cuda.device_count() > 1:
        far = SensingBank(2, device=1)
        far.set(0); far.set(1)
        torch.cuda.set_device(0)
        refused(_lib.QR_E_INVALID, b"sensing bank on another GPU", sb=far)
        far.close()
    # qr_sensing_bank_set / _read
    f32p = C.POINTER(C.c_float)
    p = lambda x: x.ctypes.data_as(f32p)
    good = np.asarray(NOISY, np.float32)
    for k, bad in ((0, np.nan), (3, np.inf), (7, -np.inf), (5, -1e-6)):
        t = good.copy()
        t[k] = bad
        assert L.qr_sensing_bank_set(sbank._h, 2, p(t), 0) == _lib.QR_E_INVALID and b"sigma %d must be finite and >= 0" % k in L.qr_last_error()
    for bad in (-1, 5, 2 ** 31 - 1):
        assert L.qr_sensing_bank_set(sbank._h, 2, p(good), bad) == _lib.QR_E_INVALID and b"delay must be in [0, 4]" in L.qr_last_error()
        assert L.qr_sensing_bank_set(sbank._h, 2, None, bad) == _lib.QR_E_INVALID
    assert L.qr_sensing_bank_set(sbank._h, 3, p(good), 0) == _lib.QR_E_INVALID and L.qr_sensing_bank_set(sbank._h, -1, p(good), 0) == _lib.QR_E_INVALID
    sig, delay = np.full(8, 7.0, np.float32), C.c_int32(-9)
    assert L.qr_sensing_bank_read(sbank._h, 2, p(sig), C.byref(delay)) == _lib.QR_E_STATE and b"never set" in L.qr_last_error()
    assert L.qr_sensing_bank_read(sbank._h, 3, p(sig), C.byref(delay)) == _lib.QR_E_INVALID
    assert L.qr_sensing_bank_read(sbank._h, 0, None, C.byref(delay)) == _lib.QR_E_INVALID
    assert bool((sig == 7.0).all()) and delay.value == -9
    refused(_lib.QR_E_STATE, b"slot 2 of the sensing bank was never set", sog=(2, 0))         # none of the refused sets filled slot 2
    sigma, d = sbank.read(0)
    assert np.array_equal(sigma, good) and d == 2
    # qr_sensing_noise
    out = torch.full((K, E, env.state_len), SENTINEL, dtype=torch.float32, device=env.device)

    def noise_refused(code, message, sb=sbank, slot=0, epg=E, k=K, first=0, o=out):
        rc = L.qr_sensing_noise(env._h, sb._h if sb is not None else None, slot, epg, k, 5, first, _ptr(o), env._stream())
        assert rc == code and b"qr_sensing_noise" in L.qr_last_error() and message in L.qr_last_error(), (message, rc, L.qr_last_error())
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
        untouched()

    noise_refused(_lib.QR_E_INVALID, b"null sensing bank", sb=None)
    noise_refused(_lib.QR_E_INVALID, b"out_dev", o=None)
    noise_refused(_lib.QR_E_INVALID, b"envs_per_group", epg=0)
    noise_refused(_lib.QR_E_INVALID, b"num_steps", k=0)
    noise_refused(_lib.QR_E_INVALID, b"num_steps", k=65536)
    noise_refused(_lib.QR_E_INVALID, b"outside the sensing bank", slot=3)
    noise_refused(_lib.QR_E_INVALID, b"outside the sensing bank", slot=-1)
    noise_refused(_lib.QR_E_INVALID, b"must not exceed 2^56", first=LIMIT - K + 1)
    noise_refused(_lib.QR_E_STATE, b"slot 2 of the sensing bank was never set", slot=2)
    # ... and valid calls run, up to the last step the counter holds, and report their time
    rec.zero_(); recf.zero_(); pend.zero_()
    assert _raw(env, pbank, cbank, dbank, sbank, E, (0, 1), (1, 0), (1, 0), (0, 1), K, pend, rec, recf, 0, 5, LIMIT - K) == _lib.QR_OK
    assert _raw(env, pbank, cbank, dbank, sbank, E, (0, 1), (1, 0), (1, 0), (0, 1), K, pend, rec, None, 2, 5, 0) == _lib.QR_OK
    assert L.qr_sensing_noise(env._h, sbank._h, 0, E, K, 5, LIMIT - K, _ptr(out), env._stream()) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((rec[:, 5] == 2 * K).all()) and env.last_rollout_ms() > 0.0 and not bool((out == SENTINEL).any())
    assert bool(pend[:E, :8].any()) and not bool(_bits(pend[E:]).any())
    env.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close()


# ---- 7. Python ----------------------------------------------------------------------------------------------------------------------------------
def test_python_evaluate_sensing_grid_ideal_column_is_evaluate_dynamics_grid():
    """1 policy x 2 conditions x 3 sensors on a 4-group env (two launches, the second padded; two phases, so first_step advances and the
    queues carry over): the ideal sensor's column equals evaluate_dynamics_grid dict for dict under the nominal and under another vehicle;
    noise and delay fly differently."""
    from optimal_quad_control_rl_amd import SensingParams, evaluate_dynamics_grid, evaluate_sensing_grid, physical_sweep
    from optimal_quad_control_rl_amd.dynamics import DynamicsParams
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(5)
    net = ActorCritic(24, 4)
    with torch.no_grad():
        net.pi[-1].bias.copy_(torch.tensor([0.4, 0.4, 0.4, 0.4]))
    E, K, W, seed = 256, 400, 250, 99
    conds = _conditions("e2e")[:2]
    ev = _twin("e2e", 4 * E, 1, conds[0], seed=1)
    sensors = [SensingParams("noisy", *NOISY), SensingParams.ideal(), SensingParams.ideal().with_delay(3)]
    res = evaluate_sensing_grid([net.pi], conds, sensors, ev, envs_per_cell=E, n_eval_steps=K, window_steps=W, seed=seed, noise_seed=7)
    want = evaluate_dynamics_grid([net.pi], conds, [DynamicsParams.nominal(0)], ev, envs_per_cell=E, n_eval_steps=K, window_steps=W, seed=seed)
    assert len(res) == 1 and len(res[0]) == 2 and all(len(r) == 3 for r in res[0])
    for c in range(2):
        assert res[0][c][1] == want[0][c][0], c
        assert res[0][c][0] != res[0][c][1] and res[0][c][2] != res[0][c][1]
    light = physical_sweep(0, "k_w", [0.85])[0]
    res2 = evaluate_sensing_grid([net.pi], conds[:1], sensors[1:2], ev, dynamics=light, envs_per_cell=E, n_eval_steps=K, window_steps=W, seed=seed)
    want2 = evaluate_dynamics_grid([net.pi], conds[:1], [light], ev, envs_per_cell=E, n_eval_steps=K, window_steps=W, seed=seed)
    assert res2[0][0][0] == want2[0][0][0] and res2[0][0][0] != res[0][0][1]
    ev.close()


# ---- 8. time, printed ---------------------------------------------------------------------------------------------------------------------------
def test_sensing_grid_time_is_printed():
    """Median us per step at N = 65 536 = 256 groups x 256 envs, K = 200, E2E + residual MLPs + training disturbances, square track, one
    seeded network in every slot, nominal vehicles: qr_evaluate_policy_sensing_grid with (a) ideal slots, (b) the NOISY sigmas, (c) NOISY
    and d = 4, each paired with qr_evaluate_policy_dynamics_grid on the same handle; the order inside a pair swaps from pair to pair, one
    warm-up pair, medians of 6, times from the handle's event bracket.  NO bound is asserted: the Philox blocks cost real time.
    Measured (one run of this test, us per step, sensing grid vs dynamics grid): f16 ideal 5.963 vs 5.846, ratio 1.020; noise on 8.047 vs
    5.718, 1.407; noise on with d = 4 8.209 vs 5.735, 1.431; f32 29.69 vs 27.54, 1.078; 31.10 vs 26.74, 1.163; 31.19 vs 26.79, 1.164."""
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
    sbank = _sensing_bank([None, _sensor(NOISY, 0), _sensor(NOISY, 4)])
    rec, recf = _records(env)
    pend = _pending(env)
    pol, zero = list(range(P)), [0] * P

    def fly(slot, precision):
        env.seed(99); env.reset_device(); rec.zero_(); recf.zero_(); pend.zero_()
        if slot is None:
            env.evaluate_dynamics_grid_device(pbank, cbank, dbank, pol, zero, pol, E, K, rec, recf, precision=precision)
        else:
            env.evaluate_sensing_grid_device(pbank, cbank, dbank, sbank, pol, zero, pol, [slot] * P, E, K, pend, rec, recf, precision=precision,
                                             noise_seed=3)
        return env.last_rollout_ms() * 1e3 / K

    for precision in ("f16-operands", "f32"):
        for slot, what in ((0, "ideal slots"), (1, "noise on"), (2, "noise on, d = 4")):
            t_sen, t_dyn = [], []
            for rep in range(7):
                if rep % 2:
                    s = fly(slot, precision); d = fly(None, precision)
                else:
                    d = fly(None, precision); s = fly(slot, precision)
                if rep:
                    t_sen.append(s); t_dyn.append(d)
            ms, md = statistics.median(t_sen), statistics.median(t_dyn)
            print("%s, %s: qr_evaluate_policy_sensing_grid median %.4f us/step %s; qr_evaluate_policy_dynamics_grid median %.4f us/step %s; ratio %.4f"
                  % (precision, what, ms, ["%.3f" % t for t in t_sen], md, ["%.3f" % t for t in t_dyn], ms / md))
            assert ms > 0.0 and md > 0.0
    env.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close()
