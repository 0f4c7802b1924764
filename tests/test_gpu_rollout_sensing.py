"""GPU: the closed-loop rollout under OBSERVATION NOISE and COMMAND DELAY (qr_rollout_policy_sensing,
rollout_policy_group_kernel<V, GA, kF32, false, true, RuntimeSensing>, csrc/quadrace_rollout_sensing.hip) and PPO(sensing=...).
Model: include/quadrace.h; the sensor is the sensing-grid evaluator's (tests/sensing_spec.py), keyed by ORDINARY env ids.

1. Ideal slots ARE the dynamics launch (qr_rollout_policy_dynamics, which tests/test_gpu_rollout_dynamics.py pins to the conditions launch and
   that to qr_rollout_policy): every output, terminal rows, last_obs and state bit-equal in all 20 forms, pending all zero bits.
2. The closed loop with noise and delay equals a per-step loop on a twin handle with env_id_base + E, bit for bit (deterministic mode):
       K x [ states_tensor + qr_sensing_noise[k] -> qr_policy_forward -> clamp -> torch-side queue with clear-on-done -> qr_step ]
3. The action noise did not move: log-probs bit-equal to the dynamics launch's, the sample within the bound of tests/test_gpu_action_noise.py.
4. The observation noise is keyed by ordinary ids.   5. K steps in one call equal K calls of one step; last_obs is the next row 0.
6. A group depends on its own triple only.   7. Refusals launch nothing.   8. PPO(sensing=...).   9. Time, printed.
No tolerance anywhere except the one borrowed in 3.  Shapes: groups of 256 or 512 envs, env_id_base = 2^32 - 300 (the low id word wraps
inside a group), first_step = 2^32 - 250 (the low step word wraps inside K), max_steps = 30 and K = 64: every env ends an episode inside K,
which each test asserts on its own outputs."""
import ctypes as C
import statistics
import time

import numpy as np
import pytest
import torch

import action_noise as N
from eval_helpers import SENTINEL, _group_equals, _ptr
from test_gpu_dynamics_grid import _dynamics_bank
from test_gpu_rollout_conditions import GROUND_ROWS, LOG_STD, _bank, _conditions, _force_rows, _handle, _policy, _term_buffer
from test_gpu_sensing_grid import BASE, NOISY, _bits, _pending, _sensing_bank, _sensor

pytestmark = pytest.mark.gpu

NAMES = ("obs", "actions", "log-probs", "rewards", "dones", "truncs", "last_obs")
K, MAX_STEPS, FIRST, SEED = 64, 30, 2 ** 32 - 250, 0xFACE + (3 << 32)


def _short(variant, k=0):
    """the scenario's own condition with a time limit well inside K (every env ends an episode), and a second one on the other track"""
    conds = _conditions(variant)
    return [conds[0].replace(name="short", max_steps=MAX_STEPS), conds[1].replace(name="other short", max_steps=MAX_STEPS - 7)][k]


def _same_state(a, b, what):
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), a.get_state_tensors(), b.get_state_tensors()):
        assert x is None or torch.equal(x, y), (what, name)


def _fly(env, pol, cbank, cog, dbank, sbank, sog, E, k, pend, first=FIRST, det=False, precision="f16-operands", out=None, seed=SEED):
    """the sensing launch over nominal vehicles; the seven tensors, last_obs as a copy (it is the env's own buffer)"""
    o = env.rollout_policy_sensing_device(pol, cbank, cog, dbank, [0] * len(cog), sbank, sog, E, k, LOG_STD, pend, noise_seed=seed, first_step=first,
                                          deterministic=det, out=out, precision=precision)
    return list(o[:6]) + [o[6].clone()]


def _every_env_ended(done, what):
    ends = done.to(torch.int32).sum(0)
    assert int(ends.min()) >= 1, (what, "envs without an episode end", int((ends == 0).sum()))


# ---- 1. ideal slots are the dynamics launch ------------------------------------------------------------------------------------------------
_FORMS = [(v, g, p) for v in ("e2e", "indi") for g in range(5) for p in ("f16-operands", "f32")]


@pytest.mark.parametrize("variant,gates_ahead,precision", _FORMS, ids=["%s-ga%d-%s" % c for c in _FORMS])
def test_ideal_slots_are_the_dynamics_launch(variant, gates_ahead, precision):
    E, cog, sog = 256, [0, 1], [0, 1]                              # slot 0: set from NULL; slot 1: zero sigmas, zero delay
    conds = [_short(variant, 0), _short(variant, 1)]
    a, b = (_handle(variant, 2 * E, gates_ahead, conds[0], env_id_base=BASE) for _ in range(2))
    cbank, pol = _bank(variant, conds), _policy(variant, a.state_len)
    dbank, sbank = _dynamics_bank(variant, [None]), _sensing_bank([None, _sensor()], capacity=3)
    for e in (a, b):
        e.condition_reset(conds, cog, E)
        _force_rows(e, 2)
    ta, tb = _term_buffer(a, K), _term_buffer(b, K)
    pend = _pending(a, fill=SENTINEL)                              # whatever the caller left there: an ideal slot writes zeros
    oa = _fly(a, pol, cbank, cog, dbank, sbank, sog, E, K, pend, precision=precision)
    ob = b.rollout_policy_dynamics_device(pol, cbank, cog, dbank, [0, 0], E, K, LOG_STD, noise_seed=SEED, first_step=FIRST, precision=precision)
    done, trunc = ob[4].bool(), ob[5].bool()
    _every_env_ended(done, "dynamics launch")
    assert int((done & ~trunc).sum()) >= 2 * len(GROUND_ROWS) and int(trunc.sum()) >= 1 and int((ob[3] > 5.0).sum()) >= 1
    for name, x, y in zip(NAMES, oa, ob):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert torch.equal(_bits(oa[0]), _bits(ob[0])) and torch.equal(_bits(oa[6]), _bits(ob[6]))
    assert torch.equal(ta, tb) and int((tb[..., 0] != SENTINEL).sum()) == int(done.sum()) > 0
    _same_state(a, b, "after")
    assert not bool(_bits(pend).any()), "pending"
    a.close(); b.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 2. the closed loop, bit for bit ---------------------------------------------------------------------------------------------------------
def _loop(twin, pol, noise, d, k_steps, precision):
    """K x [obs + noise[k] -> forward -> clamp -> queue -> step] on `twin`: (obs rows, actions, rewards, dones, truncs, terminal rows, the
    last clean observation, the queue in canonical order)"""
    n, L, dev = twin.num_envs, twin.state_len, twin.device
    obs_rows = torch.empty((k_steps, n, L), device=dev)
    act = torch.empty((k_steps, n, 4), device=dev)
    rew = torch.empty((k_steps, n), device=dev)
    dn = torch.empty((k_steps, n), dtype=torch.uint8, device=dev)
    tr = torch.empty((k_steps, n), dtype=torch.uint8, device=dev)
    term = torch.empty((k_steps, n, L), device=dev)
    row = torch.empty((n, L), device=dev)
    twin.set_terminal_obs_buffer(row)
    queue = torch.zeros((n, 16), dtype=torch.float32, device=dev)
    obs = twin.states_tensor
    for k in range(k_steps):
        seen = (obs + noise[k]).contiguous()
        obs_rows[k].copy_(seen)
        mean = pol.forward(seen, precision=precision)
        act[k].copy_(mean)
        cmd = mean.clamp(-1, 1).contiguous()
        if d > 0:
            fly = queue[:, 4 * (d - 1):4 * d].clone()
            queue[:, 4:4 * d] = queue[:, :4 * (d - 1)].clone()
            queue[:, :4] = cmd
        else:
            fly = cmd
        row.fill_(SENTINEL)
        obs, r, dd, t = twin.step_device(fly.contiguous())
        queue[dd.bool()] = 0.0
        rew[k].copy_(r); dn[k].copy_(dd); tr[k].copy_(t); term[k].copy_(row)
    return obs_rows, act, rew, dn, tr, term, obs.clone(), queue


_LOOP = [(v, p, d, E) for v in ("e2e", "indi") for p in ("f16-operands", "f32") for d in (0, 1, 4) for E in (256, 512)]


@pytest.mark.parametrize("variant,precision,d,E", _LOOP, ids=["%s-%s-d%d-E%d" % c for c in _LOOP])
def test_closed_loop_equals_the_per_step_loop(variant, precision, d, E):
    """Group 1 of four flies (NOISY, d) and is held against the loop on a twin with env_id_base + E; groups 0, 2, 3 fly ideal, noise alone
    and delay alone (d, or 1 where d = 0).  All four start from the state of group 1, so that until their first episode end two groups
    differ by their sensor (and the env id of the noise) alone."""
    cond = _short(variant)
    env = _handle(variant, 4 * E, 1, cond, env_id_base=BASE)
    twin = _handle(variant, E, 1, cond, env_id_base=BASE + E)
    cbank, pol, dbank = _bank(variant, [cond]), _policy(variant, env.state_len), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([None, _sensor(NOISY, d), _sensor(NOISY, 0), _sensor(delay=d or 1)])
    env.reset_device()
    _force_rows(env, 4 * E // 256)
    state = [None if t is None else t[E:2 * E] for t in env.get_state_tensors()]
    env.set_state_tensors(*[None if t is None else torch.cat([t] * 4).contiguous() for t in state])
    twin.set_state_tensors(*state)
    twin.update_states()
    tb = _term_buffer(env, K)
    pend = _pending(env)
    out = _fly(env, pol, cbank, [0] * 4, dbank, sbank, [0, 1, 2, 3], E, K, pend, det=True, precision=precision)
    noise = twin.sensing_noise_device(sbank, 1, E, K + 1, noise_seed=SEED, first_step=FIRST)     # ordinary ids: the twin's base is the group's
    obs_rows, act, rew, dn, tr, term, last_clean, queue = _loop(twin, pol, noise, d, K, precision)
    print(variant, precision, "d", d, "E", E, "ends", int(dn.sum()), "crashes", int((dn.bool() & ~tr.bool()).sum()), "time limits", int(tr.sum()),
          "gate passes", int((rew > 5.0).sum()))
    _every_env_ended(dn, "twin")                                                                  # non-vacuity, on the loop's own outputs
    assert int((dn.bool() & ~tr.bool()).sum()) >= 1 and int(tr.sum()) >= 1
    lo, hi = E, 2 * E
    for name, x, y in zip(NAMES[:6], out, (obs_rows, act, None, rew, dn, tr)):
        if y is not None:
            assert torch.equal(x[:, lo:hi], y), (name, int((x[:, lo:hi] != y).sum()))
    assert torch.equal(_bits(out[0][:, lo:hi]), _bits(obs_rows)), "obs rows are the noisy rows"
    assert torch.equal(tb[:, lo:hi], term), "terminal rows: the twin's clean terminal observation"
    assert int((term[..., 0] != SENTINEL).sum()) == int(dn.sum())
    assert torch.equal(_bits(out[6][lo:hi]), _bits(last_clean + noise[K])), "last_obs carries the noise of step K"
    assert not torch.equal(out[6][lo:hi], last_clean)
    _group_equals(env.get_state_tensors(), twin, lo, hi, "state after")
    assert torch.equal(_bits(pend[lo:hi]), _bits(queue)), "pending"
    assert d == 0 or bool(pend[lo:hi, :4 * d].any())
    assert not bool(_bits(pend[:E]).any()) and not bool(_bits(pend[2 * E:3 * E]).any()) and not bool(_bits(pend[:, 4 * max(d, 1):]).any())
    assert bool(pend[3 * E:, :4 * (d or 1)].any())
    # the sensors matter: before their first episode ends, two groups differ where their sensors differ
    done = out[4].to(torch.int32)

    def differ(i, j):
        alive = torch.ones((K, E), dtype=torch.bool, device=env.device)
        for g in (i, j):
            dg = done[:, g * E:(g + 1) * E]
            alive &= (dg.cumsum(0) - dg) == 0
        return bool(((out[3][:, i * E:(i + 1) * E] != out[3][:, j * E:(j + 1) * E]) & alive).any())

    for i, j in ((0, 1), (0, 2), (0, 3), (1, 3), (2, 3)) + (((1, 2),) if d else ()):
        assert differ(i, j), (i, j)
    env.close(); twin.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 3. the action noise did not move -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_the_action_noise_did_not_move(variant):
    from test_gpu_action_noise import CEILING, EPS_TOL, _pair_mask

    E, G = 256, 2
    cond = _short(variant)
    a, b = (_handle(variant, G * E, 1, cond, env_id_base=BASE) for _ in range(2))
    cbank, pol, dbank = _bank(variant, [cond]), _policy(variant, a.state_len), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(NOISY, 2), _sensor(tuple(2 * s for s in NOISY), 4)])
    oa = _fly(a, pol, cbank, [0, 0], dbank, sbank, [0, 1], E, K, _pending(a))
    ob = b.rollout_policy_dynamics_device(pol, cbank, [0, 0], dbank, [0, 0], E, K, LOG_STD, noise_seed=SEED, first_step=FIRST)
    _every_env_ended(oa[4], "sensing launch")
    assert torch.equal(_bits(oa[2]), _bits(ob[2])), "log-probs: a function of eps alone"
    assert not torch.equal(oa[0], ob[0]) and not torch.equal(oa[1], ob[1]) and not torch.equal(oa[3], ob[3])     # ... while the flight differs
    eps64, u = N.action_noise(G * E, K, SEED, env_id_base=BASE, first_step=FIRST)
    std = np.exp(LOG_STD.astype(np.float64)).astype(np.float32)
    worst = 0.0
    for k in range(K):
        mean = pol.forward(oa[0][k].contiguous()).cpu().numpy()                  # the mean of the NOISY row the kernel stored
        act = oa[1][k].cpu().numpy()
        ref = mean.astype(np.float64) + std.astype(np.float64) * eps64[k]
        tol = std * (EPS_TOL * np.maximum(1.0, np.abs(eps64[k])) + np.where(_pair_mask(tuple(x[k:k + 1] for x in u), (1, G * E, 4))[0], CEILING, 0.0)) \
            + 2.0 ** -23 * np.abs(ref)
        err = np.abs(act - ref)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), k
    print(variant, "max |act - (mean + std eps64)| / bound = %.3f" % worst)
    a.close(); b.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 4. noise is keyed by ordinary ids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,gates_ahead", [("e2e", 4), ("indi", 0)])
def test_noise_is_keyed_by_ordinary_ids(variant, gates_ahead):
    E = 256
    cond = _short(variant)
    env = _handle(variant, 2 * E, gates_ahead, cond, env_id_base=BASE)
    cbank, pol, dbank = _bank(variant, [cond]), _policy(variant, env.state_len), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(NOISY, 0)])
    clean = env.reset_device().clone()
    out = _fly(env, pol, cbank, [0, 0], dbank, sbank, [0, 0], E, 1, _pending(env))
    dumps = []
    for g in range(2):
        twin = _handle(variant, E, gates_ahead, cond, env_id_base=BASE + g * E)
        dumps.append(twin.sensing_noise_device(sbank, 0, E, 1, noise_seed=SEED, first_step=FIRST)[0].clone())
        assert torch.equal(_bits(out[0][0, g * E:(g + 1) * E]), _bits(clean[g * E:(g + 1) * E] + dumps[g])), g
        twin.close()
    assert not torch.equal(dumps[0], dumps[1]) and bool((dumps[0] != 0).any(dim=0).all())           # two streams, noise in every column
    assert not torch.equal(_bits(out[0][0, E:]), _bits(clean[E:] + dumps[0]))                       # the group-local id would give group 1 group 0's noise
    env.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 5. continuation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_k_steps_equal_k_launches_of_one_step(variant):
    from optimal_quad_control_rl_amd._closed_loop import rollout_outputs

    E, d, cog, sog = 256, 3, [0, 1, 0], [0, 1, 0]
    conds = [_short(variant, 0), _short(variant, 1)]
    a, b = (_handle(variant, 3 * E, 1, conds[0], env_id_base=BASE) for _ in range(2))
    cbank, pol, dbank = _bank(variant, conds), _policy(variant, a.state_len), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(NOISY, d), _sensor(delay=d)])
    for e in (a, b):
        e.condition_reset(conds, cog, E)
        _force_rows(e, 3)
    ta, tb = _term_buffer(a, K), _term_buffer(b, 1)
    pa, pb = _pending(a), _pending(b)
    oa = _fly(a, pol, cbank, cog, dbank, sbank, sog, E, K, pa)
    ob = rollout_outputs(K, 3 * E, b.state_len, b.device)
    terms, last = [], None
    for k in range(K):
        tb.fill_(SENTINEL)
        step = _fly(b, pol, cbank, cog, dbank, sbank, sog, E, 1, pb, first=FIRST + k, out=tuple(t[k:k + 1] for t in ob))
        terms.append(tb[0].clone())
        if last is not None:
            assert torch.equal(_bits(last), _bits(ob[0][k])), ("last_obs of call %d is row 0 of call %d" % (k - 1, k))
        last = step[6]
    _every_env_ended(oa[4], "one call")
    assert int(oa[5].sum()) >= 1 and bool(pa[:, :4 * d].any()) and not bool(_bits(pa[:, 4 * d:]).any())
    for name, x, y in zip(NAMES[:6], oa, ob):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert torch.equal(_bits(oa[6]), _bits(last)), "last_obs"
    assert torch.equal(ta, torch.stack(terms)), "terminal rows"
    _same_state(a, b, "K launches")
    assert torch.equal(_bits(pa), _bits(pb)), "pending"
    a.close(); b.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 6. a group depends on its own triple only -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_a_group_equals_its_one_group_twin(variant):
    from test_gpu_dynamics_grid import _vehicles

    E, G, cog, dog, sog = 256, 4, [1, 0, 1, 0], [1, 0, 0, 1], [2, 1, 0, 2]      # permuted maps with repeats
    conds, vehicles = [_short(variant, 0), _short(variant, 1)], _vehicles(variant, 2)
    sensors = [_sensor(NOISY, 2), _sensor(delay=4), _sensor(tuple(2 * s for s in NOISY), 0)]
    env = _handle(variant, G * E, 1, conds[0], env_id_base=BASE)
    cbank, pol = _bank(variant, conds), _policy(variant, env.state_len)
    dbank, sbank = _dynamics_bank(variant, vehicles), _sensing_bank(sensors)
    env.condition_reset(conds, cog, E)
    start = env.get_state_tensors()
    _force_rows(env, G)
    tb = _term_buffer(env, K)
    rng = np.random.default_rng(1)
    fill = torch.as_tensor(rng.uniform(-1, 1, (G * E, 16)).astype(np.float32), device=env.device)     # a queue in flight; entries behind d are dropped
    pend = fill.clone()
    kw = dict(noise_seed=SEED, first_step=FIRST)
    out = [t.clone() for t in env.rollout_policy_sensing_device(pol, cbank, cog, dbank, dog, sbank, sog, E, K, LOG_STD, pend, **kw)]
    after = env.get_state_tensors()
    for g in range(G):
        lo, hi = g * E, (g + 1) * E
        twin = _handle(variant, E, 1, conds[cog[g]], env_id_base=BASE + lo)
        _group_equals(start, twin, lo, hi, "start, group %d" % g)
        _force_rows(twin, 1)
        ttb = _term_buffer(twin, K)
        tp = fill[lo:hi].clone()
        tout = twin.rollout_policy_sensing_device(pol, cbank, [cog[g]], dbank, [dog[g]], sbank, [sog[g]], E, K, LOG_STD, tp, **kw)
        _every_env_ended(tout[4], "twin %d" % g)
        for name, x, y in zip(NAMES[:6], out, tout):
            assert torch.equal(x[:, lo:hi], y), (name, g, int((x[:, lo:hi] != y).sum()))
        assert torch.equal(_bits(out[6][lo:hi]), _bits(tout[6])), ("last_obs", g)
        assert torch.equal(tb[:, lo:hi], ttb) and int((ttb[..., 0] != SENTINEL).sum()) == int(tout[4].sum()), ("terminal-observation rows", g)
        _group_equals(after, twin, lo, hi, "state after, group %d" % g)
        assert torch.equal(_bits(pend[lo:hi]), _bits(tp)), ("pending", g)
        dl = sensors[sog[g]].delay_steps
        assert not bool(_bits(tp[:, 4 * dl:]).any()) and (dl == 0 or bool(tp[:, :4 * dl].any())), ("queue behind d", g)
        twin.close()
    env.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.sensing import SensingBank
    from test_gpu_dynamics_grid import _vehicles

    E, Kr = 256, 8
    n = 2 * E
    conds = _conditions("indi")
    env = _handle("indi", n, 1, conds[0])
    L = env._L
    pol = _policy("indi", env.state_len)
    cbank = _bank("indi", conds[:2], capacity=3)                                      # slots 0, 1 set, slot 2 never set
    dbank = _dynamics_bank("indi", _vehicles("indi", 2), capacity=3)                  # likewise
    sbank = _sensing_bank([_sensor(NOISY, 2), _sensor(delay=1)], capacity=3)          # likewise
    dev = env.device
    bufs = dict(obs=torch.full((Kr, n, env.state_len), SENTINEL, device=dev), act=torch.full((Kr, n, 4), SENTINEL, device=dev),
                logp=torch.full((Kr, n), SENTINEL, device=dev), rew=torch.full((Kr, n), SENTINEL, device=dev),
                done=torch.full((Kr, n), 7, dtype=torch.uint8, device=dev), trunc=torch.full((Kr, n), 7, dtype=torch.uint8, device=dev),
                last=torch.full((n, env.state_len), SENTINEL, device=dev), pend=torch.full((n, 16), SENTINEL, device=dev))
    before = env.get_state_tensors()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    SKIP = object()

    def call(p=pol, cb=cbank, db=dbank, sb=sbank, g=2, epg=E, cog=(1, 0), dog=(0, 1), sog=(1, 0), k=Kr, ls=LOG_STD, flags=0, first=0, misalign=False,
             **null):
        ca, da, sa = (None if m is None else np.asarray(m, np.int32) for m in (cog, dog, sog))
        b = {name: (None if null.get(name, SKIP) is None else t) for name, t in bufs.items()}
        h = lambda x: x._h if x is not None else None
        ip = lambda x: None if x is None else x.ctypes.data_as(i32p)
        pend = C.c_void_p(b["pend"].data_ptr() + 4) if misalign else _ptr(b["pend"])
        return L.qr_rollout_policy_sensing(env._h, h(p), h(cb), h(db), h(sb), g, epg, ip(ca), ip(da), ip(sa), k, None if ls is None else ls.ctypes.data_as(f32p),
                                           3, first, flags, pend, _ptr(b["obs"]), _ptr(b["act"]), _ptr(b["logp"]), _ptr(b["rew"]), _ptr(b["done"]),
                                           _ptr(b["trunc"]), _ptr(b["last"]), env._stream())

    def untouched():
        torch.cuda.synchronize()
        for name, t in bufs.items():
            assert bool((t == (7 if t.dtype == torch.uint8 else SENTINEL)).all()), name
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    def refused(code, message, **kw):
        rc = call(**kw)
        err = L.qr_last_error()
        assert rc == code, (list(kw.keys()), rc, err)
        assert b"qr_rollout_policy_sensing" in err and message in err, err
        untouched()

    # 1. one of each class qr_rollout_policy_dynamics refuses, in its order, each paired with a bad sensing argument to show the order
    refused(_lib.QR_E_INVALID, b"bad argument", k=0, sb=None)
    refused(_lib.QR_E_INVALID, b"", p=None, sb=None)
    refused(_lib.QR_E_INVALID, b"", obs=None, sog=None)
    refused(_lib.QR_E_INVALID, b"QR_ROLLOUT_DETERMINISTIC", flags=4, sb=None)
    empty = MfmaPolicy(env.state_len)
    refused(_lib.QR_E_STATE, b"", p=empty, sb=None)                                   # a policy without weights
    empty.close()
    env.pause = True
    refused(_lib.QR_E_STATE, b"", sb=None)
    env.pause = False
    refused(_lib.QR_E_INVALID, b"null condition bank", cb=None, db=None, sb=None)
    refused(_lib.QR_E_INVALID, b"condition map", cog=None, dog=None, sog=None)
    refused(_lib.QR_E_INVALID, b"multiple of 256", epg=128, g=4, cog=(0, 1, 0, 1), dog=(0, 1, 0, 9), sog=(0, 1, 0, 9))
    refused(_lib.QR_E_INVALID, b"must equal the env count", g=1, cog=(0,), dog=(5,), sog=(5,))
    refused(_lib.QR_E_INVALID, b"condition_of_group[0] is outside", cog=(3, 0), dog=(3, 0), sog=(3, 0))
    refused(_lib.QR_E_STATE, b"condition bank was never set", cog=(2, 0), dog=(2, 0), sog=(2, 0))
    refused(_lib.QR_E_INVALID, b"null dynamics bank", db=None, sb=None)
    refused(_lib.QR_E_INVALID, b"dynamics map", dog=None, sog=None)
    other = _dynamics_bank("e2e", [None, None])
    refused(_lib.QR_E_INVALID, b"dynamics bank of another variant", db=other, sb=None)
    other.close()
    refused(_lib.QR_E_INVALID, b"dynamics_of_group[1] is outside the dynamics bank", dog=(0, 3), sog=(0, 3))
    refused(_lib.QR_E_STATE, b"slot 2 of the dynamics bank was never set", dog=(2, 0), sog=(2, 0))
    # 2. the sensing bank's own, in the words of qr_evaluate_policy_sensing_grid, each ahead of a NULL pending_dev
    refused(_lib.QR_E_INVALID, b"null sensing bank", sb=None, pend=None)
    refused(_lib.QR_E_INVALID, b"sensing_of_group is required", sog=None, pend=None)
    refused(_lib.QR_E_INVALID, b"sensing_of_group[0] is outside the sensing bank", sog=(3, 0), pend=None)
    refused(_lib.QR_E_INVALID, b"sensing_of_group[1] is outside the sensing bank", sog=(0, -1), pend=None)
    refused(_lib.QR_E_INVALID, b"sensing_of_group[1] is outside the sensing bank", sog=(0, 2 ** 31 - 1), pend=None)
    refused(_lib.QR_E_INVALID, b"2^56", first=2 ** 56 - Kr, pend=None)               # last_obs would draw step 2^56
    refused(_lib.QR_E_INVALID, b"2^56", first=2 ** 64 - 1, sog=(2, 0))
    refused(_lib.QR_E_STATE, b"slot 2 of the sensing bank was never set", sog=(2, 0), pend=None)
    if torch.cuda.device_count() > 1:
        far = SensingBank(2, device=1)
        far.set(0); far.set(1)
        torch.cuda.set_device(0)
        refused(_lib.QR_E_INVALID, b"sensing bank on another GPU", sb=far, pend=None)
        far.close()
    # 3. pending_dev
    refused(_lib.QR_E_INVALID, b"pending_dev is required", pend=None)
    refused(_lib.QR_E_INVALID, b"16-byte aligned", misalign=True)
    # 4. new maps while the stream is being captured: the pair, or the sensing map alone
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        assert call(sog=(0, 1)) == _lib.QR_OK                                         # these maps are on the device now
        for t in bufs.values():
            t.fill_(7 if t.dtype == torch.uint8 else SENTINEL)
        env.set_state_tensors(*before)
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin()
        rc_sen = call(sog=(1, 1))
        err_sen = L.qr_last_error()
        rc_dyn = call(sog=(0, 1), dog=(1, 1))
        err_dyn = L.qr_last_error()
        graph.capture_end()
    assert rc_sen == _lib.QR_E_STATE and b"capture" in err_sen and b"qr_rollout_policy_sensing" in err_sen
    assert rc_dyn == _lib.QR_E_STATE and b"capture" in err_dyn
    untouched()
    # ... and a valid call runs, writes every row and the queue, and reports its time; the trunc buffer and last_obs are optional
    bufs["pend"].zero_()                                                              # (a queue of sentinels would be flown as commands)
    assert call(trunc=None, last=None) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((bufs["obs"] != SENTINEL).all()) and bool((bufs["done"] <= 1).all()) and bool((bufs["trunc"] == 7).all())
    assert bool((bufs["last"] == SENTINEL).all()) and env.last_rollout_ms() > 0.0
    pend = bufs["pend"]                                                               # group 0: slot 1, d = 1; group 1: slot 0, d = 2
    assert bool(pend[:E, :4].any()) and bool(pend[E:, 4:8].any()) and not bool(_bits(pend[:E, 4:]).any()) and not bool(_bits(pend[:, 8:]).any())
    env.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 8. PPO ---------------------------------------------------------------------------------------------------------------------------------
def _ppo_env(n, seed=21):
    cond = _conditions("e2e")[0].replace(max_steps=MAX_STEPS)
    return _handle("e2e", n, 1, cond, seed=seed)


def _theta(model):
    return torch.cat([p.detach().reshape(-1) for p in model.policy.parameters()])


def test_ppo_under_the_ideal_sensor_is_the_plain_fused_ppo():
    from optimal_quad_control_rl_amd.ppo import PPO
    from optimal_quad_control_rl_amd.sensing import SensingParams

    T, n = 16, 768
    kw = dict(n_steps=T, seed=4, fused_collect=True, native_update=True)
    ea, eb = _ppo_env(n), _ppo_env(n)
    plain = PPO(ea, **kw)
    keys = set(plain.state_dict().keys())
    assert "sensing" not in keys and "per_sensor" not in plain.stats and plain._pending is None       # without `sensing`: the keys of always
    mixed = PPO(eb, sensing=[SensingParams.ideal()], **kw)
    assert mixed.sensing_of_group == [0, 0, 0] and set(mixed.state_dict().keys()) == keys | {"sensing"}
    calls = []
    launch = eb.rollout_policy_sensing_device
    eb.rollout_policy_sensing_device = lambda *a, **k: (calls.append("sensing"), launch(*a, **k))[1]
    running = torch.zeros(n, dtype=torch.float64, device=ea.device)          # the running episode returns, restated in float64
    for _ in range(2):
        for m in (plain, mixed):
            m.collect(); m.train()
        assert torch.equal(_bits(plain.buf_rew), _bits(mixed.buf_rew)) and torch.equal(plain.buf_done, mixed.buf_done)
        abs_sum = 0.0                                                        # sum of |return| over the episodes that ended in this round
        for k in range(T):
            running += plain.buf_rew[k].double()
            d = plain.buf_done[k].double()
            abs_sum += float((running.abs() * d).sum())
            running *= 1.0 - d
    assert calls == ["sensing", "sensing"] and int(mixed._done_u8.sum()) >= 1
    assert torch.equal(plain.buf_rew, mixed.buf_rew) and torch.equal(_bits(plain.buf_obs), _bits(mixed.buf_obs))
    assert torch.equal(_bits(_theta(plain)), _bits(_theta(mixed))), "theta"
    assert torch.equal(_bits(plain._updater.m), _bits(mixed._updater.m)) and torch.equal(_bits(plain._updater.v), _bits(mixed._updater.v)), "Adam moments"
    assert int(plain._updater.step) == int(mixed._updater.step)
    # stats: every entry equal as printed, except ep_rew_mean, which the GAE kernel sums with ONE FLOAT ATOMIC PER WAVE (ppo_gae_kernel:
    # per-lane and per-wave sums in a fixed order, then n / 64 atomic adds in whatever order the waves arrive), so that two runs of the
    # same trainer on the same buffers may differ in its last bits.  Two orders of W float32 terms x_w differ by at most
    # 2 (W - 1) 2^-24 sum |x_w| to first order, and sum |x_w| <= the sum of |return| over the ended episodes (restated above in float64);
    # 1.01 covers the higher orders and the float32 rounding of the returns themselves.  ep_len_mean, gates and episodes are sums of small
    # integers, exact in any order.
    assert set(mixed.stats) == set(plain.stats) | {"per_sensor"}
    exact = [k for k in plain.stats if k != "ep_rew_mean"]
    assert repr({k: mixed.stats[k] for k in exact}) == repr({k: plain.stats[k] for k in exact})
    bound = 1.01 * 2 * (n // 64 - 1) * 2.0 ** -24 * abs_sum / plain.stats["episodes"]
    diff = abs(mixed.stats["ep_rew_mean"] - plain.stats["ep_rew_mean"])
    print("ep_rew_mean %.9g against %.9g: |difference| %.3e, bound of the atomic sum's order %.3e" % (mixed.stats["ep_rew_mean"], plain.stats["ep_rew_mean"],
                                                                                                  diff, bound))
    assert diff <= bound and plain.stats["episodes"] == mixed.stats["episodes"] == float(plain.buf_done.sum())
    assert [s["name"] for s in mixed.stats["per_sensor"]] == ["ideal"] and mixed.stats["per_sensor"][0]["episodes"] == int(mixed._done_u8.sum())
    assert not bool(_bits(mixed._pending).any())
    ea.close(); eb.close()


def test_ppo_under_a_mix_of_sensors_resumes_bit_for_bit():
    from optimal_quad_control_rl_amd.ppo import PPO
    from optimal_quad_control_rl_amd.sensing import SensingParams

    n, T, E = 1024, 16, 256
    sensors = [SensingParams.from_sigma(NOISY, 2, name="noisy d=2"), SensingParams.ideal()]
    kw = dict(n_steps=T, seed=4, fused_collect=True, native_update=True, sensing=sensors)

    def round_(m):
        m.collect(); m.train()
        done, trunc = m._done_u8.bool(), m._trunc_u8.bool()
        ps = m.stats["per_sensor"]
        assert [s["name"] for s in ps] == ["noisy d=2", "ideal"]                            # one entry per sensor
        assert sum(s["episodes"] for s in ps) == int(done.sum())
        assert sum(s["crashes"] for s in ps) == int((done & ~trunc).sum()) and sum(s["time_limits"] for s in ps) == int((done & trunc).sum())
        noisy = torch.cat([done[:, g * E:(g + 1) * E] for g in (0, 2)], 1)
        assert ps[0]["episodes"] == int(noisy.sum())
        return int(done.sum())

    ea, eb, ec = _ppo_env(n), _ppo_env(n), _ppo_env(n)
    whole, first = PPO(ea, **kw), PPO(eb, **kw)
    assert whole.sensing_of_group == [0, 1, 0, 1]
    _force_rows(ea, n // E); _force_rows(eb, n // E)                                        # episodes that end inside the first rollout
    ended = [round_(whole) for _ in range(3)]
    assert ended[0] >= len(GROUND_ROWS) * (n // E) and sum(ended[1:]) >= n                  # the time limit of 30 falls inside rounds 2 and 3
    round_(first); round_(first)
    sd, params = first.state_dict(), {k: v.clone() for k, v in first.policy.state_dict().items()}
    saved = sd["sensing"]["pending"]
    assert saved.shape == (n, 16) and bool(saved[:E, :8].any()) and not bool(saved[:, 8:].any()) and not bool(saved[E:2 * E].any())
    assert sd["sensing"]["sensing_of_group"] == [0, 1, 0, 1] and len(sd["sensing"]["slots"]) == 2
    resumed = PPO(ec, **{**kw, "sensing": [SensingParams.ideal()]})                         # the checkpoint's sensors win
    resumed.policy.load_state_dict(params)
    resumed.load_state_dict(sd)
    assert resumed.sensing == sensors and torch.equal(_bits(resumed._pending.cpu()), _bits(saved))
    round_(resumed)
    assert torch.equal(_bits(_theta(whole)), _bits(_theta(resumed))) and torch.equal(whole.buf_rew, resumed.buf_rew)
    assert torch.equal(_bits(whole.buf_obs), _bits(resumed.buf_obs)) and torch.equal(_bits(whole._pending), _bits(resumed._pending))
    assert torch.equal(_bits(whole._updater.m), _bits(resumed._updater.m)) and torch.equal(_bits(whole._updater.v), _bits(resumed._updater.v))
    assert repr(whole.stats["per_sensor"]) == repr(resumed.stats["per_sensor"])
    for e in (ea, eb, ec):
        e.close()


# ---- 9. time, printed ------------------------------------------------------------------------------------------------------------------------
def test_sensing_launch_time_is_printed():
    """Median us per step of qr_rollout_policy_sensing -- ideal slots, the NOISY sigmas, NOISY + d = 4 -- each against
    qr_rollout_policy_dynamics on the same handle: N = 65 536 = 256 groups x 256 envs, K = 200, E2E + residual MLPs + training disturbances,
    square track, nominal vehicles, every group on the condition that equals the handle's configuration.  Launches alternate from the same
    seeded reset in ORDER-SWAPPED pairs (sensing first in even repetitions, dynamics first in odd ones), one warm-up pair, medians of 6, host
    clock around a stream synchronise.  NO bound is asserted: nobody had measured this kernel when the test was written (DESIGN.md section 8
    and profiles/rollout_sensing_time.txt hold the numbers of one run)."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd._closed_loop import rollout_outputs
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    n, Kc, E = 65536, 200, 256
    groups = n // E
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=99)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    cbank = _bank("e2e", [Condition.from_env(env)])
    dbank = _dynamics_bank("e2e", [None])
    sbank = _sensing_bank([None, _sensor(NOISY, 0), _sensor(NOISY, 4)])
    torch.manual_seed(0)
    pol = MfmaPolicy(env.state_len).load_torch(ActorCritic(env.state_len, 4).pi)
    out = rollout_outputs(Kc, n, env.state_len, env.device)
    pend = _pending(env)
    log_std, zero = np.zeros(4, np.float32), [0] * groups
    stream = torch.cuda.current_stream(env.device)

    def timed(launch):
        env.seed(99); env.reset_device()
        pend.zero_()
        stream.synchronize()
        t0 = time.perf_counter()
        launch()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / Kc

    for precision in ("f16-operands", "f32"):
        for label, slot in (("ideal slots", 0), ("noise on", 1), ("noise on, d = 4", 2)):
            sen = lambda: env.rollout_policy_sensing_device(pol, cbank, zero, dbank, zero, sbank, [slot] * groups, E, Kc, log_std, pend, noise_seed=1, out=out,
                                                            precision=precision)
            dyn = lambda: env.rollout_policy_dynamics_device(pol, cbank, zero, dbank, zero, E, Kc, log_std, noise_seed=1, out=out, precision=precision)
            t_sen, t_dyn = [], []
            for rep in range(7):
                if rep % 2 == 0:
                    s = timed(sen); d = timed(dyn)
                else:
                    d = timed(dyn); s = timed(sen)
                if rep:
                    t_sen.append(s); t_dyn.append(d)
            ms, md = statistics.median(t_sen), statistics.median(t_dyn)
            print("%s, %s: qr_rollout_policy_sensing median %.4f us/step %s; qr_rollout_policy_dynamics median %.4f us/step %s; ratio %.4f"
                  % (precision, label, ms, ["%.3f" % t for t in t_sen], md, ["%.3f" % t for t in t_dyn], ms / md))
            assert ms > 0.0 and md > 0.0
    env.close(); cbank.close(); dbank.close(); sbank.close(); pol.close()
