"""GPU: the COMMAND HISTORY in the policy's row -- qr_rollout_policy_history (rollout_policy_group_kernel<V, GA, kF32, false, true,
RuntimeSensing, H>, csrc/quadrace_rollout_history.hip), qr_evaluate_policy_history_grid (eval_policy_history_grid_kernel<V, GA, H, kF32>,
csrc/quadrace_eval_history.hip) and PPO(command_history=...).  Model: include/quadrace.h, restated in tests/command_history_spec.py.

1. The rollout equals a per-step loop on a twin handle with env_id_base + E, bit for bit (deterministic mode), in every (GA, H) form:
       K x [ row(states_tensor + qr_sensing_noise[k], queue, H) -> qr_policy_forward (L + 4 H inputs) -> clamp -> push -> qr_step -> clear ]
2. A policy whose first layer ignores the 4 H history inputs flies what qr_rollout_policy_sensing flies with the L-input policy.
3. K steps in one call equal K calls of one step.   4. The evaluator equals the per-step loop; permuting the groups permutes the records.
5. A rollout hands its queue to an evaluation.   6. Refusals launch nothing.   7. PPO(command_history=2).   8. Time, printed.
Every comparison is bit for bit.  Shapes: four groups of 256 envs, env_id_base = 2^32 - 300, first_step just below 2^32 (the low step word
wraps inside K), rollouts with max_steps = 30 and K = 64, evaluations with the scenario's condition and its 600 steps: every env ends an
episode inside the window, which each test asserts on its own outputs."""
import ctypes as C
import statistics
import time

import numpy as np
import pytest
import torch

import command_history_spec as CH
import eval_spec as S
from eval_helpers import SENTINEL, _closed_loop_layers, _group_equals, _policy_bank, _ptr, _records
from test_gpu_dynamics_grid import _dynamics_bank
from test_gpu_evaluate import _target
from test_gpu_rollout_conditions import GROUND_ROWS, LOG_STD, _bank, _conditions, _force_rows, _handle, _policy, _term_buffer
from test_gpu_rollout_sensing import MAX_STEPS, NAMES, SEED, _every_env_ended, _same_state, _short
from test_gpu_sensing_grid import BASE, NOISY, _based_twin, _bits, _condition_bank, _pending, _sensing_bank, _sensor
from test_gpu_sensing_grid import _conditions as _eval_conditions

pytestmark = pytest.mark.gpu

SC = S.SCENARIO
E, K, FIRST = 256, 64, 2 ** 32 - 20
PAIRS = [(ga, h) for ga in range(5) for h in range(1, 5 - ga)]                       # the 10 (GA, H) with GA + H <= 4
# one delay per pair: d < H, d = H and d > H all occur (for both variants: the table does not depend on the variant)
DELAY = {(0, 1): 0, (0, 2): 1, (0, 3): 4, (0, 4): 4, (1, 1): 1, (1, 2): 4, (1, 3): 0, (2, 1): 4, (2, 2): 1, (3, 1): 1}
assert sorted(DELAY) == PAIRS and {(d > h) - (d < h) for (_, h), d in DELAY.items()} == {-1, 0, 1} and set(DELAY.values()) == {0, 1, 4}


def _wide_term_buffer(env, rows, width):
    tb = torch.full((rows, env.num_envs, width), SENTINEL, device=env.device)
    env.set_terminal_obs_buffer(tb, obs_len=width)
    return tb


def _fly(env, pol, cbank, cog, dbank, sbank, sog, H, k, pend, first=FIRST, det=False, precision="f16-operands", out=None, seed=SEED):
    """the history launch over nominal vehicles; the seven tensors, last_obs as a copy (it is a buffer the env reuses)"""
    o = env.rollout_policy_history_device(pol, cbank, cog, dbank, [0] * len(cog), sbank, sog, H, E, k, LOG_STD, pend, noise_seed=seed, first_step=first,
                                          deterministic=det, out=out, precision=precision)
    return list(o[:6]) + [o[6].clone()]


def _loop(twin, pol, noise, d, H, steps, precision, queue=None, targets=False):
    """steps x [row(obs + noise[k], queue, H) -> forward -> clamp -> push -> step -> clear] on `twin`, from tests/command_history_spec.py.
    Returns a dict: the rows the policy saw, the unclipped means, rewards, dones, truncs, the terminal rows at width L + 4 H (SENTINEL where
    no episode ended), the last clean observation, the queue, and with `targets` the target before / after every step."""
    n, L, dev = twin.num_envs, twin.state_len, twin.device
    W = L + 4 * H
    r = dict(obs=torch.empty((steps, n, W), device=dev), act=torch.empty((steps, n, 4), device=dev), rew=torch.empty((steps, n), device=dev),
             done=torch.empty((steps, n), dtype=torch.uint8, device=dev), trunc=torch.empty((steps, n), dtype=torch.uint8, device=dev),
             term=torch.full((steps, n, W), SENTINEL, device=dev))
    if targets:
        r["before"] = torch.empty((steps, n), dtype=torch.int32, device=dev)
        r["after"] = torch.empty((steps, n), dtype=torch.int32, device=dev)
        prev = torch.empty(n, dtype=torch.int32, device=dev)
        _target(twin, prev)
    row = torch.empty((n, L), device=dev)
    twin.set_terminal_obs_buffer(row)
    queue = torch.zeros((n, 16), dtype=torch.float32, device=dev) if queue is None else queue.clone()
    obs = twin.states_tensor
    for k in range(steps):
        seen = CH.row(obs if noise is None else obs + noise[k], queue, H).contiguous()
        r["obs"][k].copy_(seen)
        mean = pol.forward(seen, precision=precision)
        r["act"][k].copy_(mean)
        fly, queue = CH.push(queue, mean.clamp(-1, 1), d, H)
        row.fill_(SENTINEL)
        obs, rew, dd, t = twin.step_device(fly.contiguous())
        ended = dd.bool()
        r["term"][k][ended] = CH.terminal_row(row, queue, H)[ended]
        queue = CH.clear(queue, dd)
        r["rew"][k].copy_(rew); r["done"][k].copy_(dd); r["trunc"][k].copy_(t)
        if targets:
            r["before"][k].copy_(prev)
            _target(twin, r["after"][k])
            prev = r["after"][k]
    twin.set_terminal_obs_buffer(None)
    r["last_clean"], r["queue"] = obs.clone(), queue
    return r


def _tail_is_a_history(obs, done, L, what):
    """the history columns of rollout rows [K, n, L + 4 H]: zero at step 0 (the queue was zero) and in the step behind each episode end,
    non-zero somewhere afterwards"""
    tail = obs[..., L:]
    assert not bool(_bits(tail[0]).any()), (what, "step 0")
    after_end = done[:-1].bool()
    assert int(after_end.sum()) >= 1 and not bool(_bits(tail[1:][after_end]).any()), (what, "the step behind an episode end")
    assert bool(tail[1:].any()), (what, "the history is never non-zero")


# ---- 1. the rollout, bit for bit -------------------------------------------------------------------------------------------------------------
_ROLLOUT = [(v, ga, h, "f16-operands") for v in ("e2e", "indi") for ga, h in PAIRS] + \
           [(v, ga, h, "f32") for v in ("e2e", "indi") for ga, h in ((0, 4), (3, 1), (1, 2))]


@pytest.mark.parametrize("variant,ga,H,precision", _ROLLOUT, ids=["%s-ga%d-h%d-%s" % c for c in _ROLLOUT])
def test_rollout_equals_the_per_step_loop(variant, ga, H, precision):
    """Group 1 of four flies (NOISY, d) and is held against the loop on a twin with env_id_base + E; groups 0, 2, 3 fly ideal, noise alone
    and delay alone.  All four start from the state of group 1."""
    d = DELAY[(ga, H)]
    cond = _short(variant)
    env = _handle(variant, 4 * E, ga, cond, env_id_base=BASE)
    twin = _handle(variant, E, ga, cond, env_id_base=BASE + E)
    L = env.state_len
    W = L + 4 * H
    assert W == CH.obs_len(0 if variant == "e2e" else 1, ga + H)
    cbank, pol, dbank = _bank(variant, [cond]), _policy(variant, W), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([None, _sensor(NOISY, d), _sensor(NOISY, 0), _sensor(delay=d or 1)])
    env.reset_device()
    _force_rows(env, 4)
    state = [None if t is None else t[E:2 * E] for t in env.get_state_tensors()]
    env.set_state_tensors(*[None if t is None else torch.cat([t] * 4).contiguous() for t in state])
    twin.set_state_tensors(*state)
    twin.update_states()
    tb = _wide_term_buffer(env, K, W)
    pend = _pending(env)
    out = _fly(env, pol, cbank, [0] * 4, dbank, sbank, [0, 1, 2, 3], H, K, pend, det=True, precision=precision)
    noise = twin.sensing_noise_device(sbank, 1, E, K + 1, noise_seed=SEED, first_step=FIRST)     # ordinary ids: the twin's base is the group's
    assert tuple(noise.shape) == (K + 1, E, L), "qr_sensing_noise is unchanged: rows of the env's own length"
    ref = _loop(twin, pol, noise, d, H, K, precision)
    dn, tr = ref["done"].bool(), ref["trunc"].bool()
    print(variant, "ga", ga, "H", H, "d", d, precision, "ends", int(dn.sum()), "crashes", int((dn & ~tr).sum()), "time limits", int(tr.sum()),
          "gate passes", int((ref["rew"] > 5.0).sum()))
    _every_env_ended(ref["done"], "twin")                                                         # non-vacuity, on the loop's own outputs
    assert int((dn & ~tr).sum()) >= 1 and int(tr.sum()) >= 1
    lo, hi = E, 2 * E
    assert tuple(out[0].shape) == (K, 4 * E, W) and tuple(out[6].shape) == (4 * E, W)
    for name, x, y in zip(NAMES[:6], out, (ref["obs"], ref["act"], None, ref["rew"], ref["done"], ref["trunc"])):
        if y is not None:
            assert torch.equal(x[:, lo:hi], y), (name, int((x[:, lo:hi] != y).sum()))
    assert torch.equal(_bits(out[0][:, lo:hi]), _bits(ref["obs"])), "obs rows: all L + 4 H columns"
    assert torch.equal(_bits(tb[:, lo:hi]), _bits(ref["term"])), "terminal rows: [clean terminal observation | u_k, ..., u_{k-H+1}], sentinels elsewhere"
    assert int((ref["term"][..., 0] != SENTINEL).sum()) == int(dn.sum()) and bool((ref["term"][..., L:][dn] != SENTINEL).all())
    assert bool(ref["term"][..., L:L + 4][dn].any()), "the terminal rows carry the command of the step that ended the episode"
    last = CH.row(ref["last_clean"] + noise[K], ref["queue"], H)
    assert torch.equal(_bits(out[6][lo:hi]), _bits(last)), "last_obs: the noise of step K on the first L entries, the exact history behind"
    assert not torch.equal(out[6][lo:hi, :L], ref["last_clean"])
    _group_equals(env.get_state_tensors(), twin, lo, hi, "state after")
    assert torch.equal(_bits(pend[lo:hi]), _bits(ref["queue"])), "pending"
    for g, dg in enumerate((0, d, 0, d or 1)):                                                    # max(d, H) entries per group, zeros behind
        m = max(dg, H)
        assert bool(pend[g * E:(g + 1) * E, 4 * (m - 1):4 * m].any()) and not bool(_bits(pend[g * E:(g + 1) * E, 4 * m:]).any()), g
        _tail_is_a_history(out[0][:, g * E:(g + 1) * E], out[4][:, g * E:(g + 1) * E], L, "group %d" % g)
    alive = ~dn[0]                                                                                # row 1 carries u_0 wherever step 0 did not end the episode
    assert int(alive.sum()) >= 1 and torch.equal(ref["obs"][1, :, L:L + 4][alive], ref["act"][0].clamp(-1, 1)[alive])
    env.close(); twin.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 2. a policy that ignores its history flies the sensing launch -----------------------------------------------------------------------------
_IGNORE = [(v, ga, h, p) for v in ("e2e", "indi") for ga, h in ((1, 2), (0, 4)) for p in ("f16-operands", "f32")]


@pytest.mark.parametrize("variant,ga,H,precision", _IGNORE, ids=["%s-ga%d-h%d-%s" % c for c in _IGNORE])
def test_a_policy_that_ignores_its_history_flies_the_sensing_launch(variant, ga, H, precision):
    """The first-layer weights on the 4 H history inputs are zero, every other weight is the L-input policy's: the extra products are exact
    zeros and the non-zero terms keep their order, so the two launches agree bit for bit (sampling on: the noise streams are the same)."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    cond = _short(variant)
    a, b = (_handle(variant, 4 * E, ga, cond, env_id_base=BASE) for _ in range(2))
    L = a.state_len
    W = L + 4 * H
    layers = _closed_loop_layers(L, np.asarray(SC[variant + "_action"], np.float32), seed=3)
    wide = [(torch.cat([layers[0][0], torch.zeros((layers[0][0].shape[0], 4 * H))], dim=1).contiguous(), layers[0][1])] + layers[1:]
    narrow_pol, wide_pol = MfmaPolicy(L).set_weights(layers), MfmaPolicy(W).set_weights(wide)
    cbank, dbank = _bank(variant, [cond]), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([None, _sensor(NOISY, 2), _sensor(NOISY, 0), _sensor(delay=4)])
    sog = [0, 1, 2, 3]
    for e in (a, b):
        _force_rows(e, 4)
    ta, tb = _wide_term_buffer(a, K, W), _term_buffer(b, K)
    pa, pb = _pending(a), _pending(b)
    oa = _fly(a, wide_pol, cbank, [0] * 4, dbank, sbank, sog, H, K, pa, precision=precision)
    ob = b.rollout_policy_sensing_device(narrow_pol, cbank, [0] * 4, dbank, [0] * 4, sbank, sog, E, K, LOG_STD, pb, noise_seed=SEED, first_step=FIRST,
                                         precision=precision)
    ob = list(ob[:6]) + [ob[6].clone()]
    _every_env_ended(ob[4], "sensing launch")
    differ = (oa[1] != ob[1]).any(dim=2)                                             # the finding, if any: print it before asserting
    if bool(differ.any()):
        step = int(differ.any(dim=1).nonzero()[0])
        print(variant, ga, H, precision, "FINDING: actions differ, first at step", step, "largest |difference|", float((oa[1] - ob[1]).abs().max()))
    for name, x, y in zip(NAMES[1:6], oa[1:6], ob[1:6]):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert torch.equal(oa[0][..., :L], ob[0]) and torch.equal(oa[6][:, :L], ob[6]), "the first L columns of every row"
    assert torch.equal(ta[..., :L], tb), "terminal rows"
    _same_state(a, b, "after")
    for g in range(4):
        _tail_is_a_history(oa[0][:, g * E:(g + 1) * E], oa[4][:, g * E:(g + 1) * E], L, "group %d" % g)
    for g, dg in enumerate((0, 2, 0, 4)):                                            # the delay's entries are the sensing launch's; the history's come on top
        assert torch.equal(_bits(pa[g * E:(g + 1) * E, :4 * dg]), _bits(pb[g * E:(g + 1) * E, :4 * dg])), g
        assert not bool(_bits(pb[g * E:(g + 1) * E, 4 * dg:]).any()) and not bool(_bits(pa[g * E:(g + 1) * E, 4 * max(dg, H):]).any()), g
    a.close(); b.close(); cbank.close(); dbank.close(); sbank.close(); narrow_pol.close(); wide_pol.close()


# ---- 3. continuation --------------------------------------------------------------------------------------------------------------------------
_CONT = [(v, ga, h, d) for v in ("e2e", "indi") for ga, h, d in ((1, 3, 1), (1, 2, 4))]           # H > d > 0, d > H


@pytest.mark.parametrize("variant,ga,H,d", _CONT, ids=["%s-ga%d-h%d-d%d" % c for c in _CONT])
def test_k_steps_equal_k_launches_of_one_step(variant, ga, H, d):
    from optimal_quad_control_rl_amd._closed_loop import rollout_outputs

    cog, sog = [0, 1, 0, 1], [0, 1, 1, 0]
    conds = [_short(variant, 0), _short(variant, 1)]
    a, b = (_handle(variant, 4 * E, ga, conds[0], env_id_base=BASE) for _ in range(2))
    W = a.state_len + 4 * H
    cbank, pol, dbank = _bank(variant, conds), _policy(variant, W), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(NOISY, d), _sensor(delay=d)])
    for e in (a, b):
        e.condition_reset(conds, cog, E)
        _force_rows(e, 4)
    ta, tb = _wide_term_buffer(a, K, W), _wide_term_buffer(b, 1, W)
    pa, pb = _pending(a), _pending(b)
    oa = _fly(a, pol, cbank, cog, dbank, sbank, sog, H, K, pa)
    ob = rollout_outputs(K, 4 * E, W, b.device)
    terms, last = [], None
    for k in range(K):
        tb.fill_(SENTINEL)
        step = _fly(b, pol, cbank, cog, dbank, sbank, sog, H, 1, pb, first=FIRST + k, out=tuple(t[k:k + 1] for t in ob))
        terms.append(tb[0].clone())
        if last is not None:
            assert torch.equal(_bits(last), _bits(ob[0][k])), ("last_obs of call %d is row 0 of call %d" % (k - 1, k))
        last = step[6]
    _every_env_ended(oa[4], "one call")
    m = max(d, H)
    assert FIRST < 2 ** 32 < FIRST + K and int(oa[5].sum()) >= 1 and bool(pa[:, 4 * (m - 1):4 * m].any()) and not bool(_bits(pa[:, 4 * m:]).any())
    for name, x, y in zip(NAMES[:6], oa, ob):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert torch.equal(_bits(oa[0]), _bits(ob[0])) and torch.equal(_bits(oa[6]), _bits(last)), "rows and last_obs"
    assert torch.equal(_bits(ta), _bits(torch.stack(terms))) and int((ta[..., -1] != SENTINEL).sum()) == int(oa[4].sum()), "terminal rows"
    _same_state(a, b, "K launches")
    assert torch.equal(_bits(pa), _bits(pb)), "pending"
    a.close(); b.close(); cbank.close(); pol.close(); dbank.close(); sbank.close()


# ---- 4. the evaluator ------------------------------------------------------------------------------------------------------------------------
_EVAL = [(v, ga, h, d, "f16-operands") for v in ("e2e", "indi") for ga, h in ((1, 2), (0, 4), (3, 1)) for d in (0, 3)] + \
        [("e2e", 1, 2, 3, "f32"), ("indi", 0, 4, 3, "f32")]


def _evaluate(env, pbank, cbank, dbank, sbank, pol, cog, sog, H, steps, pend, rec, recf, precision, seed, first):
    return env.evaluate_history_grid_device(pbank, cbank, dbank, sbank, pol, cog, [0] * len(cog), sog, H, E, steps, pend, rec, recf, precision=precision,
                                            noise_seed=seed, first_step=first)


@pytest.mark.parametrize("variant,ga,H,d,precision", _EVAL, ids=["%s-ga%d-h%d-d%d-%s" % c for c in _EVAL])
def test_evaluator_equals_the_per_step_loop(variant, ga, H, d, precision):
    """group 1 of four flies (noise, delay d) and is held against the loop (group-local ids: the twin has the env's base); groups 0, 2, 3
    fly ideal, noise alone and delay alone from the same start"""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    steps, gpl = SC["steps"], SC[variant + "_gates_per_lap"]
    cond = _eval_conditions(variant)[0]
    env = _based_twin(variant, 4 * E, ga, cond.replace(max_steps=97), BASE)
    twin = _based_twin(variant, E, ga, cond, BASE)
    W = env.state_len + 4 * H
    layers = _closed_loop_layers(W, SC[variant + "_action"], seed=3)
    pbank, cbank, dbank = _policy_bank(W, [layers]), _condition_bank(variant, [cond]), _dynamics_bank(variant, [None])
    pol = MfmaPolicy(W).set_weights(layers)
    sbank = _sensing_bank([None, _sensor(NOISY, d), _sensor(NOISY, 0), _sensor(delay=d or 1)])
    env.condition_starts([cond], [0] * 4, E)
    state = env.get_state_tensors()
    twin.set_state_tensors(*[None if t is None else t[E:2 * E] for t in state])
    twin.update_states()
    rec, recf = _records(env)
    pend = _pending(env)
    _evaluate(env, pbank, cbank, dbank, sbank, [0] * 4, [0] * 4, [0, 1, 2, 3], H, steps, pend, rec, recf, precision, SEED, FIRST)
    noise = env.sensing_noise_device(sbank, 1, E, steps, noise_seed=SEED, first_step=FIRST)
    ref = _loop(twin, pol, noise, d, H, steps, precision, targets=True)
    seq = [ref[k].cpu().numpy() for k in ("before", "after", "done", "trunc", "rew")]
    srec, srecf = S.run(*S.new_records(E), *seq, gates_per_lap=gpl)
    ends = int(srec[:, 1].sum() + srec[:, 2].sum())
    print(variant, "ga", ga, "H", H, "d", d, precision, "passes", int(srec[:, 0].sum()), "crashes", int(srec[:, 1].sum()), "time limits", int(srec[:, 2].sum()))
    assert ends >= E and bool((srec[:, 5] == steps).all()) and bool(ref["obs"][1:, :, env.state_len:].any())
    lo, hi = E, 2 * E
    got, gotf = rec[lo:hi].cpu().numpy(), recf[lo:hi].cpu().numpy()
    bad = np.nonzero((got != srec).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:2]], srec[bad[:2]])
    assert np.array_equal(gotf.view(np.uint32), srecf.view(np.uint32)), "float records"
    _group_equals(env.get_state_tensors(), twin, lo, hi, "state after")
    assert torch.equal(_bits(pend[lo:hi]), _bits(ref["queue"])), "pending"
    for g, dg in enumerate((0, d, 0, d or 1)):
        m = max(dg, H)
        assert bool(pend[g * E:(g + 1) * E, 4 * (m - 1):4 * m].any()) and not bool(_bits(pend[g * E:(g + 1) * E, 4 * m:]).any()), g
    cells = [(rec[g * E:(g + 1) * E], _bits(recf[g * E:(g + 1) * E])) for g in range(4)]
    same = lambda i, j: torch.equal(cells[i][0], cells[j][0]) and torch.equal(cells[i][1], cells[j][1])
    assert not same(0, 2) and not same(0, 3) and (d == 0 or not same(1, 2)), "the sensors matter"
    env.close(); twin.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close(); pol.close()


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_permuting_the_groups_permutes_the_records(variant):
    """a group depends on its (policy, condition, dynamics, sensing) quadruple and H only (group-local ids): launch B flies launch A's
    cells in another order from the same starts and its records are A's, permuted"""
    ga, H, steps, order = 1, 2, 300, [2, 0, 3, 1]
    conds = _eval_conditions(variant)
    a, b = (_based_twin(variant, 4 * E, ga, conds[0], BASE) for _ in range(2))
    W = a.state_len + 4 * H
    act = np.asarray(SC[variant + "_action"], np.float32)
    pbank = _policy_bank(W, [_closed_loop_layers(W, act, seed=3), _closed_loop_layers(W, act, seed=4)])
    cbank, dbank = _condition_bank(variant, conds), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(NOISY, 3), _sensor(delay=1), _sensor(tuple(2 * s for s in NOISY), 0)])
    cells = [(0, 0, 0), (1, 1, 1), (0, 2, 2), (1, 0, 1)]                            # (policy, condition, sensing) of groups 0..3
    a.condition_starts(conds, [c[1] for c in cells], E)
    state = a.get_state_tensors()
    rows = torch.cat([torch.arange(order[j] * E, (order[j] + 1) * E) for j in range(4)]).to(a.device)
    b.set_state_tensors(*[None if t is None else t[rows].contiguous() for t in state])
    out = []
    for env, cs in ((a, cells), (b, [cells[j] for j in order])):
        rec, recf = _records(env)
        pend = _pending(env)
        _evaluate(env, pbank, cbank, dbank, sbank, [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs], H, steps, pend, rec, recf, "f16-operands",
                  SEED, FIRST)
        out.append((rec, recf, pend, env.get_state_tensors()))
    (ra, rfa, pa, sa), (rb, rfb, pb, sb) = out
    assert int((ra[:, 1] + ra[:, 2]).sum()) >= 1 and bool((ra[:, 5] == steps).all())
    assert torch.equal(ra[rows], rb) and torch.equal(_bits(rfa[rows]), _bits(rfb)) and torch.equal(_bits(pa[rows]), _bits(pb))
    for x, y in zip(sa, sb):
        assert x is None or torch.equal(x[rows], y)
    assert not torch.equal(ra[:E], ra[3 * E:]) and not torch.equal(ra[:E], ra[2 * E:3 * E])
    a.close(); b.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close()


# ---- 5. the rollout hands over to the evaluator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,ga,H,d", [("e2e", 1, 3, 1), ("indi", 2, 2, 4)])
def test_a_rollout_hands_its_queue_to_an_evaluation(variant, ga, H, d):
    """K1 deterministic rollout steps, then K2 evaluated steps through the same pending, against the two per-step loops chained.  Group 0
    is compared: its ordinary env ids (the rollout's) are its group-local ones (the evaluator's), so one twin follows both reset streams."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    K1, K2 = 24, 40
    cond = _short(variant)
    env = _handle(variant, 4 * E, ga, cond, env_id_base=BASE)
    twin = _handle(variant, E, ga, cond, env_id_base=BASE)
    W = env.state_len + 4 * H
    layers = _closed_loop_layers(W, np.asarray(SC[variant + "_action"], np.float32), seed=3)
    pol, pbank = MfmaPolicy(W).set_weights(layers), _policy_bank(W, [layers])
    cbank, dbank = _bank(variant, [cond]), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(NOISY, d), None, _sensor(delay=d), _sensor(NOISY, 0)])
    _force_rows(env, 4)
    twin.set_state_tensors(*[None if t is None else t[:E] for t in env.get_state_tensors()])
    twin.update_states()
    pend = _pending(env)
    out = _fly(env, pol, cbank, [0] * 4, dbank, sbank, [0, 1, 2, 3], H, K1, pend, det=True)
    handed = pend.clone()
    rec, recf = _records(env)
    _evaluate(env, pbank, cbank, dbank, sbank, [0] * 4, [0] * 4, [0, 1, 2, 3], H, K2, pend, rec, recf, "f16-operands", SEED, FIRST + K1)
    n1 = twin.sensing_noise_device(sbank, 0, E, K1, noise_seed=SEED, first_step=FIRST)
    n2 = twin.sensing_noise_device(sbank, 0, E, K2, noise_seed=SEED, first_step=FIRST + K1)
    r1 = _loop(twin, pol, n1, d, H, K1, "f16-operands")
    assert torch.equal(_bits(out[0][:, :E]), _bits(r1["obs"])) and torch.equal(_bits(handed[:E]), _bits(r1["queue"])) and bool(handed[:E, :4 * max(d, H)].any())
    r2 = _loop(twin, pol, n2, d, H, K2, "f16-operands", queue=r1["queue"], targets=True)
    srec, srecf = S.run(*S.new_records(E), *[r2[k].cpu().numpy() for k in ("before", "after", "done", "trunc", "rew")],
                        gates_per_lap=cond.gates_per_lap)
    ends = r1["done"].to(torch.int32).sum(0) + r2["done"].to(torch.int32).sum(0)
    assert int(ends.min()) >= 1 and int(r1["done"].sum()) >= 1 and int(r2["done"].sum()) >= 1, "episodes end in both phases"
    assert not torch.equal(r2["obs"][0, :, env.state_len:], torch.zeros_like(r2["obs"][0, :, env.state_len:])), "the evaluation starts with the rollout's history"
    assert np.array_equal(rec[:E].cpu().numpy(), srec) and np.array_equal(recf[:E].cpu().numpy().view(np.uint32), srecf.view(np.uint32))
    _group_equals(env.get_state_tensors(), twin, 0, E, "state after")
    assert torch.equal(_bits(pend[:E]), _bits(r2["queue"])), "pending"
    env.close(); twin.close(); pol.close(); pbank.close(); cbank.close(); dbank.close(); sbank.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from test_gpu_dynamics_grid import _vehicles

    Kr, ga, H = 8, 1, 2
    n = 2 * E
    conds = _conditions("indi")
    env = _handle("indi", n, ga, conds[0])
    L, Lenv = env._L, env.state_len
    W = Lenv + 4 * H
    act = np.asarray(SC["indi_action"], np.float32)
    pol, own_len, longer = _policy("indi", W), _policy("indi", Lenv), _policy("indi", Lenv + 12)
    pbank, bank_own = _policy_bank(W, [_closed_loop_layers(W, act)]), _policy_bank(Lenv, [_closed_loop_layers(Lenv, act)])
    cbank = _bank("indi", conds[:2], capacity=3)                                      # slots 0, 1 set, slot 2 never set
    dbank = _dynamics_bank("indi", _vehicles("indi", 2), capacity=3)                  # likewise
    sbank = _sensing_bank([_sensor(NOISY, 2), _sensor(delay=1)], capacity=3)          # likewise
    dev = env.device
    wide = Lenv + 16                                                                 # room for any row a refused call might have written
    bufs = dict(obs=torch.full((Kr, n, wide), SENTINEL, device=dev), act=torch.full((Kr, n, 4), SENTINEL, device=dev),
                logp=torch.full((Kr, n), SENTINEL, device=dev), rew=torch.full((Kr, n), SENTINEL, device=dev),
                done=torch.full((Kr, n), 7, dtype=torch.uint8, device=dev), trunc=torch.full((Kr, n), 7, dtype=torch.uint8, device=dev),
                last=torch.full((n, wide), SENTINEL, device=dev), pend=torch.full((n, 16), SENTINEL, device=dev),
                rec=torch.full((n, S.REC_INTS), 7, dtype=torch.int32, device=dev), recf=torch.full((n, S.REC_FLOATS), SENTINEL, device=dev),
                term=torch.full((Kr, n, wide), SENTINEL, device=dev))
    env.set_terminal_obs_buffer(bufs["term"], obs_len=wide)
    before = env.get_state_tensors()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    h = lambda x: x._h if x is not None else None
    ip = lambda m: None if m is None else np.asarray(m, np.int32).ctypes.data_as(i32p)

    def rollout(p=pol, cb=cbank, db=dbank, sb=sbank, g=2, cog=(1, 0), dog=(0, 1), sog=(1, 0), hist=H, k=Kr, flags=0, first=0, pend=True):
        return L.qr_rollout_policy_history(env._h, h(p), h(cb), h(db), h(sb), g, E, ip(cog), ip(dog), ip(sog), hist, k, LOG_STD.ctypes.data_as(f32p), 3, first,
                                           flags, _ptr(bufs["pend"]) if pend else None, _ptr(bufs["obs"]), _ptr(bufs["act"]), _ptr(bufs["logp"]),
                                           _ptr(bufs["rew"]), _ptr(bufs["done"]), _ptr(bufs["trunc"]), _ptr(bufs["last"]), env._stream())

    def evaluate(pb=pbank, cb=cbank, db=dbank, sb=sbank, g=2, pog=(0, 0), cog=(1, 0), dog=(0, 1), sog=(1, 0), hist=H, k=Kr, flags=0, first=0, pend=True):
        return L.qr_evaluate_policy_history_grid(env._h, h(pb), h(cb), h(db), h(sb), g, E, ip(pog), ip(cog), ip(dog), ip(sog), hist, k, flags, 3, first,
                                                 _ptr(bufs["pend"]) if pend else None, _ptr(bufs["rec"]), _ptr(bufs["recf"]), env._stream())

    def untouched():
        torch.cuda.synchronize()
        for name, t in bufs.items():
            assert bool((t == (SENTINEL if t.dtype == torch.float32 else 7)).all()), name
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    def refused(call, who, code, message, **kw):
        rc = call(**kw)
        err = L.qr_last_error()
        assert rc == code, (who, list(kw.keys()), rc, err)
        assert who in err and message in err, err
        untouched()

    for call, who in ((rollout, b"qr_rollout_policy_history"), (evaluate, b"qr_evaluate_policy_history_grid")):
        for bad in (0, 5, 5 - ga, -1):                                                # 5 - gates_ahead: the first value past the range
            refused(call, who, _lib.QR_E_INVALID, b"history must be in [1, 4 - gates_ahead]", hist=bad)
        refused(call, who, _lib.QR_E_INVALID, b"history must be in", hist=0, sb=None)                          # ... ahead of the sensing bank's refusals
        refused(call, who, _lib.QR_E_INVALID, b"num_steps" if call is evaluate else b"bad argument", k=0, hist=0)   # ... behind the call's own arguments
        # the sensing twin's refusals, spot-checked in its order
        refused(call, who, _lib.QR_E_INVALID, b"null condition bank", cb=None, db=None, sb=None)
        refused(call, who, _lib.QR_E_STATE, b"condition bank was never set", cog=(2, 0), dog=(2, 0), sog=(2, 0))
        refused(call, who, _lib.QR_E_INVALID, b"dynamics_of_group[1] is outside the dynamics bank", dog=(0, 3), sog=(0, 3))
        refused(call, who, _lib.QR_E_INVALID, b"null sensing bank", sb=None, pend=False)
        refused(call, who, _lib.QR_E_INVALID, b"sensing_of_group[0] is outside the sensing bank", sog=(3, 0))
        refused(call, who, _lib.QR_E_INVALID, b"2^56", first=2 ** 64 - 1, sog=(2, 0))
        refused(call, who, _lib.QR_E_STATE, b"slot 2 of the sensing bank was never set", sog=(2, 0))
        refused(call, who, _lib.QR_E_INVALID, b"pending_dev is required", pend=False)
    # the observation length: the env's own is refused, and so is any other than obs_len + 4 * history
    refused(rollout, b"qr_rollout_policy_history", _lib.QR_E_INVALID, b"policy obs_len != env obs_len + 4 * history", p=own_len)
    refused(rollout, b"qr_rollout_policy_history", _lib.QR_E_INVALID, b"policy obs_len != env obs_len + 4 * history", p=longer)
    refused(rollout, b"qr_rollout_policy_history", _lib.QR_E_INVALID, b"policy obs_len != env obs_len + 4 * history", hist=3)
    refused(rollout, b"qr_rollout_policy_history", _lib.QR_E_INVALID, b"history must be in", p=own_len, hist=0)    # the range comes first
    refused(evaluate, b"qr_evaluate_policy_history_grid", _lib.QR_E_INVALID, b"bank obs_len != env obs_len + 4 * history", pb=bank_own)
    refused(evaluate, b"qr_evaluate_policy_history_grid", _lib.QR_E_INVALID, b"bank obs_len != env obs_len + 4 * history", hist=1)
    refused(evaluate, b"qr_evaluate_policy_history_grid", _lib.QR_E_INVALID, b"history must be in", pb=bank_own, hist=4)
    # the Python layer refuses a terminal buffer of another width before the library is called
    with pytest.raises(ValueError, match="terminal-observation buffer"):
        env.rollout_policy_history_device(pol, cbank, [0, 0], dbank, [0, 0], sbank, [0, 0], H, E, Kr, LOG_STD, _pending(env))
    untouched()
    # ... and valid calls run and write every row at the longer width
    bufs["pend"].zero_()
    env.set_terminal_obs_buffer(None)
    tight = torch.full((Kr, n, W), SENTINEL, device=dev)
    out = env.rollout_policy_history_device(pol, cbank, [1, 0], dbank, [0, 1], sbank, [1, 0], H, E, Kr, LOG_STD, bufs["pend"],
                                            out=(tight, bufs["act"], bufs["logp"], bufs["rew"], bufs["done"], bufs["trunc"]))
    torch.cuda.synchronize()
    assert bool((tight != SENTINEL).all()) and bool((bufs["done"] <= 1).all()) and tuple(out[6].shape) == (n, W) and env.last_rollout_ms() > 0.0
    assert bool(bufs["pend"][:, 4:8].any()) and not bool(_bits(bufs["pend"][:, 8:]).any())       # max(d, H) = 2 entries in both groups
    bufs["rec"].zero_(); bufs["recf"].zero_()
    assert evaluate() == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((bufs["rec"][:, 5] == Kr).all())
    for x in (env, cbank, pol, own_len, longer, pbank, bank_own, dbank, sbank):
        x.close()


# ---- 7. PPO -----------------------------------------------------------------------------------------------------------------------------------
def _ppo_env(n, seed=21):
    cond = _conditions("e2e")[0].replace(max_steps=MAX_STEPS)
    return _handle("e2e", n, 1, cond, seed=seed)


def _theta(model):
    return torch.cat([p.detach().reshape(-1) for p in model.policy.parameters()])


def test_ppo_with_a_command_history_resumes_bit_for_bit():
    from optimal_quad_control_rl_amd.ppo import PPO
    from optimal_quad_control_rl_amd.sensing import SensingParams

    n, T, H = 1024, 16, 2
    sensors = [SensingParams.from_sigma(NOISY, 2, name="noisy d=2")]
    kw = dict(n_steps=T, seed=4, fused_collect=True, native_update=True, sensing=sensors, command_history=H)

    def round_(m):
        m.collect(); m.train()
        ps = m.stats["per_sensor"]
        assert [s["name"] for s in ps] == ["noisy d=2"] and ps[0]["episodes"] == int(m._done_u8.sum())
        return int(m._done_u8.sum())

    ea, eb, ec, ed = (_ppo_env(n) for _ in range(4))
    whole, first = PPO(ea, **kw), PPO(eb, **kw)
    W = ea.state_len + 4 * H
    assert whole.command_history == H and whole.policy.pi[0].in_features == W == whole.policy.vf[0].in_features
    assert tuple(whole.buf_obs.shape) == (T, n, W) and tuple(whole._term_obs.shape) == (T, n, W) and whole._mfma.obs_len == W
    calls = []
    launch = ea.rollout_policy_history_device
    ea.rollout_policy_history_device = lambda *a, **k: (calls.append(a[7]), launch(*a, **k))[1]
    _force_rows(ea, n // E); _force_rows(eb, n // E)                                        # episodes that end inside the first rollout
    ended = [round_(whole) for _ in range(3)]
    assert calls == [H] * 3 and ended[0] >= len(GROUND_ROWS) * (n // E) and sum(ended[1:]) >= n  # the time limit of 30 falls inside rounds 2 and 3
    tail = whole.buf_obs[:, :, ea.state_len:]
    assert bool(tail[1:].any()) and not bool(_bits(tail[1:][whole.buf_done[:-1].bool()]).any()), "a history, cleared behind each episode end"
    if int(whole._trunc_u8.sum()):
        rows = whole._trunc_u8.bool()
        assert bool(whole._term_obs[rows][:, ea.state_len:ea.state_len + 4].any()), "terminal rows carry the last command"
    round_(first); round_(first)
    sd, params = first.state_dict(), {k: v.clone() for k, v in first.policy.state_dict().items()}
    saved = sd["sensing"]["pending"]
    assert sd["command_history"] == H and saved.shape == (n, 16) and bool(saved[:, :8].any()) and not bool(saved[:, 8:].any())
    resumed = PPO(ec, **kw)
    resumed.policy.load_state_dict(params)
    resumed.load_state_dict(sd)
    assert torch.equal(_bits(resumed._pending.cpu()), _bits(saved))
    round_(resumed)
    assert torch.equal(_bits(_theta(whole)), _bits(_theta(resumed))) and torch.equal(whole.buf_rew, resumed.buf_rew)
    assert torch.equal(_bits(whole.buf_obs), _bits(resumed.buf_obs)) and torch.equal(_bits(whole._pending), _bits(resumed._pending))
    assert torch.equal(_bits(whole._updater.m), _bits(resumed._updater.m)) and torch.equal(_bits(whole._updater.v), _bits(resumed._updater.v))
    assert repr(whole.stats["per_sensor"]) == repr(resumed.stats["per_sensor"])
    # a checkpoint with a history into a PPO without one, and the reverse: refused, naming both values, before anything is loaded
    plain = PPO(ed, **{**kw, "command_history": 0})
    assert "command_history" not in plain.state_dict() and plain.policy.pi[0].in_features == ed.state_len
    theta = _theta(plain).clone()
    with pytest.raises(ValueError, match="command_history=2.*command_history=0"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="command_history=0.*command_history=2"):
        resumed.load_state_dict(plain.state_dict())
    assert torch.equal(theta, _theta(plain))
    # without `sensing` the run flies under one ideal sensor
    assert [s.name for s in PPO(ed, n_steps=T, seed=4, fused_collect=True, native_update=True, command_history=1).sensing] == ["ideal"]
    for e in (ea, eb, ec, ed):
        e.close()


# ---- 8. time, printed ----------------------------------------------------------------------------------------------------------------------------
def test_history_launch_time_is_printed():
    """Median us per step of the history launch at (gates_ahead 1, H 2) against the sensing launch at gates_ahead 3 -- the same row length
    (E2E: 32) and the same networks -- for the rollout and for the evaluator: ideal slots, the NOISY sigmas, NOISY + d = 4, both precisions.
    N = 65 536 = 256 groups x 256 envs, K = 200, E2E + residual MLPs + training disturbances, square track, nominal vehicles.  Launches
    alternate from the same seeded reset in ORDER-SWAPPED pairs, one warm-up pair, medians of 6, host clock around a stream synchronise.
    NO bound is asserted: nobody had measured these kernels when the test was written (DESIGN.md section 8 and
    profiles/command_history_time.txt hold the numbers of one run)."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd._closed_loop import rollout_outputs
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.policy import MfmaPolicy, MfmaPolicyBank
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    n, Kc, H = 65536, 200, 2
    groups = n // E
    envs = {}
    for name, ga in (("history", 1), ("sensing", 3)):
        env = Quadcopter3DGates(n, *square_track(), gates_ahead=ga, infos_mode="none", seed=99)
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        envs[name] = (env, _bank("e2e", [Condition.from_env(env)]), _pending(env))
    W = envs["sensing"][0].state_len
    assert W == envs["history"][0].state_len + 4 * H == 32
    dbank = _dynamics_bank("e2e", [None])
    sbank = _sensing_bank([None, _sensor(NOISY, 0), _sensor(NOISY, 4)])
    torch.manual_seed(0)
    actor = ActorCritic(W, 4).pi
    pol = MfmaPolicy(W).load_torch(actor)
    pbank = MfmaPolicyBank(W, 1)
    pbank.load_torch(0, actor)
    dev = envs["history"][0].device
    out = rollout_outputs(Kc, n, W, dev)
    rec, recf = torch.zeros((n, S.REC_INTS), dtype=torch.int32, device=dev), torch.zeros((n, S.REC_FLOATS), dtype=torch.float32, device=dev)
    log_std, zero = np.zeros(4, np.float32), [0] * groups
    stream = torch.cuda.current_stream(dev)

    def timed(name, launch):
        env, _, pend = envs[name]
        env.seed(99); env.reset_device()
        pend.zero_(); rec.zero_(); recf.zero_()
        stream.synchronize()
        t0 = time.perf_counter()
        launch()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / Kc

    eh, ch, ph = envs["history"]
    es, cs, ps = envs["sensing"]
    for precision in ("f16-operands", "f32"):
        for label, slot in (("ideal slots", 0), ("noise on", 1), ("noise on, d = 4", 2)):
            sog = [slot] * groups
            pairs = {
                "rollout": (lambda: eh.rollout_policy_history_device(pol, ch, zero, dbank, zero, sbank, sog, H, E, Kc, log_std, ph, noise_seed=1, out=out,
                                                                     precision=precision),
                            lambda: es.rollout_policy_sensing_device(pol, cs, zero, dbank, zero, sbank, sog, E, Kc, log_std, ps, noise_seed=1, out=out,
                                                                     precision=precision)),
                "evaluator": (lambda: eh._L.qr_evaluate_policy_history_grid(eh._h, pbank._h, ch._h, dbank._h, sbank._h, groups, E, *_maps(zero, sog), H, Kc,
                                                                            2 if precision == "f32" else 0, 1, 0, _ptr(ph), _ptr(rec), _ptr(recf), eh._stream()),
                              lambda: es._L.qr_evaluate_policy_sensing_grid(es._h, pbank._h, cs._h, dbank._h, sbank._h, groups, E, *_maps(zero, sog), Kc,
                                                                            2 if precision == "f32" else 0, 1, 0, _ptr(ps), _ptr(rec), _ptr(recf), es._stream())),
            }
            for what, (hist, sens) in pairs.items():
                t_h, t_s = [], []
                for rep in range(7):
                    if rep % 2 == 0:
                        a = timed("history", hist); b = timed("sensing", sens)
                    else:
                        b = timed("sensing", sens); a = timed("history", hist)
                    if rep:
                        t_h.append(a); t_s.append(b)
                mh, ms = statistics.median(t_h), statistics.median(t_s)
                print("%s, %s, %s: history (gates_ahead 1, H 2) median %.4f us/step %s; sensing (gates_ahead 3) median %.4f us/step %s; ratio %.4f"
                      % (what, precision, label, mh, ["%.3f" % t for t in t_h], ms, ["%.3f" % t for t in t_s], mh / ms))
                assert mh > 0.0 and ms > 0.0
    for env, cb, _ in envs.values():
        env.close(); cb.close()
    dbank.close(); sbank.close(); pol.close(); pbank.close()


def _maps(zero, sog):
    """the four host maps (policy, condition, dynamics, sensing) of an evaluator call as int32 pointers; the arrays live in the tuple"""
    arrs = [np.asarray(m, np.int32) for m in (zero, zero, zero, sog)]
    _maps.keep = arrs
    return [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arrs]
