"""GPU: the collect launch of the PRIVILEGED CRITIC -- qr_rollout_policy_privileged (rollout_policy_group_kernel<V, GA, kF32, false, true,
RuntimeSensing, H, true>, csrc/quadrace_rollout_privileged.hip): the sensing (H = 0) / history (H >= 1) rollout that also stores the row
before the sensor's noise.  Model: include/quadrace.h; the sensor is tests/sensing_spec.py, the history tests/command_history_spec.py.

1. Every twin output, pending, the terminal rows and the env state equal the twin launch (qr_rollout_policy_sensing for H = 0,
   qr_rollout_policy_history for H >= 1) in all 15 (GA, H) forms of both variants; the ideal group's clean rows equal obs_out, the noisy
   group's differ in every sigma group and agree in the history tail.
2. The clean rows equal a per-step loop on a twin handle: critic_obs[k] = [the twin's observation before the noise | h_k], obs[k] =
   perturb of it, critic_last_obs likewise.
3. K steps in one call equal K launches of one step, critic_last_obs of one launch being row 0 of the next.
4. Three groups (the grid runs over more than the two groups of 1.) and the widest tile (E2E, gates_ahead 4).
5. Refusals launch nothing.   6. Time, printed.
Every comparison is bit for bit.  Shapes: 512 envs = 2 groups of 256 -- group 0 through an ideal slot, group 1 through a noisy slot (all
eight sigmas non-zero) with a delay -- env_id_base = 2^32 - 300, first_step = 2^32 - 5 (the low step word wraps inside K), K = 12, and the
short-episode scenario of the sensing and history tests with its time limit moved inside these 12 steps (max_steps = 9, 7 on the other
track): crashes (the forced rows), time-limit ends and resets all fall inside the window, and every test asserts on its own outputs that
every env ended an episode."""
import ctypes as C
import statistics
import time

import numpy as np
import pytest
import torch

import command_history_spec as CH
import sensing_spec as SS
from eval_helpers import SENTINEL, _group_equals, _ptr
from test_gpu_dynamics_grid import _dynamics_bank
from test_gpu_rollout_conditions import GROUND_ROWS, LOG_STD, _bank, _force_rows, _handle, _policy
from test_gpu_rollout_sensing import NAMES, SEED, _every_env_ended, _same_state, _short
from test_gpu_sensing_grid import BASE, NOISY, VAR, _bits, _pending, _sensing_bank, _sensor

pytestmark = pytest.mark.gpu

E, K, FIRST, LIMIT = 256, 12, 2 ** 32 - 5, 9
PAIRS = [(ga, h) for ga in range(5) for h in range(0, 5 - ga)]                        # the 15 (GA, H) with GA + H <= 4, H = 0 included
assert len(PAIRS) == 15 and all(s > 0 for s in NOISY) and len(NOISY) == 8


def _delay(ga, H):
    """one delay per form: 0, 1, 2, 3 and 4 all occur, with d < H, d = H and d > H"""
    return (ga + 2 * H + 1) % 5


assert {_delay(*p) for p in PAIRS} == {0, 1, 2, 3, 4} and {(_delay(g, h) > h) - (_delay(g, h) < h) for g, h in PAIRS if h} == {-1, 0, 1}


def _cond(variant, k=0):
    """the short-episode scenario (test_gpu_rollout_sensing._short) with the time limit inside K = 12"""
    return _short(variant, k).replace(max_steps=LIMIT - 2 * k)


def _term(env, rows, width):
    tb = torch.full((rows, env.num_envs, width), SENTINEL, device=env.device)
    env.set_terminal_obs_buffer(tb, obs_len=width)
    return tb


def _fly_priv(env, pol, cbank, cog, dbank, sbank, sog, H, k, pend, first=FIRST, det=False, precision="f16-operands", out=None):
    """the privileged launch over nominal vehicles: (obs, act, logp, rew, done, trunc, last_obs) in the twin's order, then critic_obs and
    critic_last_obs; the two last-row buffers as copies (the env reuses them)"""
    o = env.rollout_policy_privileged_device(pol, cbank, cog, dbank, [0] * len(cog), sbank, sog, H, E, k, LOG_STD, pend, noise_seed=SEED, first_step=first,
                                             deterministic=det, out=out, precision=precision)
    return [o[0]] + list(o[2:7]) + [o[7].clone()], o[1], o[8].clone()


def _fly_twin(env, pol, cbank, cog, dbank, sbank, sog, H, k, pend, first=FIRST, det=False, precision="f16-operands"):
    args = (pol, cbank, cog, dbank, [0] * len(cog), sbank, sog)
    kw = dict(noise_seed=SEED, first_step=first, deterministic=det, precision=precision)
    o = env.rollout_policy_history_device(*args, H, E, k, LOG_STD, pend, **kw) if H else env.rollout_policy_sensing_device(*args, E, k, LOG_STD, pend, **kw)
    return list(o[:6]) + [o[6].clone()]


def _twin_equality(variant, ga, H, precision, groups=2, sog=None):
    """launch A = the privileged launch, launch B = its twin, from the same forced starts: everything the twin writes, bit for bit; then
    what the clean rows must be without any restatement (the ideal group, the sigma groups, the history tail)"""
    d = _delay(ga, H)
    sog = sog or [0, 1]
    cog = [g % 2 for g in range(groups)]
    conds = [_cond(variant, 0), _cond(variant, 1)]
    a, b = (_handle(variant, groups * E, ga, conds[0], env_id_base=BASE) for _ in range(2))
    L = a.state_len
    W = L + 4 * H
    cbank, pol, dbank = _bank(variant, conds), _policy(variant, W), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([None, _sensor(NOISY, d), _sensor(delay=d or 1)])
    for e in (a, b):
        e.condition_reset(conds, cog, E)
        _force_rows(e, groups)
    ta, tb = _term(a, K, W), _term(b, K, W)
    pa, pb = _pending(a), _pending(b)
    oa, critic, critic_last = _fly_priv(a, pol, cbank, cog, dbank, sbank, sog, H, K, pa, precision=precision)
    ob = _fly_twin(b, pol, cbank, cog, dbank, sbank, sog, H, K, pb, precision=precision)
    done, trunc = ob[4].bool(), ob[5].bool()
    print(variant, "ga", ga, "H", H, "d", d, precision, "groups", groups, "ends", int(done.sum()), "crashes", int((done & ~trunc).sum()), "time limits",
          int(trunc.sum()))
    _every_env_ended(ob[4], "twin launch")
    assert int((done & ~trunc).sum()) >= groups * len(GROUND_ROWS) and int(trunc.sum()) >= 1
    for name, x, y in zip(NAMES, oa, ob):
        same = torch.equal(_bits(x), _bits(y)) if x.dtype == torch.float32 else torch.equal(x, y)
        assert x.shape == y.shape and x.dtype == y.dtype and same, (name, int((x != y).sum()))
    assert torch.equal(_bits(ta), _bits(tb)) and int((tb[..., 0] != SENTINEL).sum()) == int(done.sum()), "terminal rows"
    assert torch.equal(_bits(pa), _bits(pb)), "pending"
    _same_state(a, b, "after")
    assert tuple(critic.shape) == (K, groups * E, W) and tuple(critic_last.shape) == (groups * E, W)
    groups_of = torch.as_tensor(SS.GROUPS[(VAR[variant], ga)], device=a.device)
    for g, slot in enumerate(sog):
        lo, hi = g * E, (g + 1) * E
        rows, clean, last, clean_last = oa[0][:, lo:hi], critic[:, lo:hi], oa[6][lo:hi], critic_last[lo:hi]
        assert torch.equal(_bits(rows[..., L:]), _bits(clean[..., L:])) and torch.equal(_bits(last[:, L:]), _bits(clean_last[:, L:])), ("history tail", g)
        if slot == 1:                                       # the noisy slot: the two rows differ in every sigma group
            for k in range(8):
                cols = (groups_of == k).nonzero().squeeze(1)
                if cols.numel():
                    assert bool((rows[..., cols] != clean[..., cols]).any()) and bool((last[:, cols] != clean_last[:, cols]).any()), ("sigma group", k)
            assert float((rows[..., :L] != clean[..., :L]).float().mean()) > 0.99
        else:                                               # no noise (ideal, or delay alone): the clean rows are written and equal obs_out
            assert torch.equal(_bits(rows), _bits(clean)) and torch.equal(_bits(last), _bits(clean_last)), ("clean rows of a noise-free group", g)
    assert bool(torch.isfinite(critic).all()) and not bool((critic == SENTINEL).any())
    for x in (a, b, cbank, pol, dbank, sbank):
        x.close()


# ---- 1. the twin, bit for bit ----------------------------------------------------------------------------------------------------------------
_TWIN = [(v, ga, h, "f16-operands") for v in ("e2e", "indi") for ga, h in PAIRS] + \
        [(v, ga, h, "f32") for v in ("e2e", "indi") for ga, h in ((1, 0), (1, 2), (0, 4))]


@pytest.mark.parametrize("variant,ga,H,precision", _TWIN, ids=["%s-ga%d-h%d-%s" % c for c in _TWIN])
def test_every_twin_output_is_the_twin_launch_and_the_ideal_group_is_clean(variant, ga, H, precision):
    _twin_equality(variant, ga, H, precision)


# ---- 2. the clean rows against the per-step loop ---------------------------------------------------------------------------------------------
def _loop(twin, pol, noise, sigma_groups, d, H, steps, precision):
    """steps x [clean = row(obs, queue, H); seen = perturb(clean) -> forward -> clamp -> push -> step -> clear] on `twin`.  `noise` is the
    qr_sensing_noise dump (sigma * eps, the rounded product): perturb with unit sigmas adds it in float32, as the kernel does."""
    n, L, dev = twin.num_envs, twin.state_len, twin.device
    clean_rows, seen_rows = [], []
    queue = torch.zeros((n, 16), dtype=torch.float32, device=dev)
    obs = twin.states_tensor
    ones = (1.0,) * 8
    dones = []
    for k in range(steps + 1):
        o = obs.cpu().numpy()
        noisy = torch.as_tensor(SS.perturb(o, ones, noise[k].cpu().numpy(), sigma_groups), device=dev)
        clean_rows.append(CH.row(obs.clone(), queue, H))
        seen = CH.row(noisy, queue, H).contiguous()
        seen_rows.append(seen)
        if k == steps:
            break
        mean = pol.forward(seen, precision=precision)
        fly, queue = CH.push(queue, mean.clamp(-1, 1), d, H)
        obs, _, dd, _ = twin.step_device(fly.contiguous())
        queue = CH.clear(queue, dd)
        dones.append(dd.to(torch.uint8).clone())
    return torch.stack(clean_rows), torch.stack(seen_rows), torch.stack(dones), queue


_LOOP = [("e2e", 1, 2, "f16-operands"), ("indi", 0, 4, "f16-operands"), ("e2e", 1, 0, "f16-operands"), ("indi", 3, 1, "f32"), ("e2e", 4, 0, "f32"),
         ("indi", 2, 0, "f16-operands")]


@pytest.mark.parametrize("variant,ga,H,precision", _LOOP, ids=["%s-ga%d-h%d-%s" % c for c in _LOOP])
def test_clean_rows_equal_the_per_step_loop(variant, ga, H, precision):
    """group 1 (the noisy slot, delay d) against the loop on a twin handle with env_id_base + E, deterministic mode"""
    d = _delay(ga, H)
    cond = _cond(variant)
    env = _handle(variant, 2 * E, ga, cond, env_id_base=BASE)
    twin = _handle(variant, E, ga, cond, env_id_base=BASE + E)
    L = env.state_len
    W = L + 4 * H
    cbank, pol, dbank = _bank(variant, [cond]), _policy(variant, W), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([None, _sensor(NOISY, d)])
    env.reset_device()
    _force_rows(env, 2)
    state = [None if t is None else t[E:2 * E] for t in env.get_state_tensors()]
    twin.set_state_tensors(*state)
    twin.update_states()
    pend = _pending(env)
    out, critic, critic_last = _fly_priv(env, pol, cbank, [0, 0], dbank, sbank, [0, 1], H, K, pend, det=True, precision=precision)
    noise = twin.sensing_noise_device(sbank, 1, E, K + 1, noise_seed=SEED, first_step=FIRST)     # ordinary ids: the twin's base is the group's
    clean, seen, dones, queue = _loop(twin, pol, noise, SS.GROUPS[(VAR[variant], ga)], d, H, K, precision)
    _every_env_ended(dones, "twin")
    lo, hi = E, 2 * E
    assert torch.equal(_bits(critic[:, lo:hi]), _bits(clean[:K])), "critic_obs_out[k] = [the twin's observation before the noise | h_k]"
    assert torch.equal(_bits(out[0][:, lo:hi]), _bits(seen[:K])), "obs_out[k] = perturb of it"
    assert torch.equal(_bits(critic_last[lo:hi]), _bits(clean[K])) and torch.equal(_bits(out[6][lo:hi]), _bits(seen[K])), "the two last rows"
    assert torch.equal(out[4][:, lo:hi], dones) and torch.equal(_bits(pend[lo:hi]), _bits(queue))
    assert not torch.equal(critic[:, lo:hi, :L], out[0][:, lo:hi, :L])
    _group_equals(env.get_state_tensors(), twin, lo, hi, "state after")
    for x in (env, twin, cbank, pol, dbank, sbank):
        x.close()


# ---- 3. continuation -------------------------------------------------------------------------------------------------------------------------
_CONT = [(v, ga, h, d) for v in ("e2e", "indi") for ga, h, d in ((1, 3, 1), (1, 2, 4))]           # H > d > 0, d > H


@pytest.mark.parametrize("variant,ga,H,d", _CONT, ids=["%s-ga%d-h%d-d%d" % c for c in _CONT])
def test_k_steps_equal_k_launches_of_one_step(variant, ga, H, d):
    from optimal_quad_control_rl_amd._closed_loop import rollout_outputs

    cog, sog = [0, 1], [0, 1]
    conds = [_cond(variant, 0), _cond(variant, 1)]
    a, b = (_handle(variant, 2 * E, ga, conds[0], env_id_base=BASE) for _ in range(2))
    W = a.state_len + 4 * H
    cbank, pol, dbank = _bank(variant, conds), _policy(variant, W), _dynamics_bank(variant, [None])
    sbank = _sensing_bank([_sensor(delay=d), _sensor(NOISY, d)])
    for e in (a, b):
        e.condition_reset(conds, cog, E)
        _force_rows(e, 2)
    ta, tb = _term(a, K, W), _term(b, 1, W)
    pa, pb = _pending(a), _pending(b)
    oa, ca, la = _fly_priv(a, pol, cbank, cog, dbank, sbank, sog, H, K, pa)
    ob = rollout_outputs(K, 2 * E, W, b.device)
    cb = torch.empty_like(ob[0])
    terms, last, clast = [], None, None
    for k in range(K):
        tb.fill_(SENTINEL)
        step, _, step_clast = _fly_priv(b, pol, cbank, cog, dbank, sbank, sog, H, 1, pb, first=FIRST + k,
                                        out=(ob[0][k:k + 1], cb[k:k + 1]) + tuple(t[k:k + 1] for t in ob[1:]))
        terms.append(tb[0].clone())
        if last is not None:
            assert torch.equal(_bits(last), _bits(ob[0][k])), ("last_obs of call %d is row 0 of call %d" % (k - 1, k))
            assert torch.equal(_bits(clast), _bits(cb[k])), ("critic_last_obs of call %d is row 0 of critic_obs of call %d" % (k - 1, k))
        last, clast = step[6], step_clast
    _every_env_ended(oa[4], "one call")
    m = max(d, H)
    assert FIRST < 2 ** 32 < FIRST + K and int(oa[5].sum()) >= 1 and bool(pa[:, 4 * (m - 1):4 * m].any()) and not bool(_bits(pa[:, 4 * m:]).any())
    for name, x, y in zip(NAMES[:6], oa, ob):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert torch.equal(_bits(oa[0]), _bits(ob[0])) and torch.equal(_bits(oa[6]), _bits(last)), "rows and last_obs"
    assert torch.equal(_bits(ca), _bits(cb)) and torch.equal(_bits(la), _bits(clast)), "clean rows and critic_last_obs"
    assert not torch.equal(ca[:, E:], oa[0][:, E:])
    assert torch.equal(_bits(ta), _bits(torch.stack(terms))) and int((ta[..., -1] != SENTINEL).sum()) == int(oa[4].sum()), "terminal rows"
    _same_state(a, b, "K launches")
    assert torch.equal(_bits(pa), _bits(pb)), "pending"
    for x in (a, b, cbank, pol, dbank, sbank):
        x.close()


# ---- 4. three groups, and the widest tile ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,ga,H", [("indi", 1, 2), ("e2e", 4, 0)], ids=["indi-ga1-h2", "e2e-ga4-h0-widest-tile"])
def test_three_groups_of_256(variant, ga, H):
    """768 envs = 3 groups x envs_per_group 256 (ideal, noisy + delay, delay alone): the group map is read per workgroup"""
    _twin_equality(variant, ga, H, "f16-operands", groups=3, sog=[0, 1, 2])


# ---- 5. refusals launch nothing --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from optimal_quad_control_rl_amd import _lib

    Kr, n, ga, H = 4, 2 * E, 1, 2
    cond = _cond("indi")
    env = _handle("indi", n, ga, cond)
    L, Lenv = env._L, env.state_len
    W = Lenv + 4 * H
    pol, own_len = _policy("indi", W), _policy("indi", Lenv)
    cbank, dbank = _bank("indi", [cond]), _dynamics_bank("indi", [None])
    sbank = _sensing_bank([_sensor(NOISY, 2), _sensor(delay=1)], capacity=3)          # slot 2 never set
    dev = env.device
    wide = Lenv + 16
    bufs = dict(obs=torch.full((Kr, n, wide), SENTINEL, device=dev), critic=torch.full((Kr, n, wide), SENTINEL, device=dev),
                act=torch.full((Kr, n, 4), SENTINEL, device=dev), logp=torch.full((Kr, n), SENTINEL, device=dev),
                rew=torch.full((Kr, n), SENTINEL, device=dev), done=torch.full((Kr, n), 7, dtype=torch.uint8, device=dev),
                trunc=torch.full((Kr, n), 7, dtype=torch.uint8, device=dev), last=torch.full((n, wide), SENTINEL, device=dev),
                clast=torch.full((n, wide), SENTINEL, device=dev), pend=torch.full((n, 16), SENTINEL, device=dev),
                term=torch.full((Kr, n, wide), SENTINEL, device=dev))
    env.set_terminal_obs_buffer(bufs["term"], obs_len=wide)
    before = env.get_state_tensors()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    h = lambda x: x._h if x is not None else None
    ip = lambda m: None if m is None else np.asarray(m, np.int32).ctypes.data_as(i32p)
    who = b"qr_rollout_policy_privileged"

    def call(p=pol, cb=cbank, db=dbank, sb=sbank, g=2, cog=(0, 0), dog=(0, 0), sog=(1, 0), hist=H, k=Kr, flags=0, first=0, pend=True, obs=True,
             critic=0, clast=0):
        cptr = None if critic is None else C.c_void_p(bufs["critic"].data_ptr() + critic)
        lptr = None if clast is None else C.c_void_p(bufs["clast"].data_ptr() + clast)
        return L.qr_rollout_policy_privileged(env._h, h(p), h(cb), h(db), h(sb), g, E, ip(cog), ip(dog), ip(sog), hist, k, LOG_STD.ctypes.data_as(f32p), 3,
                                              first, flags, _ptr(bufs["pend"]) if pend else None, _ptr(bufs["obs"]) if obs else None, cptr,
                                              _ptr(bufs["act"]), _ptr(bufs["logp"]), _ptr(bufs["rew"]), _ptr(bufs["done"]), _ptr(bufs["trunc"]),
                                              _ptr(bufs["last"]), lptr, env._stream())

    def untouched():
        torch.cuda.synchronize()
        for name, t in bufs.items():
            assert bool((t == (SENTINEL if t.dtype == torch.float32 else 7)).all()), name
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    def refused(code, message, **kw):
        rc = call(**kw)
        err = L.qr_last_error()
        assert rc == code, (list(kw.keys()), rc, err)
        assert who in err and message in err, err
        untouched()

    # the two new pointers: directly behind the check of obs_out_dev and its neighbours, ahead of everything about the policy
    refused(_lib.QR_E_INVALID, b"obs/act/logp/rew/done buffers are required", obs=False, critic=None)
    refused(_lib.QR_E_INVALID, b"critic_obs_out_dev is required", critic=None, p=own_len, hist=7)
    refused(_lib.QR_E_INVALID, b"must be 16-byte aligned", critic=4, p=own_len, hist=7)
    refused(_lib.QR_E_INVALID, b"must be 16-byte aligned", clast=8, sb=None)
    # the range of history starts at 0 here, and is refused where the history call refuses its own
    for bad in (-1, 5 - ga, 5):
        refused(_lib.QR_E_INVALID, b"history must be in [0, 4 - gates_ahead]", hist=bad)
    refused(_lib.QR_E_INVALID, b"history must be in", hist=-1, sb=None)
    refused(_lib.QR_E_INVALID, b"bad argument", k=0, hist=-1)
    refused(_lib.QR_E_INVALID, b"policy obs_len != env obs_len + 4 * history", p=own_len)
    refused(_lib.QR_E_INVALID, b"policy obs_len != env obs_len + 4 * history", hist=0)
    # the twin's refusals, spot-checked in its order
    refused(_lib.QR_E_INVALID, b"null condition bank", cb=None, db=None, sb=None)
    refused(_lib.QR_E_INVALID, b"null sensing bank", sb=None, pend=False)
    refused(_lib.QR_E_INVALID, b"sensing_of_group[0] is outside the sensing bank", sog=(3, 0))
    refused(_lib.QR_E_INVALID, b"2^56", first=2 ** 64 - 1, sog=(2, 0))
    refused(_lib.QR_E_STATE, b"slot 2 of the sensing bank was never set", sog=(2, 0))
    refused(_lib.QR_E_INVALID, b"pending_dev is required", pend=False)
    # ... and valid calls run: H = 2 with both pointers, H = 0 with critic_last_obs_dev = NULL
    bufs["pend"].zero_()
    assert call() == _lib.QR_OK, L.qr_last_error()
    torch.cuda.synchronize()
    assert bool((bufs["critic"].view(-1)[:Kr * n * W] != SENTINEL).all()) and bool((bufs["clast"].view(-1)[:n * W] != SENTINEL).all())
    assert bool((bufs["critic"].view(-1)[Kr * n * W:] == SENTINEL).all()) and bool((bufs["clast"].view(-1)[n * W:] == SENTINEL).all()), "nothing past the rows"
    env.set_terminal_obs_buffer(None)
    bufs["clast"].fill_(SENTINEL); bufs["critic"].fill_(SENTINEL); bufs["pend"].zero_()
    assert call(p=own_len, hist=0, clast=None) == _lib.QR_OK, L.qr_last_error()
    torch.cuda.synchronize()
    assert bool((bufs["clast"] == SENTINEL).all()) and bool((bufs["critic"].view(-1)[:Kr * n * Lenv] != SENTINEL).all())
    assert bool((bufs["critic"].view(-1)[Kr * n * Lenv:] == SENTINEL).all())
    for x in (env, pol, own_len, cbank, dbank, sbank):
        x.close()


# ---- 6. time, printed ------------------------------------------------------------------------------------------------------------------------
def test_privileged_launch_time_is_printed():
    """Median us per step of the privileged launch against its twin qr_rollout_policy_history at (gates_ahead 1, H 2): ideal slots, the NOISY
    sigmas, NOISY + d = 4, both precisions.  N = 65 536 = 256 groups x 256 envs, K = 200, E2E + residual MLPs + training disturbances, square
    track, nominal vehicles.  Launches alternate from the same seeded reset in ORDER-SWAPPED pairs, one warm-up pair, medians of 6, host clock
    around a stream synchronise.  The launch writes 4 L' more bytes per env-step and nothing else is added; NO bound is asserted: nobody had
    measured it when the test was written (DESIGN.md section 8 and profiles/privileged_critic_time.txt hold the numbers of one run)."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd._closed_loop import rollout_outputs
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    n, Kc, H = 65536, 200, 2
    groups = n // E
    envs = {}
    for name in ("privileged", "history"):
        env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=99)
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        envs[name] = (env, _bank("e2e", [Condition.from_env(env)]), _pending(env))
    W = envs["history"][0].state_len + 4 * H
    dbank = _dynamics_bank("e2e", [None])
    sbank = _sensing_bank([None, _sensor(NOISY, 0), _sensor(NOISY, 4)])
    torch.manual_seed(0)
    pol = MfmaPolicy(W).load_torch(ActorCritic(W, 4).pi)
    dev = envs["history"][0].device
    out = rollout_outputs(Kc, n, W, dev)
    out_priv = (out[0], torch.empty_like(out[0])) + tuple(out[1:])
    log_std, zero = np.zeros(4, np.float32), [0] * groups
    stream = torch.cuda.current_stream(dev)

    def timed(name, launch):
        env, _, pend = envs[name]
        env.seed(99); env.reset_device()
        pend.zero_()
        stream.synchronize()
        t0 = time.perf_counter()
        launch()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / Kc

    ep, cp, pp = envs["privileged"]
    eh, ch, ph = envs["history"]
    for precision in ("f16-operands", "f32"):
        for label, slot in (("ideal slots", 0), ("noise on", 1), ("noise on, d = 4", 2)):
            sog = [slot] * groups
            priv = lambda: ep.rollout_policy_privileged_device(pol, cp, zero, dbank, zero, sbank, sog, H, E, Kc, log_std, pp, noise_seed=1, out=out_priv,
                                                               precision=precision)
            hist = lambda: eh.rollout_policy_history_device(pol, ch, zero, dbank, zero, sbank, sog, H, E, Kc, log_std, ph, noise_seed=1, out=out,
                                                            precision=precision)
            t_p, t_h = [], []
            for rep in range(7):
                if rep % 2 == 0:
                    a = timed("privileged", priv); b = timed("history", hist)
                else:
                    b = timed("history", hist); a = timed("privileged", priv)
                if rep:
                    t_p.append(a); t_h.append(b)
            mp, mh = statistics.median(t_p), statistics.median(t_h)
            print("rollout, %s, %s: privileged (gates_ahead 1, H 2) median %.4f us/step %s; history median %.4f us/step %s; ratio %.4f"
                  % (precision, label, mp, ["%.3f" % t for t in t_p], mh, ["%.3f" % t for t in t_h], mp / mh))
            assert mp > 0.0 and mh > 0.0
    for env, cb, _ in envs.values():
        env.close(); cb.close()
    dbank.close(); sbank.close(); pol.close()
