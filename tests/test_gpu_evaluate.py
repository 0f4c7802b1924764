"""GPU: the on-device evaluator (qr_evaluate_policy, eval_policy_kernel<V, GA, kF32>) against the accounting specification
(tests/eval_spec.py) applied to a per-step loop through the C ABI on a twin handle:

    K x [ qr_policy_forward(_f32class) -> clip -> qr_step -> qr_get_state (target gate) ]

Integer records equal, float records bit-equal, env state bit-equal afterwards -- no tolerance anywhere (tests/test_gpu_policy.py
already establishes that the closed-loop kernels are bit-identical to this loop).  The scenario (eval_spec.SCENARIO: straight track
of 16 gates 0.4 m apart, time limit 250, 600 steps, a constant action from a zero-weight policy with an output bias) is shown on the
CPU oracle to produce passes, laps in every slot, crashes and time-limit ends (tests/test_eval_spec.py); the same conditions are
asserted here on the reference loop's own data, so a vacuous comparison fails instead of passing."""

import numpy as np
import pytest
import torch

import eval_spec as S
from eval_helpers import SENTINEL, _closed_loop_policy, _constant_policy, _env, _ptr, _records

pytestmark = pytest.mark.gpu

SC = S.SCENARIO


def _target(env, out):
    from optimal_quad_control_rl_amd import _lib

    _lib.check(env._L.qr_get_state(env._h, None, None, _ptr(out), None, None, env._stream()))


def _reference_loop(env, pol, K, precision):
    """The per-step loop on a twin handle; returns host arrays [K, n]: target before / after, done, trunc, reward."""
    n, dev = env.num_envs, env.device
    tb = torch.empty((K, n), dtype=torch.int32, device=dev)
    ta = torch.empty((K, n), dtype=torch.int32, device=dev)
    dn = torch.empty((K, n), dtype=torch.uint8, device=dev)
    tr = torch.empty((K, n), dtype=torch.uint8, device=dev)
    rw = torch.empty((K, n), dtype=torch.float32, device=dev)
    prev = torch.empty(n, dtype=torch.int32, device=dev)
    _target(env, prev)
    obs = env.states_tensor
    for k in range(K):
        act = pol.forward(obs.contiguous(), precision=precision).clamp(-1, 1).contiguous()
        obs, r, d, t = env.step_device(act)
        rw[k].copy_(r); dn[k].copy_(d); tr[k].copy_(t)
        tb[k].copy_(prev)
        _target(env, ta[k])
        prev = ta[k]
    return [x.cpu().numpy() for x in (tb, ta, dn, tr, rw)]


def _states_equal(a, b):
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), a.get_state_tensors(), b.get_state_tensors()):
        assert x is None or torch.equal(x, y), name


def _assert_equal_records(rec, recf, srec, srecf):
    rec, recf = rec.cpu().numpy(), recf.cpu().numpy()
    bad = np.nonzero((rec != srec).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], rec[bad[:2]], srec[bad[:2]])
    badf = np.nonzero((recf.view(np.uint32) != srecf.view(np.uint32)).any(axis=1))[0]
    assert badf.size == 0, (badf.size, badf[:5], recf[badf[:2]], srecf[badf[:2]])


_CASES = [(v, g, n, p) for v in ("e2e", "indi") for g in (0, 1) for n in (4096, 4096 + 37, 65536) for p in ("f16-operands", "f32")]


@pytest.mark.parametrize("variant,gates_ahead,n,precision", _CASES, ids=["%s-ga%d-n%d-%s" % c for c in _CASES])
def test_records_equal_the_spec(variant, gates_ahead, n, precision):
    K, gpl = SC["steps"], SC[variant + "_gates_per_lap"]
    a, b = _env(variant, n, gates_ahead), _env(variant, n, gates_ahead)
    pol = _constant_policy(a.state_len, SC[variant + "_action"])
    rec, recf = _records(a)
    a.evaluate_device(pol, K, gpl, rec, recf, precision=precision)
    seq = _reference_loop(b, pol, K, precision)
    srec, srecf = S.run(*S.new_records(n), *seq, gates_per_lap=gpl)
    nv = S.nonvacuous_e2e(srec) if variant == "e2e" else S.nonvacuous_indi(srec)
    print(variant, gates_ahead, n, precision, nv, "passes", int(srec[:, 0].sum()))
    assert nv["ok"], nv                                   # the reference loop's own data exercises the record
    _assert_equal_records(rec, recf, srec, srecf)
    assert bool((rec[:, 22:] == 0).all()) and bool((recf[:, 3] == 0).all()) and bool((rec[:, 5] == K).all())
    _states_equal(a, b)
    assert torch.equal(a.states_tensor, b.states_tensor)  # the Python wrapper refreshed its observation buffer
    a.close(); b.close(); pol.close()


_CLOSED = [("indi", 0, 4096 + 37, "f32"), ("e2e", 1, 4096 + 37, "f32"), ("indi", 1, 4096, "f16-operands"), ("e2e", 0, 4096, "f16-operands")]
# every other instantiation of eval_policy_kernel<variant, gates_ahead, f32class>, at the ragged size
_CLOSED += [(v, g, 4096 + 37, p) for v in ("e2e", "indi") for g in (2, 3, 4) for p in ("f16-operands", "f32")]


@pytest.mark.parametrize("variant,gates_ahead,n,precision", _CLOSED, ids=["%s-ga%d-n%d-%s" % c for c in _CLOSED])
def test_records_equal_the_spec_with_an_observation_dependent_policy(variant, gates_ahead, n, precision):
    """The same comparison with weights that make the action depend on the observation: a stale or mis-laid observation, or a wrong
    low-piece image in the f32-class forward, changes the actions and with them records and states."""
    _records_equal_the_spec_closed_loop(variant, gates_ahead, n, precision)


def _records_equal_the_spec_closed_loop(variant, gates_ahead, n, precision, K=SC["steps"], gpl=None, track=None, prepare=None,
                                        max_steps=SC["max_steps"], nonvacuous=None):
    """`track`, `prepare(env)`, `max_steps`, `K`, `gpl`: another track, start, time limit, window and lap length than the scenario's
    (tests/test_gpu_table_edges.py); `nonvacuous(srec)` replaces the scenario's own non-vacuity condition.  Returns the spec's records."""
    gpl = SC[variant + "_gates_per_lap"] if gpl is None else gpl
    a, b = _env(variant, n, gates_ahead, track=track, max_steps=max_steps), _env(variant, n, gates_ahead, track=track, max_steps=max_steps)
    if prepare is not None:
        prepare(a); prepare(b)
    pol = _closed_loop_policy(a.state_len, SC[variant + "_action"])
    o0 = a.states_tensor.clone()
    act0 = pol.forward(o0, precision=precision)
    assert float((act0 - act0.mean(dim=0)).abs().max()) > 1e-3          # the actions do differ from env to env
    rec, recf = _records(a)
    a.evaluate_device(pol, K, gpl, rec, recf, precision=precision)
    seq = _reference_loop(b, pol, K, precision)
    srec, srecf = S.run(*S.new_records(n), *seq, gates_per_lap=gpl)
    if nonvacuous is None:
        nv = S.nonvacuous_e2e(srec) if variant == "e2e" else S.nonvacuous_indi(srec)
        print("closed loop", variant, gates_ahead, n, precision, nv, "passes", int(srec[:, 0].sum()))
        assert nv["ok"], nv
    else:
        nonvacuous(srec)
    _assert_equal_records(rec, recf, srec, srecf)
    _states_equal(a, b)
    final_target = a.get_state_tensors()[2].cpu().numpy()
    a.close(); b.close(); pol.close()
    return srec, final_target


@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_same_end_state_as_the_rollout_kernel(variant, precision):
    """After qr_evaluate_policy the env is where qr_rollout_policy(..., QR_ROLLOUT_DETERMINISTIC) with the same K leaves a twin."""
    n, K = 4096 + 37, 300
    a, b = _env(variant, n, 1), _env(variant, n, 1)
    pol = _constant_policy(a.state_len, SC[variant + "_action"])
    rec, recf = _records(a)
    a.evaluate_device(pol, K, 2, rec, recf, precision=precision)
    out = b.rollout_policy_device(pol, K, torch.zeros(4), deterministic=True, precision=precision)
    done, trunc = out[4].bool(), out[5].bool()
    assert int((done & ~trunc).sum()) > 0 and (variant == "e2e" or int(trunc.sum()) > 0)   # (the E2E scenario crashes before any time limit)
    _states_equal(a, b)
    # ... and the records agree with what the rollout rows say
    assert int(rec[:, 1].sum()) == int((done & ~trunc).sum()) and int(rec[:, 2].sum()) == int(trunc.sum())
    a.close(); b.close(); pol.close()


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_one_call_equals_two_with_the_records_carried_over(variant):
    n, gpl = 4096 + 37, SC[variant + "_gates_per_lap"]
    a, b = _env(variant, n, 1), _env(variant, n, 1)
    pol = _constant_policy(a.state_len, SC[variant + "_action"])
    ra, rfa = _records(a)
    rb, rfb = _records(b)
    a.evaluate_device(pol, 600, gpl, ra, rfa)
    b.evaluate_device(pol, 250, gpl, rb, rfb)
    first = rb.clone()
    b.evaluate_device(pol, 350, gpl, rb, rfb)
    assert bool((first[:, 5] == 250).all()) and int(ra[:, 14:22].sum()) > int(first[:, 14:22].sum()) > 0
    assert torch.equal(ra, rb) and torch.equal(rfa.view(torch.int32), rfb.view(torch.int32))
    _states_equal(a, b)
    a.close(); b.close(); pol.close()


def test_argument_errors_launch_nothing():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    n, K = 300, 8
    env = _env("indi", n, 1)
    L = env._L
    pol = _constant_policy(env.state_len, SC["indi_action"])
    other_len = MfmaPolicy(env.state_len + 4)
    rec = torch.full((n, S.REC_INTS), 7, dtype=torch.int32, device=env.device)
    recf = torch.full((n, S.REC_FLOATS), SENTINEL, dtype=torch.float32, device=env.device)
    before = env.get_state_tensors()

    def call(e=env, p=pol, k=K, gpl=2, flags=0, r=rec, rf=recf):
        return L.qr_evaluate_policy(e._h, p._h if p is not None else None, k, gpl, flags, _ptr(r), _ptr(rf), e._stream())

    def refused(code, **kw):
        rc = call(**kw)
        assert rc == code, (kw.keys(), rc)
        assert len(L.qr_last_error()) > 0
        torch.cuda.synchronize()
        assert bool((rec == 7).all()) and bool((recf == SENTINEL).all())
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    refused(_lib.QR_E_INVALID, r=None)
    refused(_lib.QR_E_INVALID, k=0)
    refused(_lib.QR_E_INVALID, k=-3)
    refused(_lib.QR_E_INVALID, gpl=0)
    refused(_lib.QR_E_INVALID, flags=1)          # QR_ROLLOUT_DETERMINISTIC is not a flag of this call
    refused(_lib.QR_E_INVALID, flags=4)
    refused(_lib.QR_E_INVALID, flags=2 | 8)
    refused(_lib.QR_E_INVALID, p=other_len)
    refused(_lib.QR_E_INVALID, p=None)
    no_weights = MfmaPolicy(env.state_len)
    refused(_lib.QR_E_STATE, p=no_weights)
    no_weights.close()
    # records that are not 16-byte aligned (the kernel moves them in 16-byte pieces)
    big = torch.full((n * S.REC_INTS + 4,), 7, dtype=torch.int32, device=env.device)
    bigf = torch.full((n * S.REC_FLOATS + 4,), SENTINEL, dtype=torch.float32, device=env.device)
    refused(_lib.QR_E_INVALID, r=big[1:])
    refused(_lib.QR_E_INVALID, rf=bigf[2:])
    assert bool((big == 7).all()) and bool((bigf == SENTINEL).all())
    env.pause = True
    refused(_lib.QR_E_STATE)
    env.pause = False
    env.pause_if_collision = True
    refused(_lib.QR_E_STATE)
    env.pause_if_collision = False
    # a track with one gate: a pass cannot move the target
    gp, gy, sp = S.scenario_track()
    one = _env("indi", n, 1, track=(gp[:1], gy[:1], sp))
    rc = call(e=one)
    assert rc == _lib.QR_E_INVALID and b"one gate" in L.qr_last_error()
    torch.cuda.synchronize()
    assert bool((rec == 7).all()) and bool((recf == SENTINEL).all())
    one.close()
    # a registered terminal-observation buffer is left alone by a call that runs (envs do finish: time limit 5)
    env.max_steps = 5
    tb = torch.full((K, n, env.state_len), SENTINEL, device=env.device)
    env.set_terminal_obs_buffer(tb)
    rec.zero_(); recf.zero_()
    assert call(flags=2) == _lib.QR_OK and call(rf=None) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((tb == SENTINEL).all())
    assert bool((rec[:, 5] == 2 * K).all()) and int(rec[:, 2].sum()) >= n
    assert env.last_rollout_ms() > 0.0           # qr_last_step_many_ms reports the launch
    env.close(); pol.close(); other_len.close()


def test_python_evaluate_policy_equals_the_spec():
    """evaluate_policy(model, env, ...) on an untrained SB3-shaped PPO: two launches, summaries of the window and of the whole."""
    from optimal_quad_control_rl_amd import (PPO, Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, VecMonitor, evaluate_policy, square_track,
                                             summarize_eval)
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    trk = square_track()
    train = VecMonitor(Quadcopter3DGates(256, *trk, gates_ahead=1, seed=1))
    train.venv.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    model = PPO("MlpPolicy", train, policy_kwargs=dict(activation_fn=torch.nn.ReLU, net_arch=[dict(pi=[120] * 3, vf=[120] * 3)], log_std_init=0),
                n_steps=8, batch_size=256, n_epochs=1, seed=3)
    with torch.no_grad():
        model._net.pi[-1].bias.copy_(torch.tensor([0.25, 0.2, 0.25, 0.2]))   # untrained, but not falling straight down
    n, K, W = 4096, 600, 250
    ev = VecMonitor(_env("e2e", n, 1, seed=99, track=trk))
    res = evaluate_policy(model, ev, n_eval_steps=K, window_steps=W, seed=99)
    twin = _env("e2e", n, 1, seed=99, track=trk)
    pol = MfmaPolicy(twin.state_len).load_torch(model._net.pi)
    seq = _reference_loop(twin, pol, K, "f16-operands")
    rec, recf = S.new_records(n)
    S.run(rec, recf, *[x[:W] for x in seq], gates_per_lap=4)
    window = summarize_eval(rec, recf, twin.dt, 4)
    S.run(rec, recf, *[x[W:] for x in seq], gates_per_lap=4)
    total = summarize_eval(rec, recf, twin.dt, 4)
    print("window", res["window"], "\ntotal", res["total"])
    assert total["episodes"] > 0 and total["steps"] == K and window["steps"] == W
    assert res["total"] == total
    assert {k: v for k, v in res["window"].items() if k not in ("crashes_per_window", "gates_per_window")} == window
    assert res["window"]["crashes_per_window"] == window["crashes"] / n and res["window"]["gates_per_window"] == window["gates"] / n
    _states_equal(ev.venv, twin)
    # the native trainer is accepted as well, and gives the same answer for the same weights
    res2 = evaluate_policy(model._trainer, ev, n_eval_steps=K, window_steps=W, seed=99)
    assert res2 == res
    ev.venv.close(); twin.close(); pol.close(); train.venv.close()


@pytest.mark.parametrize("n", [65536, 4096])
def test_not_slower_than_the_rollout_kernel(n):
    """The evaluator does a strict subset of qr_rollout_policy's work per step, so it must not be slower: median us/step of 5 launches
    <= 1.03 x the rollout kernel's (3 % = the run-to-run spread DESIGN section 5 states for these kernels).  K = 2 000, E2E + residual
    MLPs + training disturbances, square track, f16 operands; the two kernels alternate from the same seeded start with the same seeded
    network, one warm-up pair first, times from qr_last_step_many_ms.  (tools/bench_evaluate.py is the same protocol with raw runs.)"""
    import statistics

    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    K = 2000
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=99)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = 10 ** 6
    torch.manual_seed(0)
    pol = MfmaPolicy(env.state_len).load_torch(ActorCritic(env.state_len, 4).pi)
    rec, recf = _records(env)
    dev = env.device
    out = (torch.empty((K, n, env.state_len), device=dev), torch.empty((K, n, 4), device=dev), torch.empty((K, n), device=dev),
           torch.empty((K, n), device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev))
    t_eval, t_roll = [], []
    for rep in range(6):
        env.seed(99); env.reset_device(); rec.zero_(); recf.zero_()
        env.evaluate_device(pol, K, 4, rec, recf)
        ms_e = env.last_rollout_ms()
        env.seed(99); env.reset_device()
        env.rollout_policy_device(pol, K, torch.zeros(4), deterministic=True, out=out)
        ms_r = env.last_rollout_ms()
        if rep:
            t_eval.append(ms_e * 1e3 / K); t_roll.append(ms_r * 1e3 / K)
    me, mr = statistics.median(t_eval), statistics.median(t_roll)
    print("n %d: qr_evaluate_policy %s -> median %.4f us/step; qr_rollout_policy %s -> median %.4f us/step; ratio %.4f"
          % (n, ["%.4f" % t for t in t_eval], me, ["%.4f" % t for t in t_roll], mr, me / mr))
    del out
    env.close(); pol.close()
    assert me <= 1.03 * mr, (me, mr, me / mr)
