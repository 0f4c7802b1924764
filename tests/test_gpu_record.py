"""GPU: the on-device flight recorder (qr_record_policy, record_policy_kernel<V, GA, kF32>).  Every comparison is EQUALITY -- floats bit
for bit, no tolerance, no allowance of differing rows:

  1. against qr_rollout_policy on a twin handle with identical arguments (command = clip(act), reward, end code, env state afterwards);
  2. against the per-step path: a twin teacher-forced with those clipped actions through K x [qr_get_state, qr_step] (world, target,
     step-count columns = the states read before each step);
  3. against qr_evaluate_policy on a third twin (passes, crashes, time-limit ends derived from the rows);
  4. rec_envs, 5. splitting a call, 6. argument errors, 7. the Python level, 8. time against the rollout kernel.

Scenario: the evaluator's (tests/eval_spec.py: straight track of 16 gates 0.4 m apart, constant action, seed 5), 300 steps.  INDI keeps
its time limit of 250; E2E with that limit crashes before any time-limit end (tests/test_gpu_evaluate.py notes the same), and on the
CPU oracle 1 024 E2E envs give 196 passes / 2 976 crashes / 491 time-limit ends at a limit of 100 (0 time-limit ends at 250, 24 at 150), so
E2E flies with 100.  Every test asserts that its own window holds passes, crashes and time-limit ends before it compares anything."""
import ctypes as C
import statistics

import numpy as np
import pytest
import torch

import eval_spec as S

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
SC = S.SCENARIO
K_WIN = 300
MAX_STEPS = {"e2e": 100, "indi": SC["max_steps"]}
STOCH = dict(log_std=(-1.5, -1.2, -1.5, -1.2), noise_seed=7, first_step=12345)   # std 0.22 .. 0.30 around the scenario's action


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _env(variant, n, gates_ahead, seed=SC["seed"], track=None, max_steps=None):
    from optimal_quad_control_rl_amd import Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES

    trk = S.scenario_track() if track is None else track
    if variant == "e2e":
        env = Quadcopter3DGates(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none")   # residual MLPs: the default
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    else:
        env = Quadcopter3DGatesINDI(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none")
    env.max_steps = MAX_STEPS[variant] if max_steps is None else max_steps
    env.reset_device()
    return env


def _policy(obs_len, action, seed=3, gain=5.0):
    """seeded random weights around the scenario's action (tests/test_gpu_evaluate.py::_closed_loop_policy): every action depends on the
    observation the kernel fed to its forward"""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(seed)
    net = ActorCritic(obs_len, 4)
    with torch.no_grad():
        net.pi[-1].weight.mul_(gain)
        net.pi[-1].bias.copy_(torch.as_tensor(action, dtype=torch.float32))
    return MfmaPolicy(obs_len).load_torch(net.pi)


def _mode(stochastic):
    if stochastic:
        return dict(log_std=torch.tensor(STOCH["log_std"]), noise_seed=STOCH["noise_seed"], first_step=STOCH["first_step"], deterministic=False)
    return dict(log_std=torch.zeros(4), noise_seed=0, first_step=0, deterministic=True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _equal_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = (a != b)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


def _states_equal(a, b):
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), a.get_state_tensors(), b.get_state_tensors()):
        if x is not None:
            _equal_bits(x, y, name)   # (float tensors bit for bit: torch.equal would let -0.0 pass for 0.0 and fail on equal NaNs)


def _cols(rows, s):
    return dict(world=rows[:, :, :s], command=rows[:, :, s:s + 4], reward=rows[:, :, s + 4], end=rows[:, :, s + 5], target=rows[:, :, s + 6],
                steps=rows[:, :, s + 7])


def _counts_from_rows(rows, s, final_target):
    """per-env passes / crashes / time-limit ends by the evaluator's definitions: a pass is a step that does not end the episode and
    after which the target gate differs (next row's target; after the last row: the env's target)"""
    c = _cols(rows, s)
    after = torch.cat([c["target"][1:], final_target.to(torch.float32)[None, :rows.shape[1]]], dim=0)
    passes = ((c["end"] == 0) & (after != c["target"])).sum(dim=0)
    return torch.stack([passes, (c["end"] == 1).sum(dim=0), (c["end"] == 2).sum(dim=0)], dim=1)


def _assert_window_is_not_vacuous(rows, s, final_target, what):
    cnt = _counts_from_rows(rows, s, final_target).sum(dim=0).tolist()
    print(what, "passes / crashes / time-limit ends in the window:", cnt)
    assert cnt[0] >= 1 and cnt[1] >= 1 and cnt[2] >= 1, (what, cnt)
    return cnt


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. against the rollout kernel
# ---------------------------------------------------------------------------------------------------------------------------------
_CASES = [(v, g, n, p, st) for v in ("e2e", "indi") for g in (0, 1) for n in (4096, 4096 + 37, 65536) for p in ("f16-operands", "f32")
          for st in (False, True)]
# every other instantiation of record_policy_kernel<variant, gates_ahead, f32class>, at the ragged size
_CASES += [(v, g, 4096 + 37, p, True) for v in ("e2e", "indi") for g in (2, 3, 4) for p in ("f16-operands", "f32")]

@pytest.mark.parametrize("variant,gates_ahead,n,precision,stochastic", _CASES,
                         ids=["%s-ga%d-n%d-%s-%s" % (c[0], c[1], c[2], c[3], "stoch" if c[4] else "det") for c in _CASES])
def test_rows_equal_the_rollout_kernel(variant, gates_ahead, n, precision, stochastic):
    _rows_equal_the_rollout_kernel(variant, gates_ahead, n, precision, stochastic)


def _rows_equal_the_rollout_kernel(variant, gates_ahead, n, precision, stochastic, K=K_WIN, track=None, prepare=None, max_steps=None,
                                   nonvacuous=_assert_window_is_not_vacuous):
    """`track`, `prepare(env)`, `max_steps`, `K`: another track, start, time limit and window than the scenario's
    (tests/test_gpu_table_edges.py); `nonvacuous(rows, s, final_target, what)` asserts that the window holds what the caller needs.
    Returns the rows and the final targets."""
    r, a = _env(variant, n, gates_ahead, track=track, max_steps=max_steps), _env(variant, n, gates_ahead, track=track, max_steps=max_steps)
    if prepare is not None:
        prepare(r); prepare(a)
    pol = _policy(r.state_len, SC[variant + "_action"])
    s, mode = r.STATE_LEN, _mode(stochastic)
    assert r._L.qr_record_row_len(r._h) == s + 8
    world0, _, target0, steps0, _ = r.get_state_tensors()
    rows = r.record_policy_device(pol, K, precision=precision, **mode)
    assert tuple(rows.shape) == (K, n, s + 8) and rows.dtype == torch.float32
    obs, act, logp, rew, done, trunc, _ = a.rollout_policy_device(pol, K, precision=precision, **mode)
    c = _cols(rows, s)
    final_target = r.get_state_tensors()[2]
    nonvacuous(rows, s, final_target, "%s ga%d n%d %s %s" % (variant, gates_ahead, n, precision, stochastic))
    _equal_bits(c["command"], act.clamp(-1.0, 1.0), "command = clip(action)")
    if stochastic:
        assert int((act.abs() > 1.0).sum()) > 0                       # the clip is exercised: rows hold the command, not the sample
    _equal_bits(c["reward"], rew, "reward")
    end = torch.where(trunc.bool(), 2.0, torch.where(done.bool(), 1.0, 0.0)).to(torch.float32)
    _equal_bits(c["end"], end, "end code")
    _states_equal(r, a)
    # the first row is the state the call started from
    _equal_bits(c["world"][0], world0, "world of row 0")
    assert torch.equal(c["target"][0], target0.float()) and torch.equal(c["steps"][0], steps0.float())
    assert torch.equal(r.states_tensor, a.states_tensor)                # the wrapper refreshed its observation buffer
    r.close(); a.close(); pol.close()
    return rows, final_target


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. against the per-step path
# ---------------------------------------------------------------------------------------------------------------------------------
_STEP_CASES = [("e2e", 1, 4096 + 37, "f16-operands", True), ("indi", 1, 4096 + 37, "f16-operands", True), ("e2e", 0, 4096, "f32", False),
               ("indi", 0, 4096, "f32", False)]


@pytest.mark.parametrize("variant,gates_ahead,n,precision,stochastic", _STEP_CASES,
                         ids=["%s-ga%d-n%d-%s-%s" % (c[0], c[1], c[2], c[3], "stoch" if c[4] else "det") for c in _STEP_CASES])
def test_state_columns_equal_the_per_step_path(variant, gates_ahead, n, precision, stochastic):
    K = K_WIN
    r, a, b = (_env(variant, n, gates_ahead) for _ in range(3))
    pol = _policy(r.state_len, SC[variant + "_action"])
    s, mode = r.STATE_LEN, _mode(stochastic)
    rows = r.record_policy_device(pol, K, precision=precision, **mode)
    act = a.rollout_policy_device(pol, K, precision=precision, **mode)[1]
    u = act.clamp(-1.0, 1.0).contiguous()
    world = torch.empty((K, n, s), device=r.device)
    target = torch.empty((K, n), dtype=torch.int32, device=r.device)
    steps = torch.empty((K, n), dtype=torch.int32, device=r.device)
    from optimal_quad_control_rl_amd import _lib
    for k in range(K):   # teacher-forced: the state read BEFORE each step, then the step with the recorded command
        _lib.check(b._L.qr_get_state(b._h, _ptr(world[k]), None, _ptr(target[k]), _ptr(steps[k]), None, b._stream()))
        b.step_device(u[k])
    c = _cols(rows, s)
    _assert_window_is_not_vacuous(rows, s, r.get_state_tensors()[2], "per-step %s ga%d" % (variant, gates_ahead))
    _equal_bits(c["world"], world, "world columns")
    assert torch.equal(c["target"], target.float()), "target column"
    assert torch.equal(c["steps"], steps.float()), "step-count column"
    assert int((c["steps"] == 0).sum()) > n                            # episodes do begin inside the window
    _states_equal(r, b)
    for e in (r, a, b):
        e.close()
    pol.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. against the evaluator
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_counts_from_the_rows_equal_the_evaluator(variant, precision):
    n, K = 4096 + 37, K_WIN
    r, e = _env(variant, n, 1), _env(variant, n, 1)
    pol = _policy(r.state_len, SC[variant + "_action"])
    rows = r.record_policy_device(pol, K, torch.zeros(4), deterministic=True, precision=precision)
    rec = torch.zeros((n, S.REC_INTS), dtype=torch.int32, device=e.device)
    e.evaluate_device(pol, K, SC[variant + "_gates_per_lap"], rec, None, precision=precision)
    final_target = r.get_state_tensors()[2]
    _assert_window_is_not_vacuous(rows, r.STATE_LEN, final_target, "evaluator %s %s" % (variant, precision))
    cnt = _counts_from_rows(rows, r.STATE_LEN, final_target)
    assert torch.equal(cnt, rec[:, 0:3].long()), (cnt - rec[:, 0:3].long()).abs().sum(dim=0).tolist()
    _states_equal(r, e)
    # FlightRecord agrees, with and without the target after the last step (without it the last step cannot show a pass)
    from optimal_quad_control_rl_amd import FlightRecord
    fr = FlightRecord(rows, r.dt, final_target)
    assert np.array_equal(fr.counts(), rec[:, 0:3].cpu().numpy().astype(np.int64))
    open_end = FlightRecord(rows, r.dt).counts()
    last_pass = ((rows[-1, :, r.STATE_LEN + 5] == 0) & (final_target.float() != rows[-1, :, r.STATE_LEN + 6])).cpu().numpy()
    assert np.array_equal(open_end[:, 0] + last_pass, fr.counts()[:, 0]) and np.array_equal(open_end[:, 1:], fr.counts()[:, 1:])
    r.close(); e.close(); pol.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. rec_envs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("stochastic", [False, True])
def test_rec_envs_cuts_the_record_not_the_flight(variant, stochastic):
    n, K, tail = 4096 + 37, K_WIN, 4096
    full = _env(variant, n, 1)
    pol = _policy(full.state_len, SC[variant + "_action"])
    s, mode = full.STATE_LEN, _mode(stochastic)
    R = s + 8
    rows = full.record_policy_device(pol, K, **mode)
    _assert_window_is_not_vacuous(rows[:, :100], s, full.get_state_tensors()[2], "rec_envs %s first 100" % variant)
    for m in (100, n - 1, n - 2, 64, 1):    # n - 1 = 4132 is a multiple of 4, n - 2 is not: INDI rows of 84 bytes take both store paths
        cut = _env(variant, n, 1)
        flat = torch.full((K * m * R + tail,), SENTINEL, dtype=torch.float32, device=cut.device)
        out = flat[:K * m * R].view(K, m, R)
        got = cut.record_policy_device(pol, K, rec_envs=m, out=out, **mode)
        assert got.data_ptr() == flat.data_ptr()
        _equal_bits(got, rows[:, :m], "rows of the first %d envs" % m)
        assert bool((flat[K * m * R:] == SENTINEL).all()), "memory behind [K][M][R] was written (M = %d)" % m
        _states_equal(cut, full)
        cut.close()
    full.close(); pol.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. splitting
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_one_call_equals_two_with_first_step_advanced(variant):
    n, K, K1 = 4096 + 37, K_WIN, 120
    a, b = _env(variant, n, 1), _env(variant, n, 1)
    pol = _policy(a.state_len, SC[variant + "_action"])
    mode = _mode(True)
    whole = a.record_policy_device(pol, K, **mode)
    first = b.record_policy_device(pol, K1, **mode)
    second = b.record_policy_device(pol, K - K1, **dict(mode, first_step=mode["first_step"] + K1))
    _assert_window_is_not_vacuous(whole, a.STATE_LEN, a.get_state_tensors()[2], "split %s" % variant)
    _equal_bits(torch.cat([first, second], dim=0), whole, "K1 + K2 rows")
    _states_equal(a, b)
    a.close(); b.close(); pol.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    n, K = 300, 8
    env = _env("indi", n, 1)
    L, R = env._L, env.STATE_LEN + 8
    pol = _policy(env.state_len, SC["indi_action"])
    other_len = MfmaPolicy(env.state_len + 4)
    rows = torch.full((K * n * R + 8,), SENTINEL, dtype=torch.float32, device=env.device)
    log_std = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    before = env.get_state_tensors()

    def call(e=env, p=pol, k=K, ls=log_std, flags=1, m=n, r=rows):
        return L.qr_record_policy(e._h, p._h if p is not None else None, k, ls, 0, 0, flags, m, _ptr(r), e._stream())

    def refused(code, **kw):
        rc = call(**kw)
        assert rc == code, (list(kw.keys()), rc)
        assert len(L.qr_last_error()) > 0
        torch.cuda.synchronize()
        assert bool((rows == SENTINEL).all())
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    refused(_lib.QR_E_INVALID, p=None)
    refused(_lib.QR_E_INVALID, ls=None)
    refused(_lib.QR_E_INVALID, r=None)
    refused(_lib.QR_E_INVALID, r=rows[1:])          # not 16-byte aligned
    refused(_lib.QR_E_INVALID, r=rows[2:])
    refused(_lib.QR_E_INVALID, k=0)
    refused(_lib.QR_E_INVALID, k=-3)
    refused(_lib.QR_E_INVALID, m=0)
    refused(_lib.QR_E_INVALID, m=-1)
    refused(_lib.QR_E_INVALID, m=n + 1)
    refused(_lib.QR_E_INVALID, flags=4)
    refused(_lib.QR_E_INVALID, flags=3 | 8)
    refused(_lib.QR_E_INVALID, flags=-1)
    refused(_lib.QR_E_INVALID, p=other_len)
    no_weights = MfmaPolicy(env.state_len)
    refused(_lib.QR_E_STATE, p=no_weights)
    no_weights.close()
    env.pause = True
    refused(_lib.QR_E_STATE)
    env.pause = False
    env.pause_if_collision = True
    refused(_lib.QR_E_STATE)
    env.pause_if_collision = False
    if torch.cuda.device_count() > 1:
        elsewhere = MfmaPolicy(env.state_len, 1).load_torch(_torch_actor(env.state_len))   # a policy on another GPU
        refused(_lib.QR_E_INVALID, p=elsewhere)
        elsewhere.close()
    # the Python wrapper raises with the library's message
    with pytest.raises(_lib.QuadraceError, match="rec_envs"):
        env.record_policy_device(pol, K, torch.zeros(4), rec_envs=n + 1)
    # a registered terminal-observation buffer is left alone by a call that runs (envs do finish: time limit 5), every flag accepted
    env.max_steps = 5
    tb = torch.full((K, n, env.state_len), SENTINEL, device=env.device)
    env.set_terminal_obs_buffer(tb)
    for flags in (0, 1, 2, 3):
        assert call(flags=flags) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((tb == SENTINEL).all())
    got = rows[:K * n * R].view(K, n, R)
    assert not bool((got == SENTINEL).any()) and bool((rows[K * n * R:] == SENTINEL).all())
    assert int((got[:, :, env.STATE_LEN + 5] == 2).sum()) >= n
    assert env.last_rollout_ms() > 0.0           # qr_last_step_many_ms reports the launch
    env.close(); pol.close(); other_len.close()


def _torch_actor(obs_len):
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    return ActorCritic(obs_len, 4).pi


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the Python level
# ---------------------------------------------------------------------------------------------------------------------------------
def test_python_record_policy_agrees_with_evaluate_policy():
    from optimal_quad_control_rl_amd import (PPO, FlightRecord, Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, VecMonitor, evaluate_policy,
                                             record_policy, square_track)

    trk = square_track()
    train = VecMonitor(Quadcopter3DGates(256, *trk, gates_ahead=1, seed=1))
    train.venv.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    model = PPO("MlpPolicy", train, policy_kwargs=dict(activation_fn=torch.nn.ReLU, net_arch=[dict(pi=[120] * 3, vf=[120] * 3)], log_std_init=0),
                n_steps=8, batch_size=256, n_epochs=1, seed=3)
    with torch.no_grad():
        model._net.pi[-1].bias.copy_(torch.as_tensor(SC["e2e_action"]))   # untrained: the scenario's action plus a small observation-dependent term
    n, K = 4096, 600
    ev = VecMonitor(_env("e2e", n, 1, seed=99))                           # the scenario's track and the E2E time limit of this file
    fr = record_policy(model, ev, K, seed=99)
    assert isinstance(fr, FlightRecord) and fr.rows.shape == (K, n, 24) and fr.dt == np.float32(ev.venv.dt)
    res = evaluate_policy(model, ev, n_eval_steps=K, window_steps=250, seed=99)["total"]
    tot = fr.counts().sum(axis=0).tolist()
    print("end codes of env 0:", [(a, b, float(fr.end[b - 1, 0])) for a, b in fr.episodes(0)])
    print("record_policy counts", tot, "evaluate_policy", res["gates"], res["crashes"], res["timeouts"])
    assert min(tot) >= 1                                                       # passes, crashes and time-limit ends in the window
    assert tot == [res["gates"], res["crashes"], res["timeouts"]]
    # log_dict(0) = the reference's formulas on the raw rows
    d, rows = fr.log_dict(0), fr.rows
    w, c = rows[:, 0, :16], rows[:, 0, 16:20]
    want = {"t": rows[:, 0, 23] * np.float32(ev.venv.dt), "x": w[:, 0], "y": w[:, 1], "z": w[:, 2], "vx": w[:, 3], "vy": w[:, 4], "vz": w[:, 5],
            "V": np.sqrt(w[:, 3] ** 2 + w[:, 4] ** 2 + w[:, 5] ** 2), "phi": w[:, 6], "theta": w[:, 7], "psi": w[:, 8],
            "u1": (c[:, 0] + 1) / 2, "u2": (c[:, 1] + 1) / 2, "u3": (c[:, 2] + 1) / 2, "u4": (c[:, 3] + 1) / 2}
    want["u"] = np.stack([want["u1"], want["u2"], want["u3"], want["u4"]], axis=1)
    assert list(d) == list(want)
    for k in want:
        assert d[k].dtype == np.float32 and np.array_equal(d[k].view(np.uint32), want[k].view(np.uint32)), k
    # a cut record holds the same flights, and a sampled one differs from the deterministic one
    few = record_policy(model, ev, K, envs=8, seed=99)
    assert few.rows.shape == (K, 8, 24) and np.array_equal(few.rows.view(np.uint32), fr.rows[:, :8].view(np.uint32))
    assert np.array_equal(few.counts(), fr.counts()[:8])
    noisy = record_policy(model, ev, K, envs=8, seed=99, deterministic=False)
    assert not np.array_equal(noisy.rows, few.rows) and np.array_equal(noisy.rows[0, :, :16], few.rows[0, :, :16])
    # the native trainer is accepted as well
    assert np.array_equal(record_policy(model._trainer, ev, K, envs=8, seed=99).rows.view(np.uint32), few.rows.view(np.uint32))
    ev.venv.close(); train.venv.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. time
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65536, 4096])
def test_not_slower_than_the_rollout_kernel(n):
    """The recorder runs qr_rollout_policy's loop and writes 96 B per env-step in one stream where that kernel writes 122 B in six, so it
    must not be slower: median us/step of 5 launches <= 1.03 x the rollout kernel's (3 % = the run-to-run spread DESIGN section 5 states
    for these kernels, the evaluator's bound).  The protocol of tests/test_gpu_evaluate.py::test_not_slower_than_the_rollout_kernel:
    K = 2 000, E2E + residual MLPs + training disturbances, square track, gates_ahead 1, f16 operands, rec_envs = N; the two kernels
    alternate from the same seeded start with the same seeded network, one warm-up pair first, times from qr_last_step_many_ms."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    K = 2000
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=99)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = 10 ** 6
    torch.manual_seed(0)
    pol = MfmaPolicy(env.state_len).load_torch(ActorCritic(env.state_len, 4).pi)
    dev = env.device
    rows = torch.empty((K, n, 24), device=dev)
    out = (torch.empty((K, n, env.state_len), device=dev), torch.empty((K, n, 4), device=dev), torch.empty((K, n), device=dev),
           torch.empty((K, n), device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev))
    t_rec, t_roll = [], []
    for rep in range(6):
        env.seed(99); env.reset_device()
        env.record_policy_device(pol, K, torch.zeros(4), deterministic=True, out=rows)
        ms_c = env.last_rollout_ms()
        env.seed(99); env.reset_device()
        env.rollout_policy_device(pol, K, torch.zeros(4), deterministic=True, out=out)
        ms_r = env.last_rollout_ms()
        if rep:
            t_rec.append(ms_c * 1e3 / K); t_roll.append(ms_r * 1e3 / K)
    mc, mr = statistics.median(t_rec), statistics.median(t_roll)
    print("n %d: qr_record_policy %s -> median %.4f us/step; qr_rollout_policy %s -> median %.4f us/step; ratio %.4f"
          % (n, ["%.4f" % t for t in t_rec], mc, ["%.4f" % t for t in t_roll], mr, mc / mr))
    del out, rows
    env.close(); pol.close()
    assert mc <= 1.03 * mr, (mc, mr, mc / mr)
