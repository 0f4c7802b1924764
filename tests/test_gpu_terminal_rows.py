"""GPU: the terminal-observation rows of the closed-loop kernel (qr_rollout_policy, rollout_policy_kernel<V, GA, kF32>:
store_terminal_obs inside step_env, ahead of the auto-reset) -- the rows PPO's time-limit bootstrap evaluates the value network
on.  (a) bit identity with the per-step kernel's rows at all 20 instantiations, (b) registering the buffer changes nothing else,
(c) the rows against the CPU oracle's, (d) enough finishes of both kinds in every case that nothing passes by absence,
(e) the host-side refusals.

Finishes inside the window.  Every env starts `i % 20` steps into its episode (time limits fall on different k, some envs meet
two) and every fourth env starts 1-30 cm above the ground sinking at 0.5-3 m/s (ground contacts spread over the first steps).
The CPU oracle driven by the same torch policy in float32 meets condition (d) on its own with these settings (K = 48,
max_steps = 30, gain 20); counts of (time-limit finishes, other finishes, envs that never finish):

  n = 1000, zigzag (E2E) / square (INDI), gates_ahead 0..4
    E2E   (1314, 200, 0) (1311, 203, 0) (1311, 203, 0) (1313, 200, 0) (1310, 204, 0)
    INDI  (1313, 201, 0) (1314, 200, 0) (1311, 203, 0) (1314, 198, 0) (1317, 192, 0)
  n = 65 536, gates_ahead 1:   E2E (86034, 13201, 0)   INDI (86014, 13260, 0)
  (c) n = 2048, square, gates_ahead 2:   E2E (2684, 415, 0)   INDI (2685, 414, 0)
against the required n / 20 = 50, 3277 and 103."""
import numpy as np
import pytest
import torch

import parity as P

pytestmark = pytest.mark.gpu

E2E, INDI = 0, 1
SENTINEL = -77777.0
K_STEPS, MAX_STEPS, GAIN = 48, 30, 20.0


@pytest.fixture(scope="module")
def PA():
    assert torch.cuda.is_available()
    from product_adapter import ProductAdapter

    return ProductAdapter


@pytest.fixture(scope="module")
def OA():
    from oracle_adapter import OracleAdapter

    return OracleAdapter


def arrange_starts(world, steps):
    """In place, on host arrays of a freshly reset batch: stagger the episode clocks and put every fourth env just above the
    ground, sinking (z is down: contact is z > 0)."""
    n = world.shape[0]
    i = np.arange(n)
    low = i % 4 == 0
    world[low, 2] = (-0.01 - 0.29 * ((i * 0.6180339887) % 1.0)).astype(np.float32)[low]
    world[low, 5] = (0.5 + 2.5 * ((i * 0.3819660113) % 1.0)).astype(np.float32)[low]
    steps[:] = i % 20
    return world, steps


def policy_net(obs_len, gain=GAIN):
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(3)
    net = ActorCritic(obs_len, 4)
    with torch.no_grad():
        net.pi[-1].weight.mul_(gain)   # a policy that actually moves the drone
    return net


def _policy(obs_len):
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    net = policy_net(obs_len).cuda()
    return MfmaPolicy(obs_len).load_torch(net.pi)


def _make(variant, n, gates_ahead, seed=5, arrange=True):
    from optimal_quad_control_rl_amd import (Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES,
                                             square_track, zigzag_track)

    if variant == "e2e":
        env = Quadcopter3DGates(n, *zigzag_track(), gates_ahead=gates_ahead, seed=seed, infos_mode="none")
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    else:
        env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=gates_ahead, seed=seed, infos_mode="none")
    env.max_steps = MAX_STEPS
    env.reset_device()
    if arrange:
        w, _, _, s, _ = env.get_state_tensors()
        w, s = arrange_starts(w.cpu().numpy(), s.cpu().numpy())
        env.set_state_tensors(world=w, steps=s)
        env.update_states()
    return env


def _assert_finishes(done, trunc, n):
    """Condition (d), asserted before anything else: done / trunc [K, n] of the window."""
    done, trunc = done.bool(), trunc.bool()
    by_limit, other = int((done & trunc).sum()), int((done & ~trunc).sum())
    never = int((~done.any(dim=0)).sum())
    assert by_limit >= n / 20 and other >= n / 20 and never == 0, (by_limit, other, never)


def _final_state_equal(a, b):
    for sa, sb in zip(a.get_state_tensors(), b.get_state_tensors()):
        assert sa is None or torch.equal(sa, sb)


def _terminal_rows_equal_launches(variant, n, precision, gates_ahead, stochastic=False):
    K = K_STEPS
    a, b = _make(variant, n, gates_ahead), _make(variant, n, gates_ahead)
    L = a.state_len
    assert L == (20 if variant == "e2e" else 13) + 4 * gates_ahead
    pol = _policy(L)
    ta = torch.full((K, n, L), SENTINEL, device=a.device)
    tb = torch.full((n, L), SENTINEL, device=b.device)
    a.set_terminal_obs_buffer(ta)
    b.set_terminal_obs_buffer(tb)
    log_std = torch.tensor([-0.5, -0.3, -0.7, -0.4]) if stochastic else torch.zeros(4)
    obs, act, logp, rew, done, trunc, last = a.rollout_policy_device(pol, K, log_std, noise_seed=11, first_step=7,
                                                                     deterministic=not stochastic, precision=precision)
    _assert_finishes(done, trunc, n)
    o = b.states_tensor.clone()
    for k in range(K):
        assert torch.equal(obs[k], o), k
        if not stochastic:
            assert torch.equal(act[k], pol.forward(o, precision=precision)), k
        tb.fill_(SENTINEL)
        o2, r2, d2, t2 = b.step_device(act[k].clamp(-1, 1).contiguous())    # stochastic: B is driven by A's recorded actions
        assert torch.equal(rew[k], r2) and torch.equal(done[k], d2) and torch.equal(trunc[k], t2), k
        d = d2.bool()
        assert torch.equal(ta[k][d], tb[d]), (k, int((ta[k][d] != tb[d]).any(dim=-1).sum()))
        assert bool((tb[d] != SENTINEL).any(dim=-1).all()), k               # B's own rows were written
        assert bool((ta[k][~d] == SENTINEL).all()), k                       # rows of the others: untouched, every element
        assert bool((tb[~d] == SENTINEL).all()), k
        o = o2.clone()
    assert torch.equal(last, o)
    _final_state_equal(a, b)
    a.close(); b.close()


_GATES_AHEAD = [(v, g) for v in ("e2e", "indi") for g in range(5)]


@pytest.mark.parametrize("variant,gates_ahead", _GATES_AHEAD, ids=["%s-L%d" % (v, (20 if v == "e2e" else 13) + 4 * g) for v, g in _GATES_AHEAD])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_terminal_rows_equal_the_step_kernels_at_every_instantiation(variant, gates_ahead, precision):
    """(a) all 20 instantiations of the closed-loop kernel at the ragged n = 1000: row [k][env] of every env that finishes at
    step k is, bit for bit, the row the per-step kernel writes for the same state and action; every other row keeps the sentinel."""
    _terminal_rows_equal_launches(variant, 1000, precision, gates_ahead)


@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_terminal_rows_equal_the_step_kernels_at_full_size(variant, precision):
    _terminal_rows_equal_launches(variant, 65536, precision, 1)


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_terminal_rows_equal_the_step_kernels_with_sampled_actions(variant):
    _terminal_rows_equal_launches(variant, 1000, "f16-operands", 1, stochastic=True)


@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_registering_the_buffer_changes_nothing_else(variant, precision):
    """(b) same env, seed and policy with and without the buffer: every output and the final state bit-identical."""
    n, K = 1000, K_STEPS
    runs = []
    for with_buffer in (False, True):
        env = _make(variant, n, 1)
        pol = _policy(env.state_len)
        if with_buffer:
            env.set_terminal_obs_buffer(torch.full((K, n, env.state_len), SENTINEL, device=env.device))
        out = env.rollout_policy_device(pol, K, torch.tensor([-0.5, -0.3, -0.7, -0.4]), noise_seed=5, precision=precision)
        runs.append(([t.clone() for t in out], env.get_state_tensors()))
        env.close()
    _assert_finishes(runs[0][0][4], runs[0][0][5], n)
    for x, y in zip(runs[0][0], runs[1][0]):
        assert torch.equal(x, y)
    for x, y in zip(runs[0][1], runs[1][1]):
        assert x is None or torch.equal(x, y)


@pytest.mark.parametrize("variant", [E2E, INDI])
def test_terminal_rows_vs_oracle(PA, OA, variant, residual_blob):
    """(c) teacher-forced against the CPU oracle: the oracle's state goes into the env before every step, one 1-step closed-loop
    call with a 1-row buffer, the kernel's clamped action drives the oracle twin; the terminal rows of the envs both finish agree
    within the project's one-step observation tolerance."""
    n, K = 2048, K_STEPS
    trk = P.tracks()["square"]
    kw = dict(gates_ahead=2, residual=residual_blob if variant == E2E else None,
              dist_ranges=P.TRAIN_DIST_RANGES if variant == E2E else None, seed=5)
    g, o = PA(variant, n, trk, **kw), OA(variant, n, trk, **kw)
    L = g.env.state_len
    pol = _policy(L)
    g.env.max_steps = MAX_STEPS
    o.env.set_limits(MAX_STEPS, 0.01)
    g.reset(); o.reset()
    wo, do, to, so = o.get_state()
    arrange_starts(wo, so)
    o.set_state(wo, do, to, so)
    tbuf = torch.full((1, n, L), SENTINEL, device=g.env.device)
    g.env.set_terminal_obs_buffer(tbuf)
    obuf = np.full((n, L), SENTINEL, np.float32)
    o.env.set_terminal_obs(obuf)
    done_all, trunc_all = np.zeros((K, n), bool), np.zeros((K, n), bool)
    worst, untouched, mismatches = 0.0, True, 0
    for k in range(K):
        wo, do, to, so = o.get_state()
        g.set_state(wo, do if variant == E2E else None, to, so)
        g.env.set_state_tensors(episode=o.env.episode.astype(np.int64))
        tbuf.fill_(SENTINEL); obuf[:] = SENTINEL
        _, act, _, _, dng, trg, _ = g.env.rollout_policy_device(pol, 1, torch.zeros(4), deterministic=True)
        a = act[0].clamp(-1, 1).cpu().numpy()
        dng, trg = dng[0].cpu().numpy().astype(bool), trg[0].cpu().numpy().astype(bool)
        _, _, dno, tro = o.step(a)
        t = tbuf[0].cpu().numpy()
        both = dng & dno
        mismatches += int((dng != dno).sum())
        untouched = untouched and bool((t[~dng] == SENTINEL).all()) and bool((obuf[~dno] == SENTINEL).all())
        untouched = untouched and bool((t[dng] != SENTINEL).any(axis=-1).all())
        done_all[k], trunc_all[k] = both, both & trg & tro
        if both.any():
            worst = max(worst, float(P.obs_err(t[both], obuf[both]).max()))
    _assert_finishes(torch.as_tensor(done_all), torch.as_tensor(trunc_all), n)
    print(f"terminal rows vs oracle, variant {variant}: worst obs_err {worst:.3g} (tolerance {P.TOL_STEP_OBS:g}), "
          f"{mismatches} done mismatches")
    assert untouched
    assert mismatches <= 4                      # knife-edge threshold cases only, as in the full-size lock-step test
    assert worst < P.TOL_STEP_OBS, worst
    g.env.close()


def test_closed_loop_refusals_are_made_before_any_launch():
    """(e) K above the registered row count -> QR_E_INVALID; pause / pause_if_collision -> QR_E_STATE; neither touches an output
    buffer or the env's state."""
    from optimal_quad_control_rl_amd import _lib

    n, K = 256, 4
    env = _make("indi", n, 1, arrange=False)
    L = env.state_len
    pol = _policy(L)
    dev = env.device
    out = (torch.full((K, n, L), SENTINEL, device=dev), torch.full((K, n, 4), SENTINEL, device=dev),
           torch.full((K, n), SENTINEL, device=dev), torch.full((K, n), SENTINEL, device=dev),
           torch.full((K, n), 77, dtype=torch.uint8, device=dev), torch.full((K, n), 77, dtype=torch.uint8, device=dev))
    before = env.get_state_tensors()

    def refused(code):
        with pytest.raises(_lib.QuadraceError) as ei:
            env.rollout_policy_device(pol, K, torch.zeros(4), deterministic=True, out=out)
        assert ei.value.code == code, ei.value
        torch.cuda.synchronize()
        assert all(bool((t == (77 if t.dtype == torch.uint8 else SENTINEL)).all()) for t in out)
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    for rows in (1, K - 1):
        tb = torch.full((rows, n, L), SENTINEL, device=dev)
        env.set_terminal_obs_buffer(tb if rows > 1 else tb[0])
        refused(_lib.QR_E_INVALID)
        assert bool((tb == SENTINEL).all())
    tb = torch.full((K, n, L), SENTINEL, device=dev)
    env.set_terminal_obs_buffer(tb)
    env.pause = True
    refused(_lib.QR_E_STATE)
    env.pause = False
    env.pause_if_collision = True
    refused(_lib.QR_E_STATE)
    env.pause_if_collision = False
    assert bool((tb == SENTINEL).all())
    env.rollout_policy_device(pol, K, torch.zeros(4), deterministic=True, out=out)       # K == rows, no pause: runs
    torch.cuda.synchronize()
    assert not bool((out[0] == SENTINEL).any())
    env.close()
