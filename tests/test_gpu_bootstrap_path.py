"""GPU: the time-limit bootstrap of a training run, end to end: PPO(fused_collect=True) registers a [T][N][L] terminal-observation
buffer -> the closed-loop kernel fills rows [k][env] -> collect_fused evaluates the value network on the truncated rows and
scatters into buf_term_val -> qr_ppo_gae adds gamma * term_val.  Two consecutive collect() calls per case (the buffer is reused
without clearing), the three value paths, and with the native update the advantages and episode statistics against the float64
restatement of tests/gae_spec.py fed the same buffers."""
import copy

import numpy as np
import pytest
import torch

import gae_spec as G

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
N_ENVS, MAX_STEPS, N_STEPS = 2048, 20, 48

PATHS = {
    "f16-operands": dict(fused_collect=True, native_update=True, batch_size=N_ENVS * N_STEPS // 16),
    "f32class": dict(fused_collect=True, native_update=True, batch_size=N_ENVS * N_STEPS // 16, update_precision="f32",
                     policy_forward="f32class"),
    "torch": dict(fused_collect=True),
}


def _env(seed=11):
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, zigzag_track

    env = Quadcopter3DGates(N_ENVS, *zigzag_track(), gates_ahead=1, seed=seed, infos_mode="none")
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = MAX_STEPS
    return env


def _twin_rollout(twin, tb, buf_act):
    """Step the twin with the recorded, clamped actions: terminal rows [T, N, L] (sentinel where the env did not finish), done, trunc."""
    rows, done, trunc = [], [], []
    for t in range(buf_act.shape[0]):
        tb.fill_(SENTINEL)
        _, _, d, tr = twin.step_device(buf_act[t].clamp(-1.0, 1.0).contiguous())
        rows.append(tb.clone()); done.append(d.clone()); trunc.append(tr.clone())
    return torch.stack(rows), torch.stack(done), torch.stack(trunc)


def _value_tolerance(path, v64):
    scale = max(1.0, float(v64.abs().max()))
    # f16 operands: the 2e-2 rule of test_gae_and_value_forward_match_torch; f32-class handle: the bound of
    # test_f32class_policy_matches_float64_torch; torch float32: 1e-5
    return {"f16-operands": 2e-2 * scale, "f32class": 4e-6 * scale, "torch": 1e-5}[path]


@pytest.mark.parametrize("path", list(PATHS))
def test_fused_collect_bootstrap_chain(path):
    from optimal_quad_control_rl_amd.ppo import PPO

    T, N = N_STEPS, N_ENVS
    env, twin = _env(), _env()
    model = PPO(env, n_steps=T, gamma=0.999, seed=3, **PATHS[path])
    assert model.truncation_bootstrap and tuple(model._term_obs.shape) == (T, N, env.state_len)
    twin.reset_device()
    tb = torch.full((N, env.state_len), SENTINEL, device=twin.device)
    twin.set_terminal_obs_buffer(tb)
    if path == "f16-operands":
        value = lambda o: model._updater.forward(1, o.contiguous()).contiguous()
    elif path == "f32class":
        assert model._mfma_vf is not None
        value = lambda o: model._value_f32class_loader()(o)
    else:
        assert model._updater is None and model._mfma_vf is None
        value = model.policy.value
    state, aux = (np.zeros(N), np.zeros(N), np.zeros(N)), (None, None)
    for rollout in range(2):
        model.collect()
        torch.cuda.synchronize()
        done, trunc = model._done_u8.bool(), model._trunc_u8.bool()
        n_trunc, n_other = int(trunc.sum()), int((done & ~trunc).sum())
        assert n_trunc >= N and bool(done.any(dim=0).all()), (n_trunc, n_other)       # max_steps = 20 inside 48 steps
        # --- terminal rows: bit for bit the rows of an independent twin stepped by the per-step kernel (rollout 2: no stale rows)
        rows, d_tw, t_tw = _twin_rollout(twin, tb, model.buf_act)
        assert torch.equal(d_tw.bool(), done) and torch.equal(t_tw.bool(), trunc), rollout
        assert torch.equal(model._term_obs[done], rows[done]), (rollout, int((model._term_obs[done] != rows[done]).any(-1).sum()))
        # --- buf_term_val: 0 off the truncated rows; on them the same value path over ALL rows, then masked (gather / scatter)
        assert model.stats["truncations"] == n_trunc
        assert bool((model.buf_term_val[~trunc] == 0).all())
        with torch.no_grad():
            v_all = value(model._term_obs.view(T * N, -1)).view(T, N)
            v64 = copy.deepcopy(model.policy).double().value(model._term_obs.view(T * N, -1).double()).view(T, N)
        same = model.buf_term_val[trunc] == v_all[trunc]
        print(f"{path} rollout {rollout}: {n_trunc} truncations, {n_other} other finishes; gather vs all rows: "
              f"{int((~same).sum())} differ, max {float((model.buf_term_val[trunc] - v_all[trunc]).abs().max()):.3g}; "
              f"vs float64 {float((model.buf_term_val.double() - v64)[trunc].abs().max()):.3g} "
              f"(tolerance {_value_tolerance(path, v64[trunc]):.3g}, |V| max {float(v64[trunc].abs().max()):.3g})")
        # an independently written gather (row k * N + i from the [T, N] mask) through the same path, scattered back by mask
        kk, ii = torch.where(trunc)
        with torch.no_grad():
            v_rows = value(model._term_obs.view(T * N, -1)[kk * N + ii])
        want = torch.zeros_like(model.buf_term_val)
        want[kk, ii] = v_rows
        assert torch.equal(model.buf_term_val, want)
        if path == "torch":
            # torch picks its GEMM kernel by batch size, so 98 304 rows and the 4096 gathered ones round differently (measured:
            # 3723 of 4096 values differ, by at most 9.5e-7 at |V| up to 2.2): the all-rows recomputation holds at torch's 1e-5
            assert float((model.buf_term_val[trunc] - v_all[trunc]).abs().max()) <= 1e-5
        else:
            assert bool(same.all())
        assert bool((model.buf_term_val[trunc] != 0).any())
        assert float((model.buf_term_val.double() - v64)[trunc].abs().max()) <= _value_tolerance(path, v64[trunc])
        # --- the whole chain against the float64 restatement fed the same buffers
        if model._updater is not None:
            host = [t.cpu().numpy() for t in (model.buf_rew, model.buf_done, model.buf_val, model.last_val, model.buf_term_val)]
            adv, ret = model._gae_native()
            torch.cuda.synchronize()
            adv_ref, ret_ref, bound = G.gae(*host, model.gamma, model.lam)
            e_adv = np.abs(adv.cpu().numpy() - adv_ref) / bound
            e_ret = np.abs(ret.cpu().numpy() - ret_ref) / G.bound_ret(bound, host[2])
            print(f"{path} rollout {rollout}: advantages worst error / bound {e_adv.max():.3g}, returns {e_ret.max():.3g}")
            assert e_adv.max() <= 1.0 and e_ret.max() <= 1.0
            # a chain that lost the bootstrap would sit gamma * V(terminal obs) away at every truncated row: far outside the bound
            miss = (np.float32(model.gamma) * np.abs(host[4]) / bound)[host[4] != 0]
            assert np.median(miss) > 100, float(np.median(miss))
            state, fin, (b_er, b_fin, _, _), aux = G.episode_stats(host[0], host[1], *state, *aux)
            assert np.array_equal(model.ep_len.cpu().numpy(), state[1]) and np.array_equal(model.ep_gates.cpu().numpy(), state[2])
            assert (np.abs(model.ep_ret.cpu().numpy() - state[0]) <= b_er).all()
            st = model.stats
            assert st["episodes"] == fin[3] and st["ep_len_mean"] == fin[1] / fin[3] and st["gates_per_episode"] == fin[2] / fin[3]
            assert abs(st["ep_rew_mean"] - fin[0] / fin[3]) <= (b_fin + G.U32 * abs(fin[0])) / fin[3]
    env.close(); twin.close()


def test_per_step_collect_bootstrap_rows_and_values():
    """The per-step collect() with its [N][L] buffer and torch.where(trunc, V, 0): buf_term_val[t] is V of the rows the twin's
    kernel writes at step t on the truncated envs and 0 elsewhere, and after the rollout the buffer holds, for every env, the row
    of the last step at which it finished."""
    from optimal_quad_control_rl_amd.ppo import PPO

    T, N = N_STEPS, N_ENVS
    env, twin = _env(), _env()
    model = PPO(env, n_steps=T, gamma=0.999, seed=3)
    assert tuple(model._term_obs.shape) == (N, env.state_len)
    twin.reset_device()
    tb = torch.full((N, env.state_len), SENTINEL, device=twin.device)
    twin.set_terminal_obs_buffer(tb)
    for rollout in range(2):
        model.collect()
        torch.cuda.synchronize()
        rows, d_tw, t_tw = _twin_rollout(twin, tb, model.buf_act)
        done, trunc = d_tw.bool(), t_tw.bool()
        assert torch.equal(model.buf_done, done.float())
        assert int(trunc.sum()) >= N and bool(done.any(dim=0).all())
        last_k = (done.long() * torch.arange(1, T + 1, device=done.device).view(T, 1)).amax(dim=0) - 1    # last finishing step of each env
        assert torch.equal(model._term_obs, rows[last_k, torch.arange(N, device=done.device)])
        assert bool((model.buf_term_val[~trunc] == 0).all())
        with torch.no_grad():
            v = torch.stack([model.policy.value(rows[t]) for t in range(T)])           # same path, same batch shape as collect()
            v64 = copy.deepcopy(model.policy).double().value(rows.view(T * N, -1).double()).view(T, N)
        assert torch.equal(model.buf_term_val[trunc], v[trunc])
        assert bool((model.buf_term_val[trunc] != 0).any())
        assert float((model.buf_term_val.double() - v64)[trunc].abs().max()) <= 1e-5
    env.close(); twin.close()
