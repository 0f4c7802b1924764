"""GPU: the trainers on the predecessor envs (Quadcopter3DVec / Quadcopter3DVecGates of "3D quad.ipynb"): `ppo.PPO` with the closed-loop
collect kernel (q3_rollout_policy) and the matrix-core update at observation length 16, `sb3.PPO` on top of it with save / load, and the
refusal of the per-step collect path these envs do not have."""
import numpy as np
import pytest
import torch

import parity_quad3d as pq

pytestmark = pytest.mark.gpu

N, T, B = 256, 32, 2048


def _env(kind, seed=3):
    from optimal_quad_control_rl_amd.quad3d import Quadcopter3DVec, Quadcopter3DVecGates

    env = Quadcopter3DVec(N, seed=seed) if kind == "hover" else Quadcopter3DVecGates(N, *pq.gates_track(), seed=seed)
    env.max_steps = 20      # episodes (and time-limit bootstraps) end inside every rollout
    return env


@pytest.mark.parametrize("kind,kw", [("hover", {}), ("gates", {}),
                                     ("hover", dict(update_precision="f32", policy_forward="f32class")),
                                     ("gates", dict(update_precision="f32", policy_forward="f32class")),
                                     ("hover", dict(native_update=False))],
                         ids=["hover", "gates", "hover-f32", "gates-f32", "hover-torch-update"])
def test_ppo_trains_a_q3_env(kind, kw):
    from optimal_quad_control_rl_amd.ppo import PPO

    kw = dict(dict(native_update=True), **kw)
    model = PPO(_env(kind), n_steps=T, batch_size=B, n_epochs=2, fused_collect=True, seed=1, **kw)
    theta0 = [p.detach().clone() for p in model.policy.parameters()]
    for _ in range(3):
        model.collect()
        assert bool(torch.isfinite(model.buf_obs).all()) and bool(torch.isfinite(model.buf_act).all())
        assert bool(torch.isfinite(model.buf_lp).all()) and bool(torch.isfinite(model.buf_rew).all())
        assert bool(torch.isfinite(model.buf_val).all()) and bool(torch.isfinite(model.last_val).all())
        model.train()
    assert model.num_timesteps == 3 * N * T
    assert model.noise_step == 3 * T
    for p0, p in zip(theta0, model.policy.parameters()):
        assert bool(torch.isfinite(p).all())
    assert any(not torch.equal(p0, p.detach()) for p0, p in zip(theta0, model.policy.parameters()))
    for key in ("ep_rew_mean", "ep_len_mean", "episodes", "reward_per_step", "truncations", "updates"):
        assert key in model.stats, (key, model.stats)
    assert model.stats["episodes"] >= N and model.stats["truncations"] > 0 and model.stats["non_finite_rows"] == 0
    assert 1.0 <= model.stats["ep_len_mean"] <= 20.0
    # the time-limit bootstrap read terminal rows the kernel wrote: V(terminal observation) is there for truncated steps and only there
    trunc = model._trunc_u8.bool()
    assert bool((model.buf_term_val[~trunc] == 0).all()) and bool((model.buf_term_val[trunc] != 0).any())


@pytest.mark.parametrize("kind", ["hover", "gates"])
def test_per_step_collect_is_refused(kind):
    from optimal_quad_control_rl_amd.ppo import PPO

    with pytest.raises(ValueError, match="fused_collect"):
        PPO(_env(kind), n_steps=T, batch_size=B, fused_collect=False)


@pytest.mark.parametrize("kind", ["hover", "gates"])
def test_sb3_learn_save_load_continues_bit_for_bit(kind, tmp_path):
    from optimal_quad_control_rl_amd import PPO, VecMonitor

    pk = dict(activation_fn=torch.nn.ReLU, net_arch=[dict(pi=[120, 120, 120], vf=[120, 120, 120])], log_std_init=0)

    def make():
        env = VecMonitor(_env(kind))
        return PPO("MlpPolicy", env, policy_kwargs=pk, n_steps=T, batch_size=B, n_epochs=2, gamma=0.999, seed=5), env

    model, env = make()
    tr = model._trainer
    assert tr.fused_collect and tr.native_update and tr._q3             # "auto" picks the fused path and the matrix-core update
    steps = N * T
    model.learn(total_timesteps=2 * steps)
    assert model.num_timesteps == 2 * steps and "ep_rew_mean" in model.ep_info
    path = model.save(str(tmp_path / kind / str(model.num_timesteps)))
    # predict() on the env's own observation: float64 for the hover env, cast to float32; actions clipped to the Box
    states = env.states
    assert states.dtype == (np.float64 if kind == "hover" else np.float32)
    actions, _ = model.predict(states, deterministic=True)
    assert actions.dtype == np.float32 and actions.shape == (N, 4) and np.abs(actions).max() <= 1.0
    with torch.no_grad():
        want = tr.policy.pi(torch.as_tensor(states.astype(np.float32), device=tr.dev)).clamp(-1, 1).cpu().numpy()
    np.testing.assert_array_equal(actions, want)
    sampled, _ = model.predict(states * 50.0)
    assert sampled.dtype == np.float32 and np.abs(sampled).max() <= 1.0
    # a fresh env built with the same arguments: the loaded model continues bit for bit
    _, env2 = make()
    loaded = PPO.load(path, env=env2)
    assert loaded.num_timesteps == model.num_timesteps
    for a, b in zip(tr.env.get_state_tensors(), loaded._trainer.env.get_state_tensors()):
        assert torch.equal(a, b)
    model.learn(total_timesteps=steps, reset_num_timesteps=False)
    loaded.learn(total_timesteps=steps, reset_num_timesteps=False)
    assert loaded.num_timesteps == model.num_timesteps == 3 * steps
    for name in ("buf_obs", "buf_act", "buf_lp", "buf_rew", "buf_done", "buf_val", "buf_term_val"):
        assert torch.equal(getattr(tr, name), getattr(loaded._trainer, name)), name
    sd_a, sd_b = model.policy.state_dict(), loaded.policy.state_dict()
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert torch.equal(tr._updater.m, loaded._trainer._updater.m) and torch.equal(tr._updater.v, loaded._trainer._updater.v)
    assert tr._updater.step == loaded._trainer._updater.step
    for a, b in zip(tr.env.get_state_tensors(), loaded._trainer.env.get_state_tensors()):
        assert torch.equal(a, b)
    # policy-only load (no env): the saved network, two rollouts old
    bare = PPO.load(path)
    assert bare.observation_dim == 16
    np.testing.assert_array_equal(bare.predict(states, deterministic=True)[0], actions)
