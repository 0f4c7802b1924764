"""GPU: round-3 tests -- full-size lock-step for the remaining (track, gates_ahead) cases with every tolerated `done` mismatch
PROVEN knife-edge, the terminal-observation buffer's row capacity, the SB3-shaped model object (train -> save -> load ->
identical continuation), the rollout-boundary gather on RCCL at BASELINE config-4 size with its memory bound, and the
f16-operand gradient against f32 autograd on rows of a real rollout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity as P
from parity import knife_edge_margin   # moved to tests/parity.py; test_gpu_round5 imports it from here

pytestmark = pytest.mark.gpu

E2E, INDI = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def PA():
    assert torch.cuda.is_available()
    from product_adapter import ProductAdapter

    return ProductAdapter


@pytest.fixture(scope="module")
def OA():
    from oracle_adapter import OracleAdapter

    return OracleAdapter


@pytest.mark.parametrize("variant,tname,ga", [(E2E, "zigzag", 0), (E2E, "zigzag", 2), (E2E, "square", 0), (E2E, "square", 2),
                                              (INDI, "square", 0), (INDI, "square", 2), (INDI, "zigzag", 0), (INDI, "zigzag", 2),
                                              (E2E, "square", 1), (INDI, "zigzag", 1)])
def test_full_size_lockstep_all_tracks_and_gates_ahead(PA, OA, variant, tname, ga, residual_blob):
    """N = 65 536 product vs oracle, teacher-forced through auto-resets, for the (variant, track, gates_ahead) combinations the
    round-2 test did not run.  dones / targets / step counts exact, freshly reset lanes bit-exact, live lanes within the one-step
    tolerance -- and every env whose `done` differs is shown to sit < 1e-5 from a termination threshold (no blanket allowance)."""
    n, K = 65536, 24
    trk = P.tracks()[tname]
    kw = dict(gates_ahead=ga, residual=residual_blob if variant == E2E else None,
              dist_ranges=P.TRAIN_DIST_RANGES if variant == E2E else None, seed=41 + ga)
    g, o = PA(variant, n, trk, **kw), OA(variant, n, trk, **kw)
    o.env.set_threads(16)
    g.env.max_steps = 15
    o.env.set_limits(15, 0.01)
    g.reset(); o.reset()
    gate_pos, gate_yaw = np.asarray(trk[0], np.float32), np.asarray(trk[1], np.float32)
    rng = np.random.default_rng(100 + 7 * ga + variant)
    tot_done, mismatches, worst_state, worst_obs = 0, 0, 0.0, 0.0
    for k in range(K):
        wo, do, to, so = o.get_state()
        g.set_state(wo, do if variant == E2E else None, to, so)
        g.env.set_state_tensors(episode=o.env.episode.astype(np.int64))
        a = rng.uniform(-1, 1, size=(n, 4)).astype(np.float32)
        if k % 2:
            a = (0.124 + 0.3 * a).astype(np.float32) if variant == E2E else (0.2 * a + [0, 0, 0, 0.22]).astype(np.float32)
        og, rg, dng, trg = g.step(a)
        oo, ro, dno, tro = o.step(a)
        mism = dng != dno
        for i in np.nonzero(mism)[0]:
            row = (*gate_pos[to[i] % len(gate_yaw)], gate_yaw[to[i] % len(gate_yaw)])
            margin = knife_edge_margin(variant, wo[i], a[i], do[i] if variant == E2E else None, kw["residual"], row)
            assert margin < 1e-5, f"step {k} env {i}: done differs {dng[i]} vs {dno[i]} with margin {margin:.3e}"
        mismatches += int(mism.sum())
        ok = ~mism
        wg, dg, tg, sg = g.get_state()
        wo2, do2, to2, so2 = o.get_state()
        np.testing.assert_array_equal(tg[ok], to2[ok])
        np.testing.assert_array_equal(sg[ok], so2[ok])
        np.testing.assert_array_equal(trg, tro)
        assert np.abs(rg[ok] - ro[ok]).max() < P.TOL_STEP_REWARD
        done, live = dno & ok, ~dno & ok
        np.testing.assert_array_equal(wg[done], wo2[done])                  # freshly reset lanes: bit exact
        if variant == E2E:
            np.testing.assert_array_equal(dg[done], do2[done])
        if live.any():
            worst_state = max(worst_state, float(P.rel_err(wg[live], wo2[live]).max()))
        worst_obs = max(worst_obs, float(P.obs_err(og[ok], oo[ok], wo2[ok]).max()))
        tot_done += int(dno.sum())
    assert worst_state < P.TOL_STEP_STATE and worst_obs < P.TOL_STEP_OBS, (worst_state, worst_obs)
    assert tot_done >= n and mismatches <= 8, (tot_done, mismatches)


def test_terminal_obs_buffer_capacity_is_enforced(PA, residual_blob):
    """a [N, L] terminal-observation buffer registered for qr_step must not be written at row [k][env] by a K-step
    call.  The buffer's leading dimension travels with the pointer (ABI v3) and K > rows is refused."""
    from optimal_quad_control_rl_amd._lib import QuadraceError

    n = 512
    g = PA(E2E, n, P.tracks()["zigzag"], gates_ahead=1, residual=residual_blob, dist_ranges=P.TRAIN_DIST_RANGES)
    env = g.env
    env.reset_device()
    L = env.state_len
    env.set_terminal_obs_buffer(torch.zeros((n, L), dtype=torch.float32, device=env.device))
    acts = torch.rand((4, n, 4), device=env.device) * 2 - 1
    env.step_device(acts[0].contiguous())                                   # K = 1 path is fine
    out4 = (torch.empty((4, n, L), device=env.device), torch.empty((4, n), device=env.device),
            torch.empty((4, n), dtype=torch.uint8, device=env.device), torch.empty((4, n), dtype=torch.uint8, device=env.device))
    for call in (lambda: env.rollout_device(acts), lambda: env.step_sequence_device(acts, out4)):
        with pytest.raises(QuadraceError, match="terminal-observation"):
            call()
    env.rollout_device(acts[:1])                                            # K = 1 <= rows
    env.set_terminal_obs_buffer(torch.zeros((4, n, L), dtype=torch.float32, device=env.device))
    env.rollout_device(acts)                                                # K = 4 <= rows
    with pytest.raises(QuadraceError, match="terminal-observation"):
        env.rollout_device(torch.cat([acts, acts]))                         # K = 8 > rows
    env.set_terminal_obs_buffer(None)
    env.rollout_device(torch.cat([acts, acts]))
    env.close()


def test_integer_attributes_are_int64_like_the_reference(PA):
    """R:322, R:348: `target_gates` / `step_counts` are `np.zeros(num_envs, dtype=int)` = int64; the device keeps int32, the
    attribute views hand out (and take back) int64."""
    g = PA(INDI, 64, P.tracks()["square"], gates_ahead=1)
    env = g.env
    env.reset()
    env.step(np.zeros((64, 4), np.float32))
    assert env.target_gates.dtype == np.int64 and env.step_counts.dtype == np.int64
    assert (env.step_counts == 1).all()
    env.step_counts[:] = 7
    env.target_gates[3] = 2
    assert (env.step_counts == 7).all() and env.target_gates[3] == 2 and env.target_gates[4] == 0
    env.close()


def test_states_tensor_tracks_the_rollout_buffer_without_a_copy(PA, residual_blob):
    """A K-step call leaves its last observation in row K-1 of the caller's buffer and launches NO copy; the first read of
    `states` / `states_tensor` takes a stable copy into the env's own buffer (readers must not see later reuse of the
    rollout buffer)."""
    g = PA(E2E, 1024, P.tracks()["zigzag"], gates_ahead=1, residual=residual_blob, dist_ranges=P.TRAIN_DIST_RANGES)
    env = g.env
    first = env.reset_device().clone()
    assert torch.equal(env.states_tensor, first)
    acts = torch.rand((5, 1024, 4), device=env.device) * 2 - 1
    obs, rew, done, trunc = env.rollout_device(acts)
    assert env._last_obs.data_ptr() == obs[4].data_ptr()                   # still a view of row K-1: no copy kernel behind the rollout
    last = obs[4].clone()
    st = env.states_tensor                                                 # first read: the stable copy
    assert st.data_ptr() != obs[4].data_ptr() and torch.equal(st, last)
    obs.zero_()                                                            # the caller reuses its rollout buffer ...
    assert torch.equal(env.states_tensor, last)                            # ... and the env's current observation is unaffected
    np.testing.assert_array_equal(env.states, last.cpu().numpy())
    o2, *_ = env.step_device(acts[0].contiguous())
    assert env.states_tensor.data_ptr() == o2.data_ptr()
    env.update_states()
    assert torch.equal(env.states_tensor, o2)
    env.close()


def _make_model(seed=5, n=4096, n_steps=16, **kw):
    from optimal_quad_control_rl_amd import PPO, Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, VecMonitor, square_track

    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=3)
    env = VecMonitor(env)
    env.venv.disturbance_ranges = TRAIN_DISTURBANCE_RANGES                                   # R:780
    policy_kwargs = dict(activation_fn=torch.nn.ReLU, net_arch=[dict(pi=[120, 120, 120], vf=[120, 120, 120])], log_std_init=0)
    model = PPO("MlpPolicy", env, policy_kwargs=policy_kwargs, verbose=0, n_steps=n_steps, batch_size=4096, n_epochs=2,
                gamma=0.999, seed=seed, **kw)
    return model, env


def test_sb3_model_trains_saves_loads_and_continues_bit_for_bit(tmp_path):
    """the reference's training loop (R:813-831) on the SB3-shaped object -- learn(reset_num_timesteps=False),
    save every few rollouts, PPO.load -- and a loaded model is the same model: identical predict() bits, and one more learn() on
    the original and on the reloaded copy gives identical parameters (optimiser state, step counters, env state, episode
    accumulators and generator states all travel in the checkpoint)."""
    from optimal_quad_control_rl_amd import PPO

    model, env = _make_model()
    assert model._trainer.native_update and model._trainer.fused_collect          # the kernels, not the torch path
    TIMESTEPS = model.n_steps * env.num_envs * 2
    model.learn(total_timesteps=TIMESTEPS, reset_num_timesteps=False, tb_log_name="t")      # R:820
    assert model.num_timesteps == TIMESTEPS
    model.learn(total_timesteps=TIMESTEPS, reset_num_timesteps=False, tb_log_name="t")
    assert model.num_timesteps == 2 * TIMESTEPS
    path = model.save(str(tmp_path / "E2E" / "t" / str(model.num_timesteps)))               # R:823
    states = env.states
    actions, _ = model.predict(states, deterministic=True)                                  # R:803
    assert isinstance(actions, np.ndarray) and actions.shape == (env.num_envs, 4) and np.abs(actions).max() <= 1.0

    # policy-only load (what the export cell does, R:3985-3996)
    bare = PPO.load(path)
    a_bare, _ = bare.predict(states, deterministic=True)
    np.testing.assert_array_equal(a_bare, actions)
    net = torch.nn.Sequential(*(list(bare.policy.mlp_extractor.policy_net) + [bare.policy.action_net]))
    with torch.no_grad():
        mean = net(torch.as_tensor(states, device=bare.device)).clamp(-1, 1).cpu().numpy()
    np.testing.assert_array_equal(mean, actions)

    # full load onto a fresh env built with the same arguments: the run continues bit for bit
    model2, env2 = _make_model()
    loaded = PPO.load(path, env=env2)
    assert loaded.num_timesteps == model.num_timesteps
    np.testing.assert_array_equal(loaded.predict(states, deterministic=True)[0], actions)
    for a, b in zip(model._trainer.env.get_state_tensors(), loaded._trainer.env.get_state_tensors()):
        assert a is None or torch.equal(a, b)
    model.learn(total_timesteps=TIMESTEPS, reset_num_timesteps=False)
    loaded.learn(total_timesteps=TIMESTEPS, reset_num_timesteps=False)
    assert loaded.num_timesteps == model.num_timesteps == 3 * TIMESTEPS
    sd_a, sd_b = model.policy.state_dict(), loaded.policy.state_dict()
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert torch.equal(model._trainer._updater.m, loaded._trainer._updater.m)
    assert torch.equal(model._trainer._updater.v, loaded._trainer._updater.v)
    assert model._trainer._updater.step == loaded._trainer._updater.step
    assert any(not torch.equal(sd_a[k], model2.policy.state_dict()[k].to(sd_a[k].device)) for k in sd_a)   # and it did train


def test_sb3_model_with_the_reference_hyper_parameters_runs_on_the_matrix_cores():
    """The training cell's own settings (R:783-795: n_steps = 1000, batch_size = 5000, n_epochs = 10, 100 envs): 5000 is not a multiple
    of 64 -- the gradient kernel masks the 8-row tail of the last group -- so the facade keeps the matrix-core update; every one of the
    20 x 10 updates per rollout is applied (the gradient of a 5000-row minibatch is checked against autograd in
    test_gpu_ppo_kernel.py).  Only a batch size that does not divide the rollout falls back to torch autograd."""
    from optimal_quad_control_rl_amd import PPO, Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track

    kw = dict(policy_kwargs=dict(activation_fn=torch.nn.ReLU, net_arch=[dict(pi=[120, 120, 120], vf=[120, 120, 120])]),
              n_steps=1000, batch_size=5000, n_epochs=10, gamma=0.999, seed=5)
    env = Quadcopter3DGates(100, *square_track(), gates_ahead=1, infos_mode="none", seed=3)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    m = PPO("MlpPolicy", env, **kw)
    assert m._trainer.native_update
    theta0 = m._trainer._updater.theta.clone()
    m.learn(total_timesteps=2 * 100 * 1000)
    st = m._trainer.stats
    assert m.num_timesteps == 200000 and st["updates"] == 2 * 10 * 20 and st["skipped_nonfinite"] == 0 and np.isfinite(st["loss"])
    assert torch.isfinite(m._trainer._updater.theta).all() and not torch.equal(m._trainer._updater.theta, theta0)
    env.close()
    env = Quadcopter3DGates(1000, *square_track(), gates_ahead=1, infos_mode="none", seed=3)
    m = PPO("MlpPolicy", env, **dict(kw, n_steps=10, batch_size=3000))      # 10 000 rows % 3000 != 0
    assert not m._trainer.native_update
    m.learn(total_timesteps=10 * 1000)
    assert m.num_timesteps == 10000 and np.isfinite(m.ep_info.get("loss", 0.0))
    env.close()


def test_gather_rollout_over_rccl_at_config4_size_stays_within_its_buffers():
    """BASELINE config 4's exchange on the real backend (one rank: this box has one GPU): a 32 768-env x
    64-step rollout shard gathered with RolloutGather over RCCL -- peak device memory during the gather <= 1.1 x the gathered
    bytes on the first call (the receive buffers themselves) and ~0 on the second (buffers reused); contents equal the shard."""
    code = r'''
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29541")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, zigzag_track
from optimal_quad_control_rl_amd.sharded import ShardedRaceEnv
def factory(n, base):
    e = Quadcopter3DGates(n, *zigzag_track(), gates_ahead=1, infos_mode="none", seed=0, env_id_base=base)
    e.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    return e
env = ShardedRaceEnv(32768, factory)
env.reset()
K = 64
acts = torch.rand((K, 32768, 4), device="cuda") * 2 - 1
obs, rew, done, trunc = env.rollout(acts)
torch.cuda.synchronize()
base = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
g = env.gather_rollout(obs, rew, done)
torch.cuda.synchronize()
peak1 = torch.cuda.max_memory_allocated() - base
torch.cuda.reset_peak_memory_stats()
base2 = torch.cuda.memory_allocated()
g2 = env.gather_rollout(obs, rew, done)
torch.cuda.synchronize()
peak2 = torch.cuda.max_memory_allocated() - base2
ok = bool(torch.equal(g.obs[0], obs) and torch.equal(g.rew[0], rew) and torch.equal(g.done[0], done) and g2.obs.data_ptr() == g.obs.data_ptr())
ro, rr, rd = g.rows()
ok = ok and ro.shape == (K * 32768, obs.shape[-1]) and ro.data_ptr() == g.obs.data_ptr()
print(json.dumps(dict(gathered=g.nbytes, peak1=peak1, peak2=peak2, ok=ok, shard=obs.numel() * 4 + rew.numel() * 4 + done.numel(),
                      backend=dist.get_backend(), world=dist.get_world_size())))
dist.destroy_process_group()
''' % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    import json

    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["ok"] and j["backend"] == "nccl" and j["world"] == 1
    assert j["gathered"] == j["shard"] == 64 * 32768 * (24 * 4 + 4 + 1)
    assert j["peak1"] <= 1.1 * j["gathered"], j
    assert j["peak2"] <= 0.01 * j["gathered"], j


def test_f16_operand_gradient_vs_f32_autograd_on_real_rollout_rows():
    """the matrix-core gradient (f16 operands, f32 accumulation) against plain f32 torch autograd on the rows
    of a REAL rollout (the closed-loop kernel's observations / actions / log-probs, GAE advantages), B = 16 384: cosine
    similarity >= 0.999 for every parameter tensor of both networks and for log_std."""
    import math

    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd.ppo import PPO as Trainer

    n, T, B = 16384, 8, 16384
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=2)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    tr = Trainer(env, n_steps=T, batch_size=B, n_epochs=1, gamma=0.999, seed=0, fused_collect=True, native_update=True)
    for _ in range(3):          # a few updates away from the initial policy, so that ratios are not all 1
        tr.collect(); tr.train()
    tr.collect()
    adv, ret = tr._gae_native()
    rows = T * n
    obs, act = tr.buf_obs.view(rows, -1), tr.buf_act.view(rows, 4)
    old_lp, adv, ret = tr.buf_lp.view(rows).contiguous(), adv.view(rows).contiguous(), ret.view(rows).contiguous()
    idx = torch.randperm(rows, device=env.device)[:B].to(torch.int32)
    g = tr._updater.grad(obs, act, old_lp, adv, ret, idx, 0.2, 0.5, 0.0)[:-4]
    # f32 autograd of the same loss (SB3's: clipped surrogate + 0.5 mse, per-minibatch advantage normalisation)
    pol = tr.policy
    for p_ in pol.parameters():
        p_.grad = None
    with torch.enable_grad():
        li = idx.long()
        a = adv[li]
        a = (a - a.mean()) / (a.std() + 1e-8)
        lp, _ = pol.log_prob_entropy(obs[li], act[li])
        ratio = (lp - old_lp[li]).exp()
        pg = -torch.min(a * ratio, a * ratio.clamp(0.8, 1.2)).mean()
        vl = torch.nn.functional.mse_loss(pol.value(obs[li]), ret[li])
        (pg + 0.5 * vl).backward()
    off = 0
    worst = 1.0
    names = []
    for net in (pol.pi, pol.vf):
        for lin in [m for m in net if isinstance(m, torch.nn.Linear)]:
            names += [lin.weight, lin.bias]
    names.append(pol.log_std)
    for p_ in names:
        k = p_.numel()
        ref = p_.grad.reshape(-1).double()
        got = g[off:off + k].double()
        off += k
        if ref.norm() == 0 and got.norm() == 0:
            continue
        cos = float((ref @ got) / (ref.norm() * got.norm()))
        worst = min(worst, cos)
        assert cos >= 0.999, (tuple(p_.shape), cos)
        assert 0.9 < float(got.norm() / ref.norm()) < 1.1
    assert off == g.numel() and math.isfinite(worst)
    env.close()


def test_epoch_graph_equals_minibatch_launches_and_counts_real_steps():
    """qr_ppo_epoch (one replayed hipGraph per epoch) against the same updates as stream launches (qr_ppo_epoch_begin + M x
    qr_ppo_minibatch): identical parameters and Adam moments bit for bit over two epochs with different permutations (the second
    epoch REPLAYS the graph captured by the first: the permutation buffer is rewritten in place, the Adam step count and the
    learning rate live on the device).  And the device-resident step count advances only for steps really taken:
    with a tiny target_kl the first epoch stops early, and `step` equals `applied`, not the number of launches."""
    from test_gpu_ppo_kernel import _setup
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    L, B, M = 24, 4096, 6
    pol, ref, up_a, obs, act, old_lp, adv, ret = _setup(L, rows=B * M, seed=11, max_minibatch=B)
    up_b = MfmaPpoUpdater(pol, L, obs.device, max_minibatch=B)
    up_b.theta.copy_(up_a.theta); up_b.pack()
    dev = obs.device
    perm_buf = torch.empty(B * M, dtype=torch.int32, device=dev)
    for ep, lr in enumerate((3e-4, 1e-4)):
        perm = torch.randperm(B * M, device=dev, generator=torch.Generator(device=dev).manual_seed(ep)).to(torch.int32)
        perm_buf.copy_(perm)
        up_a.control(None, clear=True); up_b.control(None, clear=True)
        up_a.epoch(obs, act, old_lp, adv, ret, perm_buf, B, lr)
        up_b.begin_epoch(adv, perm, B)
        for k in range(M):
            up_b.minibatch(obs, act, old_lp, adv, ret, perm[k * B:(k + 1) * B], lr)
        torch.cuda.synchronize()
        assert torch.equal(up_a.theta, up_b.theta) and torch.equal(up_a.m, up_b.m) and torch.equal(up_a.v, up_b.v), ep
        assert up_a.status()[1] == M and up_a.step == up_b.step == M * (ep + 1)
    # SB3's early stop: KL limit far below what one step moves -> the epoch stops after its first step or two
    before = up_a.step
    up_a.control(1e-9, clear=True)
    up_a.epoch(obs, act, old_lp, adv, ret, perm_buf, B, 3e-4)
    stopped, applied, skipped, timeouts = up_a.status()
    assert stopped and applied < M and timeouts == 0
    assert up_a.step == before + applied          # launches that became no-ops did not advance the bias-correction count
    up_a.step = 1234                              # checkpoint restore path
    assert up_a.step == 1234
    up_a.close(); up_b.close()


def test_device_shuffle_is_a_fresh_permutation_every_epoch_and_is_checkpointable():
    """qr_ppo_epoch(device_shuffle): the permutation buffer is filled by a keyed Feistel bijection per epoch.  Every epoch's buffer
    is a permutation of [0, rows) (also for a row count that is not a power of two: cycle walking), consecutive epochs differ, the
    sequence is a function of (seed, epoch count) -- restoring the state replays it -- and it looks uniform (position / value
    correlation and fixed points like a random permutation's).  num_epochs epochs in one graph == the same epochs launched singly."""
    from test_gpu_ppo_kernel import _setup
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    for B, M in ((4096, 8), (192, 5)):
        L = 17
        pol, ref, up_a, obs, act, old_lp, adv, ret = _setup(L, rows=B * M, seed=3, max_minibatch=B)
        up_b = MfmaPpoUpdater(pol, L, obs.device, max_minibatch=B)
        up_b.theta.copy_(up_a.theta); up_b.pack()
        rows = B * M
        pa = torch.empty(rows, dtype=torch.int32, device=obs.device)
        pb = torch.empty(rows, dtype=torch.int32, device=obs.device)
        up_c = MfmaPpoUpdater(pol, L, obs.device, max_minibatch=B)   # replays the permutations through LOADED indices
        up_c.theta.copy_(up_a.theta); up_c.pack()
        up_a.set_shuffle(1234, 0); up_b.set_shuffle(1234, 0)
        seen = []
        for ep in range(3):
            up_a.epoch(obs, act, old_lp, adv, ret, pa, B, 3e-4, device_shuffle=True)
            torch.cuda.synchronize()
            q = pa.cpu().long()
            assert torch.equal(torch.sort(q).values, torch.arange(rows)), (B, M, ep)
            seen.append(q)
            assert up_a.shuffle_state() == (1234, ep + 1)
            # the epoch graph and the same rows fed through stream launches, minibatch by minibatch: same parameters bit for bit
            pc = pa.clone()
            up_c.begin_epoch(adv, pc, B)
            for k in range(M):
                up_c.minibatch(obs, act, old_lp, adv, ret, pc[k * B:(k + 1) * B], 3e-4)
            torch.cuda.synchronize()
            assert torch.equal(up_a.theta, up_c.theta) and torch.equal(up_a.v, up_c.v), (B, M, ep)
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
        if rows > 10000:
            pos = torch.arange(rows, dtype=torch.float64)
            for q in seen:
                r = torch.corrcoef(torch.stack([pos, q.double()]))[0, 1]
                assert abs(float(r)) < 0.02 and int((q == torch.arange(rows)).sum()) <= 8
                # minibatch k draws its rows from the whole buffer, not from a neighbourhood
                first = q[:B].double()
                assert abs(float(first.mean()) / rows - 0.5) < 0.02 and float(first.std()) / rows > 0.27
        # three epochs in ONE graph from the same state: same permutations (last one left in the buffer), same parameters
        up_b.epoch(obs, act, old_lp, adv, ret, pb, B, 3e-4, num_epochs=3, device_shuffle=True)
        torch.cuda.synchronize()
        assert torch.equal(pb.cpu().long(), seen[2]) and up_b.shuffle_state() == (1234, 3)
        assert torch.equal(up_a.theta, up_b.theta) and torch.equal(up_a.m, up_b.m) and up_a.step == up_b.step == 3 * M
        # restoring (seed, count) replays the sequence
        up_a.set_shuffle(1234, 1)
        up_a.epoch(obs, act, old_lp, adv, ret, pa, B, 3e-4, device_shuffle=True)
        torch.cuda.synchronize()
        assert torch.equal(pa.cpu().long(), seen[1])
        up_a.close(); up_b.close(); up_c.close()


def test_target_kl_guard_halves_the_learning_rate_instead_of_stalling():
    """VERDICT r02 item 6 / the seed-3 stall of round 2: when SB3's target_kl rule ends `patience` consecutive train() calls after
    at most one optimiser step, the learning rate is halved (and keeps being halved) rather than leaving the run stuck at one
    step per rollout for ever.  A limit far below what a single step moves forces the situation."""
    from optimal_quad_control_rl_amd import Quadcopter3DGatesINDI, square_track
    from optimal_quad_control_rl_amd.ppo import PPO as Trainer

    env = Quadcopter3DGatesINDI(4096, *square_track(), gates_ahead=1, infos_mode="none", seed=4)
    tr = Trainer(env, n_steps=8, batch_size=4096, n_epochs=3, gamma=0.999, seed=0, target_kl=1e-9, fused_collect=True, native_update=True)
    lrs = []
    for _ in range(8):
        tr.collect(); tr.train()
        lrs.append(tr.opt.param_groups[0]["lr"])
        assert tr.stats["early_stop"]
    assert tr._kl_lr_scale <= 0.25 and tr.stats["kl_lr_halvings"] >= 2, (tr._kl_lr_scale, tr.stats)
    assert lrs[-1] < lrs[0] and lrs[0] == pytest.approx(3e-4)
    # and an unarmed trainer (the reference's target_kl = None) never touches the learning rate
    tr2 = Trainer(env, n_steps=8, batch_size=4096, n_epochs=2, gamma=0.999, seed=0, target_kl=None, fused_collect=True, native_update=True)
    for _ in range(4):
        tr2.collect(); tr2.train()
    assert tr2._kl_lr_scale == 1.0 and "kl_lr_halvings" not in tr2.stats and tr2.stats["updates"] == 4 * 2 * (8 * 4096 // 4096)
    env.close()


def test_sb3_infos_under_pause_if_collision_hand_back_the_frozen_observation():
    """with pause_if_collision there is no auto-reset (R:573-578), so the kernels write no terminal-observation row;
    `infos_mode="sb3"` must hand back the observation of the frozen env itself (what the reference's `self.states[i]` is in that
    mode), not a stale row of the terminal-observation buffer."""
    from optimal_quad_control_rl_amd import Quadcopter3DGatesINDI, square_track

    n = 256
    env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=1, pause_if_collision=True, infos_mode="sb3", seed=9)
    env.reset()
    env.max_steps = 30
    rng = np.random.default_rng(0)
    seen = 0
    for k in range(40):
        obs, rew, done, infos = env.step(rng.uniform(-1, 1, size=(n, 4)).astype(np.float32))
        assert len(infos) == n
        for i in np.nonzero(done)[0]:
            np.testing.assert_array_equal(infos[i]["terminal_observation"], obs[i])
            assert infos[i]["TimeLimit.truncated"] in (True, False)
            seen += 1
        for i in np.nonzero(~done)[0][:4]:
            assert infos[i] == {}
    assert seen > 0
    env.close()


def _shuffle_reference(n, seed, count):
    """NumPy restatement of ppo_shuffle_kernel (csrc/quadrace_ppo.hip): keyed 8-round alternating Feistel network over
    ceil(log2 n) bits (at least 2), cycle-walked into [0, n); round keys = SplitMix64 finaliser of (seed, count, round)."""
    M64 = (1 << 64) - 1
    bits = 2
    while (1 << bits) < n:
        bits += 1
    lb = bits >> 1
    rb = bits - lb
    lmask, rmask = np.uint32((1 << lb) - 1), np.uint32((1 << rb) - 1)
    keys = []
    for r in range(8):
        z = (seed + 0x9E3779B97F4A7C15 * ((count * 8 + r + 1) & M64)) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        keys.append(np.uint32((z ^ (z >> 31)) & 0xFFFFFFFF))

    def mix(x, k):
        with np.errstate(over="ignore"):
            h = x * np.uint32(0x9E3779B1) + k
            h ^= h >> np.uint32(15); h = h * np.uint32(0x85EBCA77)
            h ^= h >> np.uint32(13); h = h * np.uint32(0xC2B2AE3D)
            h ^= h >> np.uint32(16)
        return h

    x = np.arange(n, dtype=np.uint32)
    todo = np.ones(n, dtype=bool)
    first = True
    while todo.any():
        xs = x[todo]
        l, r_ = xs >> np.uint32(rb), xs & rmask
        for r in range(0, 8, 2):
            l = l ^ (mix(r_, keys[r]) & lmask)
            r_ = r_ ^ (mix(l, keys[r + 1]) & rmask)
        x[todo] = (l << np.uint32(rb)) | r_
        todo = x >= n if first else (todo & (x >= n))
        first = False
        todo = x >= n
    return x.astype(np.int64)


@pytest.mark.parametrize("B,M,seed", [(4096, 8, 1234), (192, 5, 7), (64, 1, 2 ** 40 + 3)])
def test_device_shuffle_equals_its_numpy_restatement(B, M, seed):
    """The on-device epoch permutation against an independent NumPy restatement of the same keyed bijection, for a power-of-two
    row count, one that needs cycle walking, and the smallest minibatch: identical permutations for consecutive epochs."""
    from test_gpu_ppo_kernel import _setup

    L = 17
    pol, ref, up, obs, act, old_lp, adv, ret = _setup(L, rows=B * M, seed=3, max_minibatch=B)
    rows = B * M
    perm = torch.empty(rows, dtype=torch.int32, device=obs.device)
    up.set_shuffle(seed, 0)
    for ep in range(3):
        up.epoch(obs, act, old_lp, adv, ret, perm, B, 3e-4, device_shuffle=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(perm.cpu().numpy().astype(np.int64), _shuffle_reference(rows, seed, ep))
    up.close()
