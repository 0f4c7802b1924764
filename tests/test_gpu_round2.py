"""GPU: round-2 parity hardening -- full-size lock-step through auto-resets, the residual
MLP / body velocity pinned DIRECTLY against the reference's fixture rows, true terminal observations, the 8-shard
partition of BASELINE config 4 on one GPU, and the complete config-5 training loop at 65 536 envs."""
import numpy as np
import pytest
import torch

import parity as P

pytestmark = pytest.mark.gpu

E2E, INDI = 0, 1


@pytest.fixture(scope="module")
def PA():
    assert torch.cuda.is_available()
    from product_adapter import ProductAdapter

    return ProductAdapter


@pytest.fixture(scope="module")
def OA():
    from oracle_adapter import OracleAdapter

    return OracleAdapter


def _pair(PA, OA, variant, n, tname, ga, blob, seed=11, env_id_base=0):
    trk = P.tracks()[tname]
    kw = dict(gates_ahead=ga, residual=blob if variant == E2E else None,
              dist_ranges=P.TRAIN_DIST_RANGES if variant == E2E else None, seed=seed, env_id_base=env_id_base)
    return PA(variant, n, trk, **kw), OA(variant, n, trk, **kw)


def test_residual_and_body_velocity_match_reference_rows_directly(PA, residual_blob):
    """F1 (reference: get_body_velocity R:155, thrust_moment_model_world_states R:254-262 on 257 states): the device
    functions the step kernels inline, read back through qr_probe_residual -- no finite differences."""
    d = P.load("f1_residual")
    s = d["states"]
    n = s.shape[0]
    a = PA(E2E, n, P.tracks()["zigzag"], gates_ahead=0, residual=residual_blob)
    a.set_state(s, np.zeros((n, 6), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    out = a.env.probe_residual().cpu().numpy().astype(np.float64)
    ref = np.concatenate([d["vb"], d["thrust"].reshape(n, 1), d["moment"]], axis=1).astype(np.float64)
    err = np.abs(out - ref) / np.maximum(1.0, np.abs(ref))
    assert err[:, :3].max() < 1e-5, err[:, :3].max()        # body velocity
    assert err[:, 3].max() < 1e-5, err[:, 3].max()          # residual thrust (values up to ~40)
    assert err[:, 4:].max() < 1e-5, err[:, 4:].max()        # residual moments
    # the notebook's own printed known answer (R:184+), state = [0..15]
    assert abs(out[0, 3] - 36.098232) < 2e-4
    np.testing.assert_allclose(out[0, 4:], [0.2847767, -0.22512697, -0.05896095], rtol=0, atol=2e-6)


@pytest.mark.parametrize("variant", [E2E, INDI])
def test_full_size_lockstep_through_resets_vs_oracle(PA, OA, variant, residual_blob):
    """BASELINE size N = 65 536, 64 teacher-forced steps through auto-resets (max_steps = 40 truncates every env once;
    random actions crash many more): dones / targets / step counts exact, freshly reset lanes bit-exact, integrated lanes
    within the one-step tolerance.  Every env whose `done` differs is shown to sit < 1e-5 from a termination threshold
    (parity.knife_edge_margin, from the oracle's pre-step state), and the whole run may hold at most 8 of them."""
    n, K = 65536, 64
    tname = "zigzag" if variant == E2E else "square"
    g, o = _pair(PA, OA, variant, n, tname, 1, residual_blob, seed=21)
    o.env.set_threads(16)
    g.env.max_steps = 40
    o.env.set_limits(40, 0.01)
    g.reset(); o.reset()
    rng = np.random.default_rng(31)
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
        mismatches += P.assert_knife_edges(variant, mism, wo, a, do, residual_blob, P.tracks()[tname], to, where=f"step {k}")
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
        if live.any():   # (at the time-limit step of a crash-free batch every env is done at once)
            worst_state = max(worst_state, float(P.rel_err(wg[live], wo2[live]).max()))
        worst_obs = max(worst_obs, float(P.obs_err(og[ok], oo[ok], wo2[ok]).max()))
        tot_done += int(dno.sum())
    assert worst_state < P.TOL_STEP_STATE and worst_obs < P.TOL_STEP_OBS, (worst_state, worst_obs)
    assert tot_done >= n and mismatches <= 8, (tot_done, mismatches)


@pytest.mark.parametrize("variant", [E2E, INDI])
def test_terminal_observation_vs_oracle_and_across_kernels(PA, OA, variant, residual_blob):
    """qr_set_terminal_obs: every env that finishes writes the observation of its FINAL state (before the auto-reset).
    (a) per-step kernel vs the oracle twin; (b) the fused rollout kernel and the captured per-step launches write the same
    rows [k][env] bit for bit; rows of unfinished envs stay untouched."""
    n, K = 4096, 48
    g, o = _pair(PA, OA, variant, n, "square", 2, residual_blob, seed=5)
    L = g.env.state_len
    g.env.max_steps = 30
    o.env.set_limits(30, 0.01)
    g.reset(); o.reset()
    tbuf = torch.full((n, L), -7.0, device=g.env.device)
    g.env.set_terminal_obs_buffer(tbuf)
    obuf = np.full((n, L), -7.0, np.float32)
    o.env.set_terminal_obs(obuf)
    rng = np.random.default_rng(77)
    seen = 0
    for k in range(K):
        wo, do, to, so = o.get_state()
        g.set_state(wo, do if variant == E2E else None, to, so)
        g.env.set_state_tensors(episode=o.env.episode.astype(np.int64))
        tbuf.fill_(-7.0); obuf[:] = -7.0
        a = rng.uniform(-1, 1, size=(n, 4)).astype(np.float32)
        _, _, dng, _ = g.step(a)
        _, _, dno, _ = o.step(a)
        t = tbuf.cpu().numpy()
        both = dng & dno
        assert (t[~dng] == -7.0).all() and (obuf[~dno] == -7.0).all()       # untouched rows
        if both.any():
            wfin = None
            err = P.obs_err(t[both], obuf[both])
            assert err.max() < P.TOL_STEP_OBS, err.max()
            seen += int(both.sum())
    assert seen >= n   # every env was truncated at least once
    g.env.set_terminal_obs_buffer(None)
    # (b) K-step kernels: same rows from the fused kernel and from the per-step launches
    from optimal_quad_control_rl_amd import Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES

    cls = Quadcopter3DGates if variant == E2E else Quadcopter3DGatesINDI
    outs = []
    acts = torch.rand((K, n, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 2 - 1
    for mode in ("fused", "launches"):
        e = cls(n, *P.tracks()["square"], gates_ahead=2, seed=9, infos_mode="none")
        if variant == E2E:
            e.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        e.max_steps = 30
        e.reset_device()
        tb = torch.full((K, n, L), -7.0, device=e.device)
        e.set_terminal_obs_buffer(tb)
        if mode == "fused":
            res = e.rollout_device(acts)
        else:
            res = (torch.empty((K, n, L), device=e.device), torch.empty((K, n), device=e.device),
                   torch.empty((K, n), dtype=torch.uint8, device=e.device), torch.empty((K, n), dtype=torch.uint8, device=e.device))
            e.step_sequence_device(acts, res)
        torch.cuda.synchronize()
        outs.append((tb.clone(), res[2].clone()))
        e.close()
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])
    done = outs[0][1].bool()
    assert done.sum() >= n and (outs[0][0][~done] == -7.0).all() and (outs[0][0][done] != -7.0).any(dim=-1).all()


def test_eight_shards_of_32768_equal_one_262144_env_handle():
    """BASELINE config 4 (262 144 envs = 8 x 32 768) on ONE GPU: eight handles with env_id_base = r * 32 768, stepped one
    after the other, produce bit for bit the rows [r * 32 768, (r + 1) * 32 768) of a single 262 144-env handle -- reset,
    20 fused steps with auto-resets, final state."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, zigzag_track

    n, R, K = 32768, 8, 20
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(123)
    acts = torch.rand((K, n * R, 4), device=dev, generator=gen) * 2 - 1

    def make(num, base):
        e = Quadcopter3DGates(num, *zigzag_track(), gates_ahead=1, seed=17, env_id_base=base, infos_mode="none")
        e.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        e.max_steps = 12   # truncations inside the window on top of the crashes
        return e

    big = make(n * R, 0)
    obs0 = big.reset_device().clone()
    ob, rb, db, tb = big.rollout_device(acts)
    wb = big.get_state_tensors()[0]
    assert int(db.sum()) >= n * R   # every env is auto-reset at least once inside the window
    for r in range(R):
        sl = slice(r * n, (r + 1) * n)
        e = make(n, r * n)
        assert torch.equal(e.reset_device(), obs0[sl])
        o, rw, d, t = e.rollout_device(acts[:, sl].contiguous())
        assert torch.equal(o, ob[:, sl]) and torch.equal(rw, rb[:, sl]) and torch.equal(d, db[:, sl]) and torch.equal(t, tb[:, sl])
        assert torch.equal(e.get_state_tensors()[0], wb[sl])
        e.close()
    big.close()


@pytest.mark.parametrize("variant", ["indi", "e2e"])
def test_config5_training_loop_at_full_size(variant):
    """BASELINE config 5 as a whole loop at 65 536 envs: three iterations of closed-loop collection in one kernel
    (qr_rollout_policy) + value forward + GAE with the time-limit bootstrap + 2 epochs x 32 matrix-core minibatch updates,
    the reference's gamma = 0.999 (R:784-795)."""
    from optimal_quad_control_rl_amd import (Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES, square_track)
    from optimal_quad_control_rl_amd.ppo import PPO

    n, T = 65536, 32
    if variant == "indi":
        env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=1, seed=1, infos_mode="none")
    else:
        env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, seed=1, infos_mode="none")
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = 48    # time-limit truncations inside the three rollouts
    ppo = PPO(env, n_steps=T, batch_size=n * T // 32, n_epochs=2, gamma=0.999, fused_collect=True, native_update=True, seed=0,
              target_kl=None)
    theta0 = ppo._updater.theta.clone()
    for it in range(3):
        ppo.collect()
        if it >= 1:
            assert ppo.stats["truncations"] > 0 and float(ppo.buf_term_val.abs().sum()) > 0
            tr = ppo._trunc_u8.bool()
            assert (ppo.buf_term_val[~tr] == 0).all()
        ppo.train()
        assert ppo.stats["updates"] == 64 * (it + 1) and not ppo.stats["early_stop"] and ppo.stats["skipped_nonfinite"] == 0
    assert ppo.num_timesteps == 3 * n * T
    assert torch.isfinite(ppo._updater.theta).all() and not torch.equal(ppo._updater.theta, theta0)
    assert np.isfinite(ppo.stats["loss"]) and ppo.stats["approx_kl"] >= 0 and ppo.stats["episodes"] > 0
    env.close()


FAKE_SB3 = '''
import warnings
from abc import ABC, abstractmethod


class VecEnv(ABC):
    """The parts of stable_baselines3 2.1 `VecEnv` the reference class relies on (constructor contract incl. the
    `get_attr("render_mode")` probe that R:603-604 answers with AttributeError, abstract method set, step())."""

    def __init__(self, num_envs, observation_space, action_space):
        self.num_envs = num_envs
        self.observation_space = observation_space
        self.action_space = action_space
        self.reset_infos = [{} for _ in range(num_envs)]
        self._seeds = [None for _ in range(num_envs)]
        self._options = [{} for _ in range(num_envs)]
        try:
            render_modes = self.get_attr("render_mode")
        except AttributeError:
            warnings.warn("The `render_mode` attribute is not defined in your environment. It will be set to None.")
            render_modes = [None for _ in range(num_envs)]
        assert all(m == render_modes[0] for m in render_modes)
        self.render_mode = render_modes[0]

    @abstractmethod
    def reset(self): ...
    @abstractmethod
    def step_async(self, actions): ...
    @abstractmethod
    def step_wait(self): ...
    @abstractmethod
    def close(self): ...
    @abstractmethod
    def get_attr(self, attr_name, indices=None): ...
    @abstractmethod
    def set_attr(self, attr_name, value, indices=None): ...
    @abstractmethod
    def env_method(self, method_name, *method_args, indices=None, **method_kwargs): ...
    @abstractmethod
    def env_is_wrapped(self, wrapper_class, indices=None): ...

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()
'''

SB3_CHILD = '''
import sys, warnings, numpy as np
sys.path.insert(0, %r)
import stable_baselines3.common.vec_env as sb3v
from optimal_quad_control_rl_amd import Quadcopter3DGates, zigzag_track
from optimal_quad_control_rl_amd import vec_env as V
assert V._SB3VecEnv is sb3v.VecEnv and issubclass(Quadcopter3DGates, sb3v.VecEnv)
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    env = Quadcopter3DGates(64, *zigzag_track(), gates_ahead=1)           # would raise TypeError if an abstract method were missing
assert any("render_mode" in str(x.message) for x in w)                    # the R:603-604 path: get_attr raised AttributeError
assert env.render_mode is None and len(env.reset_infos) == 64 and env.num_envs == 64
obs = env.reset()
assert obs.shape == (64, env.observation_space.shape[0]) and env.action_space.shape == (4,)
o, r, d, infos = env.step(np.zeros((64, 4), np.float32))                  # the BASE class's step(): step_async + step_wait
assert o.shape == obs.shape and r.shape == (64,) and d.dtype == bool and len(infos) == 64
assert env.env_is_wrapped(object) == [False] * 64
# attribute idioms of the reference-side harness (R:4499-4500): in-place edits reach the device
env.world_states[3] = np.arange(16, dtype=np.float32)
env.target_gates[:] = 2
assert (env.world_states[3] == np.arange(16)).all() and (env.target_gates == 2).all()
env.pause_if_collision = True                                             # plain attribute in the reference (R:293): assignable
env.step_counts[:] = env.max_steps - 1
ws = env.world_states.copy()
o, r, d, _ = env.step(np.zeros((64, 4), np.float32))
assert d.all() and (env.world_states == ws).all()                         # done envs frozen, not reset (R:573-578)
env.pause_if_collision = False
o, r, d, _ = env.step(np.zeros((64, 4), np.float32))
assert d.all() and (env.step_counts == 0).all()                           # auto-reset again
print("sb3 child ok")
'''


def test_derives_from_sb3_vecenv_when_present(tmp_path):
    """The reference class IS an SB3 VecEnv (R:287).  SB3 is not installable here, so a stand-in package with SB3 2.1's
    constructor contract is put on the path of a child process: the adapter must pick it up as its base class, satisfy the
    abstract method set and survive the `get_attr("render_mode")` probe exactly like the reference does."""
    import os
    import subprocess
    import sys

    pkg = tmp_path / "stable_baselines3" / "common"
    pkg.mkdir(parents=True)
    (tmp_path / "stable_baselines3" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "vec_env.py").write_text(FAKE_SB3)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=str(tmp_path) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", SB3_CHILD % root], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "sb3 child ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_step_launches_graph_follows_configuration_changes():
    """qr_step_launches replays a captured graph while (K, buffers, env configuration) are unchanged; the kernel parameters
    are baked into the graph nodes, so ANY configuration change between two calls must re-capture: same buffers, but
    max_steps / pause / disturbance table edited in between -- results must equal a fresh env doing the same."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, zigzag_track

    n, K = 4096, 12
    dev = torch.device("cuda", 0)
    acts = torch.rand((K, n, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 2 - 1

    def make():
        e = Quadcopter3DGates(n, *zigzag_track(), gates_ahead=1, seed=3, infos_mode="none")
        e.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        return e

    def buffers(e):
        L = e.state_len
        return (torch.empty((K, n, L), device=dev), torch.empty((K, n), device=dev),
                torch.empty((K, n), dtype=torch.uint8, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev))

    a, b = make(), make()
    out_a, out_b = buffers(a), buffers(b)
    a.reset_device(); b.reset_device()
    a.step_sequence_device(acts, out_a)                 # captures the graph
    a.step_sequence_device(acts, out_a)                 # replays it
    b.rollout_device(acts, out_b); b.rollout_device(acts, out_b)
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b))
    for e in (a, b):
        e.max_steps = 30                                # every env is truncated inside the next window
    a.step_sequence_device(acts, out_a)                 # same K, same buffers: must NOT replay the old parameters
    b.rollout_device(acts, out_b)
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b)) and int(out_a[3].sum()) >= n
    for e in (a, b):
        e.pause = True
    before = a.get_state_tensors()[0].clone()
    a.step_sequence_device(acts, out_a); b.rollout_device(acts, out_b)
    assert torch.equal(a.get_state_tensors()[0], before) and torch.equal(out_a[1], out_b[1]) and int(out_a[2].sum()) == 0
    for e in (a, b):
        e.pause = False
        e.disturbance_scale = 0.0                       # table edit: resets draw zero disturbances from now on
        e.max_steps = 5
    a.step_sequence_device(acts, out_a); b.rollout_device(acts, out_b)
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b))
    assert float(a.get_state_tensors()[1].abs().max()) == 0.0
    # the action CONTENT may change under the same pointer: the graph reads the buffer at replay time
    acts2 = acts.clone()
    acts.mul_(-1.0)
    a.step_sequence_device(acts, out_a); b.rollout_device(acts, out_b)
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b))
    a.close(); b.close()


def test_sb3_infos_mode_hands_out_true_terminal_observations():
    """infos_mode="sb3": per-env dicts; `terminal_observation` = the observation of the episode's FINAL state (not the first row of
    the next episode, which is what obs[i] already holds), `TimeLimit.truncated` only where the time limit ended the episode."""
    from optimal_quad_control_rl_amd import Quadcopter3DGatesINDI, square_track

    n = 512
    env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=1, seed=2, infos_mode="sb3")
    env.max_steps = 25
    env.reset()
    rng = np.random.default_rng(4)
    seen = 0
    for k in range(60):
        a = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        pre = env.world_states.copy(); pre_t = env.target_gates.copy(); pre_s = env.step_counts.copy()
        obs, rew, done, infos = env.step(a)
        assert len(infos) == n and all((("terminal_observation" in infos[i]) == bool(done[i])) for i in range(n))
        if done.any():
            # (the values themselves are pinned against the oracle in test_terminal_observation_vs_oracle_and_across_kernels)
            for i in np.nonzero(done)[0][:8]:
                t = infos[i]["terminal_observation"]
                assert t.shape == (env.state_len,) and np.isfinite(t).all()
                assert not np.allclose(t, obs[i])                      # not the post-reset row
                assert infos[i]["TimeLimit.truncated"] == bool(pre_s[i] + 1 >= 25)
                # position part of the observation is continuous with the pre-step state (one 10 ms Euler step apart)
                assert np.abs(t[5:8] - pre[i][5:8]).max() < 1.0
            seen += int(done.sum())
    assert seen > n
    env.close()


def test_bench_collectives_over_rccl_on_one_rank():
    """`bench.py` launched exactly as the driver launches a multi-GPU run (torch.distributed.run, one rank per GPU) with
    QR_BENCH_FORCE_DIST=1: ONE rank, but the process group is RCCL ("nccl" backend on ROCm) and every collective of the
    N > 1 path runs on the device -- init, barrier, MAX all-reduce of the timings, all-gather of the packed rollout shard,
    and the config-4 object.  (tests/test_bench_gloo.py covers world 2 on CPU; this is the same code on the real backend.)"""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, QR_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29517", os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5",
           "--envs", "32768", "--repeats", "2", "--no-cpu-baseline", "--no-parity", "--full"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 4096, "stdout carries ONE compact JSON line"
    j = json.loads(lines[0])
    assert j["n_gpus"] == 1 and j["value"] > 1e9
    assert j["rccl"]["rccl_world_size"] == 1 and j["rccl"]["backend"] == "nccl" and j["rccl"]["rccl_version"][0].isdigit()
    assert len(j["rccl"]["per_rank_ms_per_step"]) == 1
    assert j["exchange"]["ms"] > 0 and j["config4"]["envs_per_gpu"] == 32768 and j["config4"]["exchange_ms"] > 0
    # the full object goes to stderr (and to bench_out/bench_full_*.json)
    full = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith("{")][-1])
    ex = full["exchange"]
    assert ex["gathered_shape"][:2] == [1, ex["steps"]] and ex["gathered_bytes"] == ex["bytes_per_rank"]
    c4 = full["config4"]
    assert c4["exchange"]["bytes_per_rank"] > 0 and c4["value_incl_exchange"] > 0


def test_data_parallel_training_over_rccl_on_one_rank():
    """tools/train_ppo.py under torch.distributed.run with one rank: the data-parallel update path (qr_ppo_grad -> RCCL
    all-reduce of the [n + 4] gradient + statistics vector -> qr_ppo_apply, parameter broadcast) runs on the real backend
    and the run still learns something (a few iterations: the surrogate statistics are finite and steps were counted)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29519", os.path.join(root, "tools", "train_ppo.py"), "--variant", "indi", "--envs", "8192",
           "--n-steps", "32", "--steps", "2e6", "--fused", "--native-update"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["world_size"] == 1 and j["train_steps"] >= 2e6 and j["native_update"] and j["fused_collect"]
    assert np.isfinite(j["eval_gates_per_12s"]) and j["train_Msteps_per_s"] > 1.0


def test_numpy_step_path_buffers_and_async_semantics():
    """SB3-facing NumPy path: same numbers as the device path; the observation array is the env's own (alternating) pinned buffer
    -- intact during the NEXT step, recycled by the one after --, rewards / dones are fresh arrays; step_async() enqueues the
    device work and step_wait() without a new step_async() steps again with the stored actions (reference behaviour, R:498-501)."""
    from optimal_quad_control_rl_amd import Quadcopter3DGatesINDI, square_track

    n = 1024
    a_env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=1, seed=5, infos_mode="reference")
    b_env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=1, seed=5, infos_mode="none")
    o0 = a_env.reset()
    b_env.reset_device()
    rng = np.random.default_rng(8)
    acts = [rng.uniform(-1, 1, (n, 4)).astype(np.float32) for _ in range(4)]
    outs = []
    for k in range(3):
        a_env.step_async(acts[k])
        obs, rew, done, infos = a_env.step_wait()
        d_obs, d_rew, d_done, _ = b_env.step_device(torch.as_tensor(acts[k]).cuda())
        assert np.array_equal(obs, d_obs.cpu().numpy()) and np.array_equal(rew, d_rew.cpu().numpy())
        assert np.array_equal(done, d_done.cpu().numpy().astype(bool)) and len(infos) == n
        outs.append((obs, obs.copy(), rew, rew.copy()))
    assert np.array_equal(outs[1][0], outs[1][1])                 # step 1's array survived step 2
    assert outs[0][0] is not outs[1][0] and np.shares_memory(outs[0][0], outs[2][0])   # two buffers alternate
    assert np.array_equal(outs[0][2], outs[0][3]) and not np.shares_memory(outs[0][2], outs[2][2])   # rewards are never recycled
    # step_wait() again, no step_async(): one more step with the stored actions
    obs, rew, done, _ = a_env.step_wait()
    d_obs, d_rew, _, _ = b_env.step_device(torch.as_tensor(acts[2]).cuda())
    assert np.array_equal(obs, d_obs.cpu().numpy()) and np.array_equal(rew, d_rew.cpu().numpy())
    with pytest.raises(ValueError):
        a_env.step(np.zeros((n, 3), dtype=np.float32))
    a_env.close(); b_env.close()
