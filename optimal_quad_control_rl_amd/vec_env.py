"""Host-side mirror of the reference's `Quadcopter3DGates` VecEnv (R:287-620, I:142-410) on top of libquadrace.

Same constructor, methods and public attributes as the reference class, so the reference's training cell
(SB3 `VecMonitor` + `PPO`, R:765-795), `animate_policy` (R:800-810) and the C-controller test (R:4487-4519)
can consume it unchanged -- but every step is one fused HIP kernel over all envs on the MI355X, and a
device-tensor fast path (`step_device`, `rollout_device`) avoids any host round trip.

There is no NumPy fallback: constructing an env without a gfx950 GPU raises.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._closed_loop import _f32p, _precision_flags, check_records, log_std_array, log_std_rows, noise_seed_array, rollout_outputs
from ._lib import QR_VARIANT_E2E, QR_VARIANT_INDI

try:  # the reference imports `gymnasium.spaces` (R:284) / `gym.spaces` (I:139); neither is required here
    from gymnasium import spaces as _spaces  # type: ignore
except Exception:  # pragma: no cover - depends on the environment
    try:
        from gym import spaces as _spaces  # type: ignore
    except Exception:
        _spaces = None

try:
    from stable_baselines3.common.vec_env import VecEnv as _SB3VecEnv  # type: ignore
except Exception:  # pragma: no cover
    _SB3VecEnv = None


class Box:
    """Minimal stand-in for gymnasium.spaces.Box when gymnasium is not installed."""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.shape = tuple(shape) if shape is not None else tuple(np.shape(low))
        self.low = np.broadcast_to(np.asarray(low, dtype=dtype), self.shape).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=dtype), self.shape).copy()
        self.dtype = np.dtype(dtype)

    def sample(self):
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return np.random.uniform(lo, hi).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))


def _make_box(low, high, shape=None):
    if _spaces is not None:
        if shape is not None:
            return _spaces.Box(low=low, high=high, shape=shape, dtype=np.float32)
        return _spaces.Box(low=np.asarray(low, np.float32), high=np.asarray(high, np.float32), dtype=np.float32)
    return Box(low, high, shape)


class _VecEnvBase:
    """What SB3's abstract VecEnv provides to the reference class: the constructor contract and step()."""

    def __init__(self, num_envs, observation_space, action_space):
        self.num_envs = num_envs
        self.observation_space = observation_space
        self.action_space = action_space
        self.render_mode = None

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()


_Base = _SB3VecEnv if _SB3VecEnv is not None else _VecEnvBase

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def default_residual_blob():
    """The reference's trained residual thrust/moment MLP weights (NNDroneModel/*.pt, R:227-229) as 740 f32."""
    return np.fromfile(os.path.join(_DATA, "residual_mlp_f32.bin"), dtype=np.float32)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _DeviceBackedArray(np.ndarray):
    """Host copy of a device-resident env attribute that writes itself back when it is modified in place.

    In the reference `world_states`, `disturbances`, `target_gates` and `step_counts` are plain NumPy arrays owned by
    the env, and callers edit them in place (`env.world_states[i] = ...`, `env.target_gates[:] = 0`, `R:4499-4500`).
    Here the state lives in HBM, so the attribute is a snapshot; item / slice assignment and the in-place operators
    on the snapshot -- or on any view derived from it -- push the whole (small, evaluation-time) array back to the
    device, which keeps that idiom working instead of silently editing a temporary."""

    def __new__(cls, arr, writeback):
        obj = np.asarray(arr).view(cls)
        obj._root, obj._writeback = obj, writeback
        return obj

    def __array_finalize__(self, src):
        if src is None:
            return
        root = getattr(src, "_root", None)
        same_memory = root is not None and np.shares_memory(self, root) if root is not None else False
        self._root = root if same_memory else None          # copies / results of arithmetic are ordinary arrays
        self._writeback = getattr(src, "_writeback", None) if same_memory else None

    def _push(self):
        if getattr(self, "_writeback", None) is not None and self._root is not None:
            self._writeback(np.asarray(self._root))

    def __setitem__(self, key, value):
        super().__setitem__(key, value)
        self._push()

    def _inplace(name):
        def op(self, other):
            r = getattr(np.ndarray, name)(self, other)
            self._push()
            return r
        op.__name__ = name
        return op

    for _n in ("__iadd__", "__isub__", "__imul__", "__itruediv__", "__ifloordiv__", "__imod__", "__iand__", "__ior__"):
        locals()[_n] = _inplace(_n)
    del _n, _inplace

    def fill(self, value):
        super().fill(value)
        self._push()


class Quadcopter3DGates(_Base):
    """End-to-end (motor command) Bebop race environment, vectorised on one MI355X.  Mirrors R:287-620.

    Extra keyword-only arguments (not in the reference): `device` (cuda ordinal), `seed`, `residual`
    ('default' = the reference's NNDroneModel weights, None = no residual model, or a 740-float blob),
    `env_id_base` (global index of env 0 when sharding over GPUs), `infos_mode` ('reference' reproduces the
    shared-dict behaviour of R:589-594, 'per_env' gives one dict per done env, 'sb3' gives one dict per done env whose
    `terminal_observation` is the TRUE final observation of the episode -- what SB3's time-limit bootstrap expects --
    and `TimeLimit.truncated` only for the envs that hit the time limit, 'none' skips the list).
    """

    VARIANT = QR_VARIANT_E2E
    STATE_LEN = 16
    _RENDER_KEYS = ['x', 'y', 'z', 'vx', 'vy', 'vz', 'phi', 'theta', 'psi', 'p', 'q', 'r', 'w1', 'w2', 'w3', 'w4']

    def __init__(self, num_envs, gates_pos, gate_yaw, start_pos, gates_ahead=0, pause_if_collision=False, *,
                 device=None, seed=0, residual="default", env_id_base=0, infos_mode="reference"):
        self._h = None
        self._L = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("Quadcopter3DGates needs a gfx950 GPU: libquadrace has no CPU fallback")
        self._dev_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self._dev_index)

        # Define the race track (R:298-302)
        self.start_pos = np.asarray(start_pos).astype(np.float32)
        self.gate_pos = np.asarray(gates_pos).astype(np.float32)
        self.gate_yaw = np.asarray(gate_yaw).astype(np.float32)
        self.num_gates = int(self.gate_pos.shape[0])
        self.gates_ahead = int(gates_ahead)
        self._pause_if_collision = bool(pause_if_collision)
        self.infos_mode = infos_mode

        cfg = _lib.QrConfig(self.VARIANT, int(num_envs), self.gates_ahead, self._dev_index,
                            int(self._pause_if_collision), 0, int(env_id_base))
        h = C.c_void_p()
        _lib.check(self._L.qr_create(C.byref(cfg), C.byref(h)))
        self._h = h
        gp = np.ascontiguousarray(self.gate_pos)
        gy = np.ascontiguousarray(self.gate_yaw)
        sp = np.ascontiguousarray(self.start_pos)
        _lib.check(self._L.qr_set_track(self._h, _f32p(gp), _f32p(gy), self.num_gates, _f32p(sp)))
        # relative gates as computed by the library (R:307-319)
        self.gate_pos_rel = np.zeros((self.num_gates, 3), dtype=np.float32)
        self.gate_yaw_rel = np.zeros(self.num_gates, dtype=np.float32)
        _lib.check(self._L.qr_get_track_tables(self._h, _f32p(self.gate_pos_rel), _f32p(self.gate_yaw_rel)))

        self.state_len = int(self._L.qr_obs_len(self._h))  # R:330 / I:185
        action_space = _make_box(-1, 1, shape=(4,))
        observation_space = _make_box(np.array([-np.inf] * self.state_len), np.array([np.inf] * self.state_len))
        _Base.__init__(self, int(num_envs), observation_space, action_space)

        n, dev = self.num_envs, self.device
        self._obs = torch.zeros((n, self.state_len), dtype=torch.float32, device=dev)
        self._last_obs = self._obs      # where the current observation lives: the env's own buffer, or row K-1 of the caller's
                                        # rollout buffer after a K-step call (a view: no copy kernel behind every rollout)
        self._rew = torch.zeros(n, dtype=torch.float32, device=dev)
        self._done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._trunc = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._act = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        self.actions = np.zeros((n, 4), dtype=np.float32)
        self.dones = np.zeros(n, dtype=bool)
        self.final_gate_passed = np.zeros(n, dtype=bool)

        self._max_steps = 1200          # R:345
        self._dt = np.float32(0.01)     # R:346
        self._pause = False             # R:360
        self._disturbance_ranges = np.zeros((6, 2), dtype=np.float32)  # R:355
        self._disturbance_scale = 1     # R:358
        if self.VARIANT == QR_VARIANT_E2E:
            if isinstance(residual, str):
                if residual != "default":
                    raise ValueError("residual must be 'default', None or a 740-float array")
                residual = default_residual_blob()
            self.set_residual(residual)
        self.seed(seed)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.qr_destroy(self._h)
            self._h = None

    def set_residual(self, blob):
        if blob is None:
            _lib.check(self._L.qr_set_residual(self._h, None, 0))
        else:
            b = np.ascontiguousarray(blob, dtype=np.float32)
            _lib.check(self._L.qr_set_residual(self._h, _f32p(b), b.size))

    def _to_dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device)

    # ------------------------------------------------------------------ reference attributes
    @property
    def max_steps(self):
        return self._max_steps

    @max_steps.setter
    def max_steps(self, v):  # `test_env.max_steps = 10000` (I:648)
        self._max_steps = int(v)
        _lib.check(self._L.qr_set_limits(self._h, self._max_steps, float(self._dt)))

    @property
    def dt(self):
        return self._dt

    @dt.setter
    def dt(self, v):
        self._dt = np.float32(v)
        _lib.check(self._L.qr_set_limits(self._h, self._max_steps, float(self._dt)))

    @property
    def pause(self):
        return self._pause

    @pause.setter
    def pause(self, v):
        self._pause = bool(v)
        _lib.check(self._L.qr_set_pause(self._h, int(self._pause)))

    @property
    def pause_if_collision(self):
        return self._pause_if_collision

    @pause_if_collision.setter
    def pause_if_collision(self, v):  # R:293 is a plain attribute read by step_wait (R:573): assignable at any time
        self._pause_if_collision = bool(v)
        if getattr(self, "_h", None) is not None:
            _lib.check(self._L.qr_set_pause_if_collision(self._h, int(self._pause_if_collision)))

    @property
    def disturbance_ranges(self):
        return self._disturbance_ranges

    @disturbance_ranges.setter
    def disturbance_ranges(self, v):  # `env.venv.disturbance_ranges = ...` (R:780-781)
        self._disturbance_ranges = np.array(v)
        self._push_disturbance()

    @property
    def disturbance_scale(self):
        return self._disturbance_scale

    @disturbance_scale.setter
    def disturbance_scale(self, v):
        self._disturbance_scale = v
        self._push_disturbance()

    def _push_disturbance(self):
        if self.VARIANT != QR_VARIANT_E2E:
            return
        r = np.ascontiguousarray(self._disturbance_ranges, dtype=np.float32).reshape(6, 2)
        _lib.check(self._L.qr_set_disturbance(self._h, _f32p(r), float(self._disturbance_scale)))

    def get_state_tensors(self):
        """(world[N,S], disturbances[N,6] or None, target[N] i32, steps[N] i32, episode[N] u32->i64) on device."""
        n, dev = self.num_envs, self.device
        world = torch.empty((n, self.STATE_LEN), dtype=torch.float32, device=dev)
        dist = torch.empty((n, 6), dtype=torch.float32, device=dev) if self.VARIANT == QR_VARIANT_E2E else None
        target = torch.empty(n, dtype=torch.int32, device=dev)
        steps = torch.empty(n, dtype=torch.int32, device=dev)
        episode = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(self._L.qr_get_state(self._h, _ptr(world), _ptr(dist), _ptr(target), _ptr(steps), _ptr(episode),
                                        self._stream()))
        return world, dist, target, steps, episode

    def set_state_tensors(self, world=None, dist=None, target=None, steps=None, episode=None):
        w = None if world is None else self._to_dev(world, torch.float32)
        d = None if dist is None or self.VARIANT != QR_VARIANT_E2E else self._to_dev(dist, torch.float32)
        t = None if target is None else self._to_dev(target, torch.int32)
        s = None if steps is None else self._to_dev(steps, torch.int32)
        ep = None if episode is None else self._to_dev(episode, torch.int32)
        if w is not None:
            assert tuple(w.shape) == (self.num_envs, self.STATE_LEN), w.shape
        _lib.check(self._L.qr_set_state(self._h, _ptr(w), _ptr(d), _ptr(t), _ptr(s), _ptr(ep), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # staging tensors may be freed after return

    @property
    def world_states(self):
        return _DeviceBackedArray(self.get_state_tensors()[0].cpu().numpy(), lambda a: self.set_state_tensors(world=a))

    @world_states.setter
    def world_states(self, v):
        self.set_state_tensors(world=v)

    @property
    def disturbances(self):
        d = self.get_state_tensors()[1]
        return None if d is None else _DeviceBackedArray(d.cpu().numpy(), lambda a: self.set_state_tensors(dist=a))

    @disturbances.setter
    def disturbances(self, v):
        self.set_state_tensors(dist=v)

    @property
    def target_gates(self):
        return _DeviceBackedArray(self.get_state_tensors()[2].cpu().numpy().astype(np.int64),
                                  lambda a: self.set_state_tensors(target=np.asarray(a, dtype=np.int32)))

    @target_gates.setter
    def target_gates(self, v):
        self.set_state_tensors(target=np.asarray(v, dtype=np.int32))

    @property
    def step_counts(self):
        return _DeviceBackedArray(self.get_state_tensors()[3].cpu().numpy().astype(np.int64),
                                  lambda a: self.set_state_tensors(steps=np.asarray(a, dtype=np.int32)))

    @step_counts.setter
    def step_counts(self, v):
        self.set_state_tensors(steps=np.asarray(v, dtype=np.int32))

    @property
    def states(self):
        """Observation array [N, state_len] of the last reset()/step() (R:343, read by animate_policy R:803)."""
        return self._current_obs().cpu().numpy()

    @property
    def states_tensor(self):
        """The current observation on the device: always the env's OWN buffer.  A K-step call (rollout_device /
        step_sequence_device) leaves its last observation in row K-1 of the caller's rollout buffer and does not copy it (that copy
        was a 6 MB kernel behind every rollout); the FIRST read here takes the copy, so readers get a stable buffer that later
        reuse of the rollout buffer cannot change.  Read it before overwriting that buffer yourself."""
        return self._current_obs()

    def _current_obs(self):
        if self._last_obs is not self._obs:     # first read after a K-step call: row K-1 of the caller's buffer -> own buffer
            self._obs.copy_(self._last_obs)
            self._last_obs = self._obs
        return self._obs

    # ------------------------------------------------------------------ reference methods
    def update_states(self):
        """update_states_gate (R:365-450)."""
        _lib.check(self._L.qr_observe(self._h, _ptr(self._obs), self._stream()))
        self._last_obs = self._obs

    update_states_gate = update_states

    def update_states_world(self):
        """Alternative observation of the reference (R:362-363, unused by default): the raw world state."""
        return self.world_states

    def reset_(self, dones):
        mask = self._to_dev(np.asarray(dones, dtype=np.uint8), torch.uint8)
        _lib.check(self._L.qr_reset(self._h, _ptr(mask), _ptr(self._obs), self._stream()))
        self._last_obs = self._obs
        return self.states

    def reset(self):
        self.reset_device()
        return self.states

    def step_async(self, actions):
        """Stores the actions (R:498-499) and, unlike the reference, already enqueues the work on the device: the H->D copy of the
        actions, the step kernel and the D->H copies of its results run while the caller does whatever it does before
        step_wait(), which only synchronises."""
        self.actions = actions
        self._pending = self._enqueue_host_step()

    def _ensure_host(self):
        """Pinned host staging: TWO sets of result buffers used alternately (the arrays handed out by one step stay intact
        during the next one) and one action buffer."""
        if getattr(self, "_host", None) is None:
            n = self.num_envs

            def one_set():
                return (torch.empty((n, self.state_len), dtype=torch.float32).pin_memory(),
                        torch.empty(n, dtype=torch.float32).pin_memory(),
                        torch.empty(n, dtype=torch.uint8).pin_memory(),
                        torch.empty(n, dtype=torch.uint8).pin_memory())

            self._host = (one_set(), one_set())
            self._host_act = torch.empty((n, 4), dtype=torch.float32).pin_memory()
            self._host_flip = 0

    def _host_buffers(self):
        """the result buffer set of THIS step (alternates)"""
        self._ensure_host()
        self._host_flip ^= 1
        return self._host[self._host_flip]

    def _actions_to_device(self, actions):
        """H->D copy of the SB3-side action array through a pinned buffer into the env's own device tensor (a pageable
        source makes the runtime stage the copy itself, synchronously: 60 us instead of 29 us for the 1 MB at N = 65 536)."""
        if isinstance(actions, torch.Tensor):
            if actions.is_cuda:
                return self._to_dev(actions, torch.float32)
            actions = actions.detach().numpy()
        a = np.asarray(actions, dtype=np.float32)
        if a.shape != (self.num_envs, 4):
            raise ValueError(f"actions must have shape ({self.num_envs}, 4), got {a.shape}")
        self._ensure_host()
        self._host_act.numpy()[...] = a
        self._act.copy_(self._host_act, non_blocking=True)
        return self._act

    def _enqueue_host_step(self):
        act = self._actions_to_device(self.actions)
        if self.infos_mode == "sb3" and getattr(self, "_term_obs_buf", None) is None:
            self.set_terminal_obs_buffer(torch.zeros((self.num_envs, self.state_len), dtype=torch.float32, device=self.device))
        dev = self.step_device(act)
        host = self._host_buffers()
        for h, d in zip(host, dev):
            h.copy_(d, non_blocking=True)
        return host

    def step_wait(self):
        """SB3-facing step: NumPy in, NumPy out (one H->D copy of the actions through a pinned buffer, one batch of async
        D->H copies into pinned buffers, one synchronisation).  Like the reference, which returns its own `self.states`
        (R:595), the observation array is the env's buffer, not a copy: here one of two alternating pinned buffers, so it is
        overwritten by the step AFTER the next one.  Rewards and dones are fresh arrays.  Use step_device() to stay on the GPU."""
        host = getattr(self, "_pending", None)
        if host is None:   # step_wait() without a step_async() before it: the reference steps again with self.actions
            host = self._enqueue_host_step()
        self._pending = None
        torch.cuda.current_stream(self.device).synchronize()
        obs_np, rew_np = host[0].numpy(), host[1].numpy().copy()
        done_np, trunc_np = host[2].numpy().astype(bool), host[3].numpy().view(np.bool_)   # kernels write 0 / 1
        self.dones = done_np
        infos = self._make_infos(obs_np, done_np, trunc_np)
        return obs_np, rew_np, done_np, infos

    def _make_infos(self, obs_np, done_np, trunc_np):
        if self.infos_mode == "none":
            return []
        if self.infos_mode == "reference":
            # R:589-594: `[{}] * N` aliases ONE dict, so every env sees terminal_observation (the post-reset row
            # of the last done env) as soon as any env is done, and TimeLimit.truncated if any env timed out.
            shared = {}
            if done_np.any():
                shared["terminal_observation"] = obs_np[np.nonzero(done_np)[0][-1]]
            if trunc_np.any():
                shared["TimeLimit.truncated"] = True
            return [shared] * self.num_envs
        infos = [{} for _ in range(self.num_envs)]
        if self.infos_mode == "sb3":
            if done_np.any():
                idx = np.nonzero(done_np)[0]
                if self._pause_if_collision:   # no auto-reset in this mode (R:573-578): the row handed back IS the final observation
                    term = obs_np[idx]
                else:
                    tb = self._term_obs_buf if self._term_obs_buf.dim() == 2 else self._term_obs_buf[0]   # qr_step writes row [0][env]
                    term = tb[torch.as_tensor(idx, device=self.device)].cpu().numpy()   # rows written by the step kernel
                for j, i in enumerate(idx):
                    infos[i]["terminal_observation"] = term[j]
                    infos[i]["TimeLimit.truncated"] = bool(trunc_np[i])
            return infos
        if done_np.any():
            for i in np.nonzero(done_np)[0]:
                infos[i]["terminal_observation"] = obs_np[i]
                if trunc_np[i]:
                    infos[i]["TimeLimit.truncated"] = True
        return infos

    def seed(self, seed=None):
        """Upstream seed() is a no-op (R:600-601); here it keys the in-kernel Philox reset stream."""
        self._seed = int(0 if seed is None else seed)   # condition_starts reseeds with it
        _lib.check(self._L.qr_seed(self._h, self._seed))
        return [seed] * self.num_envs

    def get_attr(self, attr_name, indices=None):
        raise AttributeError()  # R:603-604: makes SB3 >= 2.0 fall back to render_mode=None

    def set_attr(self, attr_name, value, indices=None):
        pass

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        pass

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * self.num_envs

    def render(self, mode='human'):
        """Dict of per-env arrays consumed by quadcopter_animation (R:615-620)."""
        state_dict = dict(zip(self._RENDER_KEYS, self.world_states.T))
        a = self.actions.detach().cpu().numpy() if isinstance(self.actions, torch.Tensor) else np.array(self.actions)
        action_dict = dict(zip(['u1', 'u2', 'u3', 'u4'], (a.T + 1) / 2))
        return {**state_dict, **action_dict}

    # ------------------------------------------------------------------ device fast path (no host sync)
    def set_terminal_obs_buffer(self, buf, obs_len=None):
        """Register (or, with None, remove) a float32 CUDA tensor that receives the TRUE terminal observation -- the
        gate-frame observation of an episode's final state, taken before the auto-reset -- of every env that finishes
        at a step: shape [N, L] for step_device, [K, N, L] for rollout_device / step_sequence_device /
        rollout_policy_device (row [k, env]).  Rows of envs that did not finish are left untouched.  This is what SB3
        bootstraps time-limit truncations from; the reference itself fills `terminal_observation` after reset_()
        (R:589-594), i.e. with the first observation of the NEXT episode.
        obs_len (default: the env's own): the row length of `buf` -- obs_len + 4 H for rollout_policy_history_device with
        command_history = H, which writes [terminal observation | last H commands] rows and refuses a buffer of any other width."""
        rows = 0
        if buf is not None:
            width = self.state_len if obs_len is None else int(obs_len)
            assert buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.shape[-1] == width
            assert buf.dim() in (2, 3) and buf.shape[-2] == self.num_envs
            rows = int(buf.shape[0]) if buf.dim() == 3 else 1   # K-step calls with K > rows are refused by the library
        self._term_obs_buf = buf   # keep it alive while the library holds the pointer
        _lib.check(self._L.qr_set_terminal_obs(self._h, _ptr(buf), rows))

    def probe_residual(self):
        """[N, 7] device tensor (vb[3], residual thrust, residual moment[3]) of the current states (E2E + residual only)."""
        out = torch.empty((self.num_envs, 7), dtype=torch.float32, device=self.device)
        _lib.check(self._L.qr_probe_residual(self._h, _ptr(out), self._stream()))
        return out

    def reset_device(self):
        _lib.check(self._L.qr_reset(self._h, None, _ptr(self._obs), self._stream()))
        self._last_obs = self._obs
        return self._obs

    def step_device(self, actions):
        """actions: float32 CUDA tensor [N,4].  Returns (obs, reward, done u8, trunc u8) device tensors; they are
        the env's own buffers and are overwritten by the next step (clone them to keep a copy)."""
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        assert tuple(actions.shape) == (self.num_envs, 4)
        obs, rew, done, trunc = self._obs, self._rew, self._done, self._trunc
        _lib.check(self._L.qr_step(self._h, _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done), _ptr(trunc),
                                   self._stream()))
        if not self._pause:   # with pause set the kernel leaves the observation untouched (R:570-572)
            self._last_obs = obs
        return obs, rew, done, trunc

    ROLLOUT_FORMS = {"auto": 0, "multi_wave": 1, "general": 2, "general_multi_wave": 3, "one_wave": 4}

    def set_rollout_form(self, form):
        """Which family of fused kernels `rollout_device` may use: "auto" (by env count and mode), "multi_wave" (the forms built for more
        than one workgroup per CU, at any env count), "general" (the general kernels for every launch), "general_multi_wave" (both), "one_wave" (the one-wave forms at any env count).  All bit-identical: a test / A-B hook."""
        _lib.check(self._L.qr_set_rollout_form(self._h, self.ROLLOUT_FORMS[form]))
        return self

    def rollout_kernel_name(self):
        """Symbol of the device kernel rollout_device() launches on this env right now, as rocprofv3 prints it."""
        name = self._L.qr_rollout_kernel_name(self._h).decode()
        return "qr::%s<%d, %d>" % (name, int(self.VARIANT), self.gates_ahead)

    def rollout_device(self, actions, out=None):
        """K steps with pre-recorded actions [K,N,4] -> (obs[K,N,L], reward[K,N], done[K,N], trunc[K,N])."""
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        K = actions.shape[0]
        assert tuple(actions.shape) == (K, self.num_envs, 4)
        n, dev = self.num_envs, self.device
        if out is None:
            out = (torch.empty((K, n, self.state_len), dtype=torch.float32, device=dev),
                   torch.empty((K, n), dtype=torch.float32, device=dev),
                   torch.empty((K, n), dtype=torch.uint8, device=dev),
                   torch.empty((K, n), dtype=torch.uint8, device=dev))
        obs, rew, done, trunc = out
        _lib.check(self._L.qr_step_many(self._h, int(K), _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done), _ptr(trunc),
                                        self._stream()))
        if not self._pause:
            self._last_obs = obs[K - 1]
        return out

    def step_sequence_device(self, actions, out):
        """K per-step kernel launches (qr_step each) writing into rollout buffers `out` -- what a closed-loop
        caller does when the policy runs between steps.  Same results as rollout_device (fused kernel)."""
        K = actions.shape[0]
        obs, rew, done, trunc = out
        _lib.check(self._L.qr_step_launches(self._h, int(K), _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done),
                                            _ptr(trunc), self._stream()))
        if not self._pause:
            self._last_obs = obs[K - 1]
        return out

    def rollout_policy_device(self, policy, num_steps, log_std, noise_seed=0, first_step=0, deterministic=False, out=None,
                              precision="f16-operands"):
        """Closed-loop rollout in ONE kernel (qr_rollout_policy): K x [obs -> MFMA policy -> sample -> env.step].
        `policy` is an optimal_quad_control_rl_amd.policy.MfmaPolicy.  Returns device tensors
        (obs[K,N,L], actions[K,N,4] unclipped, logp[K,N], reward[K,N], done[K,N] u8, trunc[K,N] u8, last_obs[N,L]).
        precision="f32": the policy forward inside the kernel at the reference's precision (QR_ROLLOUT_F32CLASS)."""
        flags = _precision_flags(precision)
        K, n, dev = int(num_steps), self.num_envs, self.device
        if out is None:
            out = rollout_outputs(K, n, self.state_len, dev)
        obs, act, logp, rew, done, trunc = out
        ls = log_std_array(log_std)
        _lib.check(self._L.qr_rollout_policy(self._h, policy._h, K, _f32p(ls), int(noise_seed), int(first_step),
                                             int(bool(deterministic)) | flags, _ptr(obs), _ptr(act), _ptr(logp), _ptr(rew),
                                             _ptr(done), _ptr(trunc), _ptr(self._obs), self._stream()))
        self._last_obs = self._obs
        return obs, act, logp, rew, done, trunc, self._obs

    def _check_eval_records(self, rec, recf):
        """The evaluators' record tensors: `rec` int32 [N, 24], `recf` float32 [N, 4] or None, both on the device and contiguous."""
        check_records(rec, recf, self.num_envs, (24, 4), AssertionError)

    def evaluate_device(self, policy, num_steps, gates_per_lap, rec, recf=None, precision="f16-operands"):
        """Closed-loop deterministic evaluation in ONE kernel (qr_evaluate_policy): K x [obs -> MFMA policy -> env.step(clip(mean))]
        with the lap / crash accounting on the device and nothing stored per step.  `rec` int32 CUDA tensor [N, 24] and `recf`
        float32 [N, 4] (optional) are read at the start and written at the end: zero them for a fresh evaluation, pass them again
        to continue one (record layout: include/quadrace.h; summary: evaluation.summarize_eval).  Returns (rec, recf)."""
        flags = _precision_flags(precision)
        self._check_eval_records(rec, recf)
        _lib.check(self._L.qr_evaluate_policy(self._h, policy._h, int(num_steps), int(gates_per_lap), flags,
                                              _ptr(rec), _ptr(recf), self._stream()))
        self.update_states()   # the kernel stores no observation: refresh the env's own buffer from the state it left
        return rec, recf

    def evaluate_bank_device(self, bank, num_policies, envs_per_policy, num_steps, gates_per_lap, rec, recf=None, precision="f16-operands"):
        """A bank of policies in ONE kernel (qr_evaluate_policy_bank): slot p of `bank` (policy.MfmaPolicyBank), p < num_policies, flies
        envs [p E, (p + 1) E), E = envs_per_policy (a multiple of 256; num_policies * E == num_envs), with the evaluator's accounting.
        Records as in evaluate_device: rows [p E, (p + 1) E) of `rec` [N, 24] / `recf` [N, 4] belong to policy p.  Inside this call an env
        that ends its episode restarts from the reset stream of its index WITHIN its group, so groups that start equal (share_starts)
        see the same starts, disturbances and restarts; every other call on this env resets with the ordinary ids.  Returns (rec, recf)."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_evaluate_policy_bank")
        self._check_eval_records(rec, recf)
        _lib.check(fn(self._h, bank._h, int(num_policies), int(envs_per_policy), int(num_steps), int(gates_per_lap),
                      flags, _ptr(rec), _ptr(recf), self._stream()))
        self.update_states()   # the kernel stores no observation: refresh the env's own buffer from the state it left
        return rec, recf

    def share_starts(self, envs_per_policy):
        """Copy the full state (world, disturbances, target, steps, episode) of envs [0, E) onto every following group of E envs
        (E = envs_per_policy divides num_envs).  After `seed(s); reset_device(); share_starts(E)` every group is bit-equal to an E-env
        handle after `seed(s); reset_device()`: the common starts evaluate_bank_device's group-local reset stream continues from."""
        e, n = int(envs_per_policy), self.num_envs
        if e < 1 or n % e != 0:
            raise ValueError("envs_per_policy must divide num_envs")
        reps = n // e
        if reps > 1:
            world, dist, target, steps, episode = self.get_state_tensors()
            tile = lambda t: None if t is None else t[:e].repeat((reps,) + (1,) * (t.dim() - 1)).contiguous()
            self.set_state_tensors(tile(world), tile(dist), tile(target), tile(steps), tile(episode))
        self.update_states()
        return self

    def evaluate_grid_device(self, policy_bank, condition_bank, policy_of_group, condition_of_group, envs_per_group, num_steps, rec, recf=None,
                             precision="f16-operands"):
        """A grid of policies x flight conditions in ONE kernel (qr_evaluate_policy_grid): group g = envs [g E, (g + 1) E), E =
        envs_per_group (a multiple of 256; len(policy_of_group) * E == num_envs), flies slot policy_of_group[g] of `policy_bank`
        (policy.MfmaPolicyBank) under slot condition_of_group[g] of `condition_bank` (conditions.ConditionBank): track, start,
        disturbance ranges and scale, max_steps and gates_per_lap are the condition's; residual weights, dt and gates_ahead this
        env's.  Records as in evaluate_device, rows [g E, (g + 1) E) belong to group g; restarts use the group-local reset stream of
        evaluate_bank_device, so groups that start equal draw the same random numbers and every group flies what an E-env handle
        configured with its condition flies (condition_starts gives those starts).  Afterwards the env's observation buffer holds,
        for every group, the observation a handle under the group's condition has of the state the call left (one reconfigure +
        observe per distinct condition of the map, then the env's own configuration again).  Returns (rec, recf)."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_evaluate_policy_grid")
        pol = np.ascontiguousarray(policy_of_group, dtype=np.int32).reshape(-1)
        cond = np.ascontiguousarray(condition_of_group, dtype=np.int32).reshape(-1)
        if pol.shape != cond.shape:
            raise ValueError("policy_of_group and condition_of_group must have one entry per group each")
        self._check_eval_records(rec, recf)
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy_bank._h, condition_bank._h, int(pol.shape[0]), int(envs_per_group), pol.ctypes.data_as(i32p),
                      cond.ctypes.data_as(i32p), int(num_steps), flags, _ptr(rec), _ptr(recf), self._stream()))
        # the kernel stores no observation: refresh the env's own buffer from the state it left, every group as ITS condition observes it
        self._observe_under(condition_bank.conditions, cond, int(envs_per_group))
        return rec, recf

    def evaluate_dynamics_grid_device(self, policy_bank, condition_bank, dynamics_bank, policy_of_group, condition_of_group, dynamics_of_group,
                                      envs_per_group, num_steps, rec, recf=None, precision="f16-operands"):
        """evaluate_grid_device with a third axis, the VEHICLE (qr_evaluate_policy_dynamics_grid): group g additionally flies the
        coefficients of slot dynamics_of_group[g] of `dynamics_bank` (dynamics.DynamicsBank) in its equations of motion.  A group
        whose slot holds the nominal table flies bit for bit what evaluate_grid_device flies; the residual weights and the
        observation stay this env's.  Everything else -- groups, records, restarts, the observation buffer afterwards -- as
        evaluate_grid_device.  Returns (rec, recf)."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_evaluate_policy_dynamics_grid")
        pol = np.ascontiguousarray(policy_of_group, dtype=np.int32).reshape(-1)
        cond = np.ascontiguousarray(condition_of_group, dtype=np.int32).reshape(-1)
        dyn = np.ascontiguousarray(dynamics_of_group, dtype=np.int32).reshape(-1)
        if not (pol.shape == cond.shape == dyn.shape):
            raise ValueError("policy_of_group, condition_of_group and dynamics_of_group must have one entry per group each")
        self._check_eval_records(rec, recf)
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy_bank._h, condition_bank._h, dynamics_bank._h, int(pol.shape[0]), int(envs_per_group),
                      pol.ctypes.data_as(i32p), cond.ctypes.data_as(i32p), dyn.ctypes.data_as(i32p), int(num_steps), flags, _ptr(rec),
                      _ptr(recf), self._stream()))
        self._observe_under(condition_bank.conditions, cond, int(envs_per_group))
        return rec, recf

    def evaluate_sensing_grid_device(self, policy_bank, condition_bank, dynamics_bank, sensing_bank, policy_of_group, condition_of_group,
                                     dynamics_of_group, sensing_of_group, envs_per_group, num_steps, pending, rec, recf=None,
                                     precision="f16-operands", noise_seed=0, first_step=0):
        """evaluate_dynamics_grid_device with a fourth axis, the SENSOR (qr_evaluate_policy_sensing_grid): group g additionally flies
        through slot sensing_of_group[g] of `sensing_bank` (sensing.SensingBank) -- Gaussian noise on the observation the policy sees,
        keyed by (`noise_seed`, env_id_base + the env's index within its group, `first_step` + t), and a command delay of 0..4 steps
        whose queue lives in `pending`, float32 CUDA [N, 16]: zero it with every (re)start, pass it again -- with `first_step` advanced
        by the steps flown -- to continue.  A group with an ideal slot flies bit for bit what evaluate_dynamics_grid_device flies.
        Returns (rec, recf)."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_evaluate_policy_sensing_grid")
        maps = [np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in (policy_of_group, condition_of_group, dynamics_of_group, sensing_of_group)]
        if len({m.shape for m in maps}) != 1:
            raise ValueError("policy_of_group, condition_of_group, dynamics_of_group and sensing_of_group must have one entry per group each")
        self._check_eval_records(rec, recf)
        if not (pending.is_cuda and pending.dtype == torch.float32 and pending.is_contiguous() and tuple(pending.shape) == (self.num_envs, 16)):
            raise AssertionError("pending must be a contiguous float32 CUDA tensor [num_envs, 16]")
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy_bank._h, condition_bank._h, dynamics_bank._h, sensing_bank._h, int(maps[0].shape[0]), int(envs_per_group),
                      *[m.ctypes.data_as(i32p) for m in maps], int(num_steps), flags, int(noise_seed) & (2 ** 64 - 1), int(first_step), _ptr(pending),
                      _ptr(rec), _ptr(recf), self._stream()))
        self._observe_under(condition_bank.conditions, maps[1], int(envs_per_group))
        return rec, recf

    def sensing_noise_device(self, sensing_bank, slot, envs_per_group, num_steps, noise_seed=0, first_step=0, out=None):
        """What evaluate_sensing_grid_device adds to the observations of a group under slot `slot` (qr_sensing_noise): float32 CUDA
        [num_steps, envs_per_group, obs_len], row [t, e] = sigma[group(j)] * eps[j] of the group-local env e at step first_step + t, from
        the device function the evaluator calls.  An all-zero slot gives +0.0."""
        fn = _lib.require(self._L, "qr_sensing_noise")
        shape = (int(num_steps), int(envs_per_group), self.state_len)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
            raise AssertionError("out must be a contiguous float32 CUDA tensor [num_steps, envs_per_group, obs_len]")
        _lib.check(fn(self._h, sensing_bank._h, int(slot), shape[1], shape[0], int(noise_seed) & (2 ** 64 - 1), int(first_step), _ptr(out),
                      self._stream()))
        return out

    def _under_each_condition(self, conditions, condition_of_group, fn):
        """fn(c) with the HANDLE configured as conditions[c] (track, start, disturbances, max_steps), once per distinct entry of
        condition_of_group in ascending order; the handle's own configuration is restored afterwards, also when fn raises."""
        own = (self.gate_pos, self.gate_yaw, self.start_pos, np.array(self._disturbance_ranges), self._disturbance_scale, self._max_steps)
        try:
            for c in sorted(set(int(c) for c in condition_of_group)):
                cond = conditions[c]
                if cond is None:
                    raise ValueError("condition slot %d was never set" % c)
                if cond.disturbance_ranges is not None and self.VARIANT != QR_VARIANT_E2E:
                    raise ValueError("an INDI env has no disturbances: the condition's disturbance_ranges must be None")
                # ranges None on an E2E env = the state of a handle whose disturbances were never set: zero ranges, scale 1
                ranges = np.zeros((6, 2), dtype=np.float32) if cond.disturbance_ranges is None else cond.disturbance_ranges
                scale = 1 if cond.disturbance_ranges is None else cond.disturbance_scale
                self._configure(cond.gate_pos, cond.gate_yaw, cond.start_pos, ranges, scale, cond.max_steps)
                fn(c)
        finally:
            self._configure(*own)

    def _observe_under(self, conditions, condition_of_group, envs_per_group):
        """The env's own observation buffer <- the observation of the current state, rows of group g as a handle configured with
        conditions[condition_of_group[g]] observes them (gate rows and disturbance scaling are the condition's)."""
        e = int(envs_per_group)
        cog = [int(c) for c in condition_of_group]
        tmp = torch.empty_like(self._obs)

        def observe(c):
            _lib.check(self._L.qr_observe(self._h, _ptr(tmp), self._stream()))
            for g, cg in enumerate(cog):
                if cg == c:
                    self._obs[g * e:(g + 1) * e].copy_(tmp[g * e:(g + 1) * e])

        self._under_each_condition(conditions, cog, observe)
        torch.cuda.current_stream(self.device).synchronize()   # tmp is freed on return
        self._last_obs = self._obs

    def _configure(self, gate_pos, gate_yaw, start_pos, disturbance_ranges, disturbance_scale, max_steps):
        """Track, start, disturbances and max_steps of the HANDLE (qr_set_track, qr_set_disturbance, qr_set_limits) and the attributes
        that mirror them.  disturbance_ranges None leaves the disturbances alone."""
        self.gate_pos = np.array(gate_pos, dtype=np.float32).reshape(-1, 3)
        self.gate_yaw = np.array(gate_yaw, dtype=np.float32).reshape(-1)
        self.start_pos = np.array(start_pos, dtype=np.float32).reshape(3)
        self.num_gates = int(self.gate_pos.shape[0])
        _lib.check(self._L.qr_set_track(self._h, _f32p(self.gate_pos), _f32p(self.gate_yaw), self.num_gates, _f32p(self.start_pos)))
        self.gate_pos_rel = np.zeros((self.num_gates, 3), dtype=np.float32)
        self.gate_yaw_rel = np.zeros(self.num_gates, dtype=np.float32)
        _lib.check(self._L.qr_get_track_tables(self._h, _f32p(self.gate_pos_rel), _f32p(self.gate_yaw_rel)))
        if disturbance_ranges is not None and self.VARIANT == QR_VARIANT_E2E:
            self._disturbance_ranges = np.array(disturbance_ranges)
            self._disturbance_scale = disturbance_scale
            self._push_disturbance()
        self.max_steps = max_steps

    def _group_map(self, conditions, condition_of_group, envs_per_group, seed):
        """(E, condition_of_group as ints, seed to use) of condition_starts / condition_reset, the map checked against the env"""
        e = int(envs_per_group)
        cog = [int(c) for c in condition_of_group]
        if e < 1 or len(cog) * e != self.num_envs:
            raise ValueError("len(condition_of_group) * envs_per_group must equal num_envs")
        if any(c < 0 or c >= len(conditions) for c in cog):
            raise ValueError("condition_of_group holds an index outside `conditions`")
        return e, cog, self._seed if seed is None else int(seed)

    def condition_starts(self, conditions, condition_of_group, envs_per_group, seed=None):
        """Give every group g of E = envs_per_group envs the start an E-env handle configured with conditions[condition_of_group[g]]
        gets from `seed(s); reset_device()` (s = `seed`, default: the seed this env was last seeded with): per distinct condition the
        handle takes the condition's track, start, disturbances and max_steps, is seeded and reset, and rows [0, E) of its state are
        kept; then the env's own configuration is restored and the assembled state set.  Groups under the same condition start
        bit-equal; groups under conditions that differ in the disturbance scale only differ in `disturbances` only.  A few N-env
        resets; the episode counters and step counts are those of a fresh reset."""
        e, cog, s = self._group_map(conditions, condition_of_group, envs_per_group, seed)
        starts = {}

        def start(c):
            self.seed(s)
            self.reset_device()
            starts[c] = [None if t is None else t[:e].clone() for t in self.get_state_tensors()]

        self._under_each_condition(conditions, cog, start)
        parts = list(zip(*[starts[c] for c in cog]))
        self.set_state_tensors(*[None if p[0] is None else torch.cat(p).contiguous() for p in parts])
        self._observe_under(conditions, cog, e)
        return self

    def rollout_policy_conditions_device(self, policy, condition_bank, condition_of_group, envs_per_group, num_steps, log_std, noise_seed=0,
                                         first_step=0, deterministic=False, out=None, precision="f16-operands"):
        """rollout_policy_device across a MIX of flight conditions in ONE kernel (qr_rollout_policy_conditions): group g = envs
        [g E, (g + 1) E), E = envs_per_group (a multiple of 256; len(condition_of_group) * E == num_envs), flies under slot
        condition_of_group[g] of `condition_bank` (conditions.ConditionBank): track, start, disturbance ranges and scale and max_steps
        are the condition's (its gates_per_lap is not used); residual weights, dt and gates_ahead this env's.  Reset stream and action
        noise use the env's ORDINARY ids (unlike evaluate_grid_device): group g computes bit for bit what an E-env handle with
        env_id_base + g E, configured with its condition, computes under rollout_policy_device (condition_reset gives the starts).
        The E2E observation's disturbance terms are scaled by each condition's own ranges.  Same return tuple as
        rollout_policy_device; a registered terminal-observation buffer is honoured."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_rollout_policy_conditions")
        cond = np.ascontiguousarray(condition_of_group, dtype=np.int32).reshape(-1)
        K, n, dev = int(num_steps), self.num_envs, self.device
        if out is None:
            out = rollout_outputs(K, n, self.state_len, dev)
        obs, act, logp, rew, done, trunc = out
        ls = log_std_array(log_std)
        _lib.check(fn(self._h, policy._h, condition_bank._h, int(cond.shape[0]), int(envs_per_group), cond.ctypes.data_as(C.POINTER(C.c_int32)),
                      K, _f32p(ls), int(noise_seed), int(first_step), int(bool(deterministic)) | flags, _ptr(obs), _ptr(act), _ptr(logp),
                      _ptr(rew), _ptr(done), _ptr(trunc), _ptr(self._obs), self._stream()))
        self._last_obs = self._obs
        return obs, act, logp, rew, done, trunc, self._obs

    def rollout_policy_dynamics_device(self, policy, condition_bank, condition_of_group, dynamics_bank, dynamics_of_group, envs_per_group,
                                       num_steps, log_std, noise_seed=0, first_step=0, deterministic=False, out=None, precision="f16-operands"):
        """rollout_policy_conditions_device across a MIX of VEHICLES in ONE kernel (qr_rollout_policy_dynamics): group g additionally
        flies the coefficients of slot dynamics_of_group[g] of `dynamics_bank` (dynamics.DynamicsBank) in its equations of motion,
        loaded once per workgroup into scalar registers.  A group whose slot holds the nominal table computes bit for bit what
        rollout_policy_conditions_device computes; group g equals the one-group call on an E-env handle with env_id_base + g E under
        the group's condition and slot.  The residual weights and the observation stay this env's: the vehicle is not observed.
        Everything else -- groups, ordinary env ids, return tuple, terminal-observation buffer -- as rollout_policy_conditions_device."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_rollout_policy_dynamics")
        cond = np.ascontiguousarray(condition_of_group, dtype=np.int32).reshape(-1)
        dyn = np.ascontiguousarray(dynamics_of_group, dtype=np.int32).reshape(-1)
        if cond.shape != dyn.shape:
            raise ValueError("condition_of_group and dynamics_of_group must have one entry per group each")
        K, n, dev = int(num_steps), self.num_envs, self.device
        if out is None:
            out = rollout_outputs(K, n, self.state_len, dev)
        obs, act, logp, rew, done, trunc = out
        ls = log_std_array(log_std)
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy._h, condition_bank._h, dynamics_bank._h, int(cond.shape[0]), int(envs_per_group), cond.ctypes.data_as(i32p),
                      dyn.ctypes.data_as(i32p), K, _f32p(ls), int(noise_seed), int(first_step), int(bool(deterministic)) | flags, _ptr(obs),
                      _ptr(act), _ptr(logp), _ptr(rew), _ptr(done), _ptr(trunc), _ptr(self._obs), self._stream()))
        self._last_obs = self._obs
        return obs, act, logp, rew, done, trunc, self._obs

    def new_sensing_queue(self):
        """The command queues of rollout_policy_sensing_device / evaluate_sensing_grid_device for a freshly (re)started env: a zeroed
        float32 CUDA tensor [num_envs, 16]."""
        return torch.zeros((self.num_envs, 16), dtype=torch.float32, device=self.device)

    def rollout_policy_sensing_device(self, policy, condition_bank, condition_of_group, dynamics_bank, dynamics_of_group, sensing_bank,
                                      sensing_of_group, envs_per_group, num_steps, log_std, pending, noise_seed=0, first_step=0,
                                      deterministic=False, out=None, precision="f16-operands"):
        """rollout_policy_dynamics_device under OBSERVATION NOISE and COMMAND DELAY in ONE kernel (qr_rollout_policy_sensing): group g
        additionally flies through slot sensing_of_group[g] of `sensing_bank` (sensing.SensingBank), the sensor of
        evaluate_sensing_grid_device -- but keyed by the env's ORDINARY ids (`noise_seed`, env_id_base + i, `first_step` + k).  The
        returned obs rows and last_obs are the NOISY rows the policy saw; the terminal-observation rows stay clean; actions and
        log-probs are this step's sample, the reward is that of the step flown (with the command of d steps ago).  `pending`, float32
        CUDA [num_envs, 16] (new_sensing_queue), carries the command queues from call to call: zero it with every (re)start, pass it
        again with `first_step` advanced by the steps flown to continue.  A group with an ideal slot computes bit for bit what
        rollout_policy_dynamics_device computes.  Everything else -- groups, return tuple, terminal-observation buffer -- as
        rollout_policy_dynamics_device."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_rollout_policy_sensing")
        maps = [np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in (condition_of_group, dynamics_of_group, sensing_of_group)]
        if len({m.shape for m in maps}) != 1:
            raise ValueError("condition_of_group, dynamics_of_group and sensing_of_group must have one entry per group each")
        if not (pending.is_cuda and pending.dtype == torch.float32 and pending.is_contiguous() and tuple(pending.shape) == (self.num_envs, 16)):
            raise AssertionError("pending must be a contiguous float32 CUDA tensor [num_envs, 16]")
        K, n, dev = int(num_steps), self.num_envs, self.device
        if out is None:
            out = rollout_outputs(K, n, self.state_len, dev)
        obs, act, logp, rew, done, trunc = out
        ls = log_std_array(log_std)
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy._h, condition_bank._h, dynamics_bank._h, sensing_bank._h, int(maps[0].shape[0]), int(envs_per_group),
                      *[m.ctypes.data_as(i32p) for m in maps], K, _f32p(ls), int(noise_seed) & (2 ** 64 - 1), int(first_step),
                      int(bool(deterministic)) | flags, _ptr(pending), _ptr(obs), _ptr(act), _ptr(logp), _ptr(rew), _ptr(done), _ptr(trunc),
                      _ptr(self._obs), self._stream()))
        self._last_obs = self._obs
        return obs, act, logp, rew, done, trunc, self._obs

    def rollout_policy_history_device(self, policy, condition_bank, condition_of_group, dynamics_bank, dynamics_of_group, sensing_bank,
                                      sensing_of_group, command_history, envs_per_group, num_steps, log_std, pending, noise_seed=0, first_step=0,
                                      deterministic=False, out=None, precision="f16-operands"):
        """rollout_policy_sensing_device for a policy that OBSERVES ITS LAST COMMANDS (qr_rollout_policy_history): with
        H = command_history in 1 .. 4 - gates_ahead the policy's row at call-step k is [noisy observation | u_{k-1}, ..., u_{k-H}], the
        last H clipped commands COMPUTED (not flown) in the current episode, newest first, zeros before the episode's start and after
        the step that ends it; the history part carries no noise.  `policy` is an MfmaPolicy of obs_len + 4 H inputs -- the length of an
        env with gates_ahead + H gates ahead, which is why gates_ahead + H <= 4.  obs rows are [K, N, obs_len + 4 H], last_obs
        [N, obs_len + 4 H] (a buffer of this call's own; the env's observation buffer takes its first obs_len columns on the next read);
        a registered terminal-observation buffer must have rows of obs_len + 4 H floats (set_terminal_obs_buffer(buf, obs_len=...)) and
        receives [clean terminal observation | u_k, ..., u_{k-H+1}].  `pending` carries max(delay, H) commands per env and passes
        between this call, rollout_policy_sensing_device and the two evaluators.  Everything else as rollout_policy_sensing_device."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_rollout_policy_history")
        H = int(command_history)
        width = self.state_len + 4 * H
        maps = [np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in (condition_of_group, dynamics_of_group, sensing_of_group)]
        if len({m.shape for m in maps}) != 1:
            raise ValueError("condition_of_group, dynamics_of_group and sensing_of_group must have one entry per group each")
        if not (pending.is_cuda and pending.dtype == torch.float32 and pending.is_contiguous() and tuple(pending.shape) == (self.num_envs, 16)):
            raise AssertionError("pending must be a contiguous float32 CUDA tensor [num_envs, 16]")
        term = getattr(self, "_term_obs_buf", None)
        if term is not None and H >= 1 and int(term.shape[-1]) != width:   # the kernel would write rows of `width` floats into it
            raise ValueError("the registered terminal-observation buffer has rows of %d floats; command_history=%d writes rows of %d: "
                             "register it with set_terminal_obs_buffer(buf, obs_len=%d)" % (int(term.shape[-1]), H, width, width))
        K, n, dev = int(num_steps), self.num_envs, self.device
        if out is None:
            out = rollout_outputs(K, n, width, dev)
        obs, act, logp, rew, done, trunc = out
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.numel() >= K * n * max(width, self.state_len)):
            raise AssertionError("the obs rows must be a contiguous float32 CUDA tensor [num_steps, num_envs, obs_len + 4 * command_history]")
        last = getattr(self, "_obs_history", None)
        if last is None or int(last.shape[1]) != max(width, self.state_len):
            last = self._obs_history = torch.zeros((n, max(width, self.state_len)), dtype=torch.float32, device=dev)
        ls = log_std_array(log_std)
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy._h, condition_bank._h, dynamics_bank._h, sensing_bank._h, int(maps[0].shape[0]), int(envs_per_group),
                      *[m.ctypes.data_as(i32p) for m in maps], H, K, _f32p(ls), int(noise_seed) & (2 ** 64 - 1), int(first_step),
                      int(bool(deterministic)) | flags, _ptr(pending), _ptr(obs), _ptr(act), _ptr(logp), _ptr(rew), _ptr(done), _ptr(trunc),
                      _ptr(last), self._stream()))
        self._last_obs = last[:, :self.state_len]
        return obs, act, logp, rew, done, trunc, last

    def rollout_policy_privileged_device(self, policy, condition_bank, condition_of_group, dynamics_bank, dynamics_of_group, sensing_bank,
                                         sensing_of_group, command_history, envs_per_group, num_steps, log_std, pending, noise_seed=0,
                                         first_step=0, deterministic=False, out=None, precision="f16-operands"):
        """rollout_policy_history_device that ALSO stores the rows a PRIVILEGED CRITIC reads (qr_rollout_policy_privileged):
        critic_obs [K, N, obs_len + 4 H] holds, at call-step k, [the observation BEFORE the sensor's noise | the same history tail] -- the
        row obs[k] is the slot's noise added to -- and critic_last_obs [N, obs_len + 4 H] the clean row behind the last step, bit for bit
        row 0 of critic_obs of the next call with first_step advanced through the same `pending`.  command_history = H may be 0 (the
        form of rollout_policy_sensing_device) up to 4 - gates_ahead.  Every other output, `pending` and the env state are bit for bit
        those of the twin call (rollout_policy_sensing_device for H = 0, rollout_policy_history_device otherwise); terminal rows are
        clean already and unchanged.  out = (obs, critic_obs, act, logp, rew, done, trunc).
        Returns (obs, critic_obs, act, logp, rew, done, trunc, last_obs, critic_last_obs)."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_rollout_policy_privileged")
        H = int(command_history)
        width = self.state_len + 4 * H
        maps = [np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in (condition_of_group, dynamics_of_group, sensing_of_group)]
        if len({m.shape for m in maps}) != 1:
            raise ValueError("condition_of_group, dynamics_of_group and sensing_of_group must have one entry per group each")
        if not (pending.is_cuda and pending.dtype == torch.float32 and pending.is_contiguous() and tuple(pending.shape) == (self.num_envs, 16)):
            raise AssertionError("pending must be a contiguous float32 CUDA tensor [num_envs, 16]")
        term = getattr(self, "_term_obs_buf", None)
        if term is not None and H >= 1 and int(term.shape[-1]) != width:   # the kernel would write rows of `width` floats into it
            raise ValueError("the registered terminal-observation buffer has rows of %d floats; command_history=%d writes rows of %d: "
                             "register it with set_terminal_obs_buffer(buf, obs_len=%d)" % (int(term.shape[-1]), H, width, width))
        K, n, dev = int(num_steps), self.num_envs, self.device
        if out is None:
            obs, act, logp, rew, done, trunc = rollout_outputs(K, n, width, dev)
            out = (obs, torch.empty_like(obs), act, logp, rew, done, trunc)
        obs, critic_obs, act, logp, rew, done, trunc = out
        for rows in (obs, critic_obs):
            if not (rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() >= K * n * max(width, self.state_len)):
                raise AssertionError("the obs and critic_obs rows must be contiguous float32 CUDA tensors [num_steps, num_envs, obs_len + 4 * command_history]")
        last = getattr(self, "_obs_history", None)
        if last is None or int(last.shape[1]) != max(width, self.state_len):
            last = self._obs_history = torch.zeros((n, max(width, self.state_len)), dtype=torch.float32, device=dev)
        critic_last = getattr(self, "_obs_critic", None)
        if critic_last is None or int(critic_last.shape[1]) != int(last.shape[1]):
            critic_last = self._obs_critic = torch.zeros_like(last)
        ls = log_std_array(log_std)
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy._h, condition_bank._h, dynamics_bank._h, sensing_bank._h, int(maps[0].shape[0]), int(envs_per_group),
                      *[m.ctypes.data_as(i32p) for m in maps], H, K, _f32p(ls), int(noise_seed) & (2 ** 64 - 1), int(first_step),
                      int(bool(deterministic)) | flags, _ptr(pending), _ptr(obs), _ptr(critic_obs), _ptr(act), _ptr(logp), _ptr(rew), _ptr(done),
                      _ptr(trunc), _ptr(last), _ptr(critic_last), self._stream()))
        self._last_obs = last[:, :self.state_len]
        return obs, critic_obs, act, logp, rew, done, trunc, last, critic_last

    def evaluate_history_grid_device(self, policy_bank, condition_bank, dynamics_bank, sensing_bank, policy_of_group, condition_of_group,
                                     dynamics_of_group, sensing_of_group, command_history, envs_per_group, num_steps, pending, rec, recf=None,
                                     precision="f16-operands", noise_seed=0, first_step=0):
        """evaluate_sensing_grid_device for policies that OBSERVE THEIR LAST COMMANDS (qr_evaluate_policy_history_grid): `policy_bank`
        holds policies of obs_len + 4 * command_history inputs, fed [noisy observation | the last command_history clipped commands
        computed in the episode] as rollout_policy_history_device feeds them; `pending` carries max(delay, command_history) commands
        per env.  Everything else as evaluate_sensing_grid_device.  Returns (rec, recf)."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_evaluate_policy_history_grid")
        maps = [np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in (policy_of_group, condition_of_group, dynamics_of_group, sensing_of_group)]
        if len({m.shape for m in maps}) != 1:
            raise ValueError("policy_of_group, condition_of_group, dynamics_of_group and sensing_of_group must have one entry per group each")
        self._check_eval_records(rec, recf)
        if not (pending.is_cuda and pending.dtype == torch.float32 and pending.is_contiguous() and tuple(pending.shape) == (self.num_envs, 16)):
            raise AssertionError("pending must be a contiguous float32 CUDA tensor [num_envs, 16]")
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy_bank._h, condition_bank._h, dynamics_bank._h, sensing_bank._h, int(maps[0].shape[0]), int(envs_per_group),
                      *[m.ctypes.data_as(i32p) for m in maps], int(command_history), int(num_steps), flags, int(noise_seed) & (2 ** 64 - 1),
                      int(first_step), _ptr(pending), _ptr(rec), _ptr(recf), self._stream()))
        self._observe_under(condition_bank.conditions, maps[1], int(envs_per_group))
        return rec, recf

    def rollout_policy_population_device(self, bank, policy_of_group, condition_bank, condition_of_group, envs_per_group, num_steps, log_stds,
                                         noise_seeds, first_step=0, deterministic=False, out=None, precision="f16-operands"):
        """rollout_policy_conditions_device for a POPULATION of policies in ONE kernel (qr_rollout_policy_population): group g = envs
        [g E, (g + 1) E), E = envs_per_group (a multiple of 256; len(policy_of_group) * E == num_envs), flies slot policy_of_group[g]
        of `bank` (policy.MfmaPolicyBank) under slot condition_of_group[g] of `condition_bank` (conditions.ConditionBank), sampling
        with log_stds[g] ([G][4]) and the action-noise seed noise_seeds[g] ([G]); first_step, deterministic and precision hold for the
        whole launch.  Ordinary env ids: group g computes bit for bit what an E-env handle with env_id_base + g E, configured with its
        condition, computes under rollout_policy_device with that slot's weights in an MfmaPolicy, its log_std and its seed.  Same
        return tuple as rollout_policy_device; a registered terminal-observation buffer is honoured."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_rollout_policy_population")
        pol = np.ascontiguousarray(policy_of_group, dtype=np.int32).reshape(-1)
        cond = np.ascontiguousarray(condition_of_group, dtype=np.int32).reshape(-1)
        if pol.shape != cond.shape:
            raise ValueError("policy_of_group and condition_of_group must have one entry per group each")
        groups = int(pol.shape[0])
        ls, seeds = log_std_rows(log_stds, groups), noise_seed_array(noise_seeds, groups)
        K, n, dev = int(num_steps), self.num_envs, self.device
        if out is None:
            out = rollout_outputs(K, n, self.state_len, dev)
        obs, act, logp, rew, done, trunc = out
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, bank._h, condition_bank._h, groups, int(envs_per_group), pol.ctypes.data_as(i32p), cond.ctypes.data_as(i32p),
                      K, _f32p(ls), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(first_step), int(bool(deterministic)) | flags, _ptr(obs),
                      _ptr(act), _ptr(logp), _ptr(rew), _ptr(done), _ptr(trunc), _ptr(self._obs), self._stream()))
        self._last_obs = self._obs
        return obs, act, logp, rew, done, trunc, self._obs

    def condition_reset(self, conditions, condition_of_group, envs_per_group, seed=None):
        """The training counterpart of condition_starts: reset every group g of E = envs_per_group envs under
        conditions[condition_of_group[g]] with the env's ORDINARY ids.  Per distinct condition the handle takes the condition's track,
        start, disturbances and max_steps, is seeded (s = `seed`, default: the seed this env was last seeded with) and reset over all N
        envs, and the rows of the groups flying that condition are kept; then the env's own configuration is restored and the assembled
        state set.  Group g then starts where an E-env handle with env_id_base + g E, configured with its condition, starts after
        `seed(s); reset_device()` -- the twin of rollout_policy_conditions_device's contract.  Returns the observation tensor, rows of
        group g as its condition observes them."""
        e, cog, s = self._group_map(conditions, condition_of_group, envs_per_group, seed)
        state = None

        def reset(c):
            nonlocal state
            self.seed(s)
            self.reset_device()
            fresh = self.get_state_tensors()
            if state is None:
                state = [None if t is None else torch.empty_like(t) for t in fresh]
            for g, cg in enumerate(cog):
                if cg == c:
                    for dst, src in zip(state, fresh):
                        if dst is not None:
                            dst[g * e:(g + 1) * e].copy_(src[g * e:(g + 1) * e])

        self._under_each_condition(conditions, cog, reset)
        self.set_state_tensors(*state)
        self._observe_under(conditions, cog, e)
        return self._obs

    RECORD_EXTRA = 8  # QR_RECORD_EXTRA of include/quadrace.h

    def record_policy_device(self, policy, num_steps, log_std, noise_seed=0, first_step=0, deterministic=True, rec_envs=None, out=None,
                             precision="f16-operands"):
        """The flight recorder (qr_record_policy): the closed loop of rollout_policy_device in ONE kernel whose only per-step output is
        one packed row per env.  Returns the float32 device tensor [K, M, R], M = rec_envs (None: every env; all envs fly either way),
        R = STATE_LEN + 8: columns [0, S) the world state BEFORE the step (what get_state_tensors would give), [S, S + 4) the command
        the env received (clip(action, -1, 1)), then reward, end code (0 running / 1 crash / 2 time limit), target gate before the
        step, step count before the step (time = steps * dt).  recording.FlightRecord gives the columns names.  `out`: a tensor of
        that shape to write into.  Same noise stream and env state afterwards as rollout_policy_device with the same arguments."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_record_policy")
        K, n, dev = int(num_steps), self.num_envs, self.device
        m = n if rec_envs is None else int(rec_envs)
        r = self.STATE_LEN + self.RECORD_EXTRA
        if out is None:
            out = torch.empty((max(K, 0), min(max(m, 0), n), r), dtype=torch.float32, device=dev)
        else:
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (K, m, r), (out.dtype, out.shape)
        ls = log_std_array(log_std)
        _lib.check(fn(self._h, policy._h, K, _f32p(ls), int(noise_seed), int(first_step),
                      int(bool(deterministic)) | flags, m, _ptr(out), self._stream()))
        self.update_states()   # the kernel stores no observation: refresh the env's own buffer from the state it left
        return out

    BLACKBOX_ST_INTS = 4  # QR_BLACKBOX_ST_INTS of include/quadrace.h

    def blackbox_policy_device(self, policy, num_steps, log_std, window=64, trigger=1, noise_seed=0, first_step=0, deterministic=True,
                               rec_envs=None, ring=None, status=None, terminal=None, precision="f16-operands"):
        """The black box (qr_blackbox_policy): the closed loop of record_policy_device in ONE kernel that keeps, per env, only the last
        `window` recorder rows in a ring and stops overwriting them when the env's episode ends the way `trigger` selects (bit 1 crash,
        bit 2 time limit; 0 never freezes).  Returns device tensors (ring [W, M, R] float32, status [M, 4] int32, terminal [M, S]
        float32), M = rec_envs (None: every env; all envs fly either way): the row of call-step k sits in slot (first_step + k) % W;
        status = (frozen, rows stored so far, slot of the trigger row or -1, cause bits); terminal = the world state at the end of a
        frozen env's trigger step (blackbox.CrashLog unrolls all three).  Pass the returned tensors back as `ring`, `status`,
        `terminal` with first_step advanced by num_steps and the same window to continue; fresh ones are NaN / zero filled.  Same noise
        stream and env state afterwards as record_policy_device / rollout_policy_device with the same arguments."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_blackbox_policy")
        K, n, dev, w = int(num_steps), self.num_envs, self.device, int(window)
        m = n if rec_envs is None else int(rec_envs)
        mm, r = min(max(m, 0), n), self.STATE_LEN + self.RECORD_EXTRA
        if ring is None:
            ring = torch.full((max(w, 1), max(mm, 1), r), float("nan"), dtype=torch.float32, device=dev)   # (never empty: the library names a bad argument)
        else:
            assert ring.is_cuda and ring.dtype == torch.float32 and ring.is_contiguous() and tuple(ring.shape) == (w, m, r), (ring.dtype, ring.shape)
        if status is None:
            status = torch.zeros((max(mm, 1), self.BLACKBOX_ST_INTS), dtype=torch.int32, device=dev)
        else:
            assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and tuple(status.shape) == (m, self.BLACKBOX_ST_INTS), \
                (status.dtype, status.shape)
        if terminal is None:
            terminal = torch.full((max(mm, 1), self.STATE_LEN), float("nan"), dtype=torch.float32, device=dev)
        else:
            assert terminal.is_cuda and terminal.dtype == torch.float32 and terminal.is_contiguous() and \
                tuple(terminal.shape) == (m, self.STATE_LEN), (terminal.dtype, terminal.shape)
        ls = log_std_array(log_std)
        _lib.check(fn(self._h, policy._h, K, _f32p(ls), int(noise_seed), int(first_step), int(bool(deterministic)) | flags,
                      int(trigger), w, m, _ptr(ring), _ptr(status), _ptr(terminal), self._stream()))
        self.update_states()   # the kernel stores no observation: refresh the env's own buffer from the state it left
        return ring, status, terminal

    def blackbox_grid_device(self, policy_bank, condition_bank, dynamics_bank, sensing_bank, policy_of_group, condition_of_group,
                             dynamics_of_group, sensing_of_group, command_history, envs_per_group, num_steps, pending, rec, recf=None,
                             precision="f16-operands", noise_seed=0, first_step=0, window=64, trigger=1, rec_per_group=None, ring=None,
                             status=None, terminal=None):
        """The black box of the sensing-grid evaluator (qr_blackbox_policy_grid): the launch of evaluate_history_grid_device
        (command_history = 0: of evaluate_sensing_grid_device) -- rec, recf, pending and the env state afterwards are bit for bit that
        call's -- which also keeps, for the first M = rec_per_group envs of every group (None: all of them), the last `window` recorder
        rows in a ring frozen the way `trigger` selects, as blackbox_policy_device does.  Env g E + j, j < M, owns column g M + j of
        ring [W, G M, R], status [G M, 4] and terminal [G M, S]; the row of call-step k sits in slot (first_step + k) % W and holds the
        TRUE world state before the step and the command FLOWN (under a delay, the one computed that many steps earlier).  window =
        num_steps with trigger 0 is the flight recorder of every cell.  Pass the returned tensors back, with first_step advanced by
        num_steps and the same pending / rec / recf, to continue; fresh ones are NaN / zero filled.
        Returns (rec, recf, ring, status, terminal)."""
        flags = _precision_flags(precision)
        fn = _lib.require(self._L, "qr_blackbox_policy_grid")
        maps = [np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in (policy_of_group, condition_of_group, dynamics_of_group, sensing_of_group)]
        if len({m.shape for m in maps}) != 1:
            raise ValueError("policy_of_group, condition_of_group, dynamics_of_group and sensing_of_group must have one entry per group each")
        self._check_eval_records(rec, recf)
        if not (pending.is_cuda and pending.dtype == torch.float32 and pending.is_contiguous() and tuple(pending.shape) == (self.num_envs, 16)):
            raise AssertionError("pending must be a contiguous float32 CUDA tensor [num_envs, 16]")
        g, e, w, dev = int(maps[0].shape[0]), int(envs_per_group), int(window), self.device
        m = e if rec_per_group is None else int(rec_per_group)
        cols, r = max(g, 1) * min(max(m, 1), max(e, 1)), self.STATE_LEN + self.RECORD_EXTRA   # (never empty: the library names a bad argument)
        if ring is None:
            ring = torch.full((max(w, 1), cols, r), float("nan"), dtype=torch.float32, device=dev)
        else:
            assert ring.is_cuda and ring.dtype == torch.float32 and ring.is_contiguous() and tuple(ring.shape) == (w, g * m, r), (ring.dtype, ring.shape)
        if status is None:
            status = torch.zeros((cols, self.BLACKBOX_ST_INTS), dtype=torch.int32, device=dev)
        else:
            assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and \
                tuple(status.shape) == (g * m, self.BLACKBOX_ST_INTS), (status.dtype, status.shape)
        if terminal is None:
            terminal = torch.full((cols, self.STATE_LEN), float("nan"), dtype=torch.float32, device=dev)
        else:
            assert terminal.is_cuda and terminal.dtype == torch.float32 and terminal.is_contiguous() and \
                tuple(terminal.shape) == (g * m, self.STATE_LEN), (terminal.dtype, terminal.shape)
        i32p = C.POINTER(C.c_int32)
        _lib.check(fn(self._h, policy_bank._h, condition_bank._h, dynamics_bank._h, sensing_bank._h, g, e,
                      *[mp.ctypes.data_as(i32p) for mp in maps], int(command_history), int(num_steps), flags, int(noise_seed) & (2 ** 64 - 1),
                      int(first_step), _ptr(pending), _ptr(rec), _ptr(recf), int(trigger), w, m, _ptr(ring), _ptr(status), _ptr(terminal),
                      self._stream()))
        self._observe_under(condition_bank.conditions, maps[1], e)
        return rec, recf, ring, status, terminal

    def profile_rollout(self, actions, out):
        """Like rollout_device but every step kernel is bracketed by its own hipEvent pair on the launch stream.
        Returns (mean single-kernel duration in ms, whole-region ms).  Blocks."""
        K = actions.shape[0]
        obs, rew, done, trunc = out
        mean_ms, region_ms = C.c_float(), C.c_float()
        _lib.check(self._L.qr_profile_steps(self._h, int(K), _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done),
                                            _ptr(trunc), self._stream(), C.byref(mean_ms), C.byref(region_ms)))
        return float(mean_ms.value), float(region_ms.value)

    def set_timing(self, on):
        """hipEvent bracket around every K-step call (read back by last_rollout_ms()); off = two marker packets fewer per call"""
        _lib.check(self._L.qr_set_timing(self._h, int(bool(on))))

    def last_rollout_ms(self):
        ms = C.c_float()
        _lib.check(self._L.qr_last_step_many_ms(self._h, C.byref(ms)))
        return float(ms.value)


class Quadcopter3DGatesINDI(Quadcopter3DGates):
    """INDI inner-loop variant: actions are (p_cmd, q_cmd, r_cmd, T_cmd), 13-state model.  Mirrors I:142-410."""

    VARIANT = QR_VARIANT_INDI
    STATE_LEN = 13
    _RENDER_KEYS = ['x', 'y', 'z', 'vx', 'vy', 'vz', 'phi', 'theta', 'psi', 'p', 'q', 'r', 'T']

    def __init__(self, num_envs, gates_pos, gate_yaw, start_pos, gates_ahead=0, pause_if_collision=False, **kw):
        kw.pop("residual", None)
        super().__init__(num_envs, gates_pos, gate_yaw, start_pos, gates_ahead, pause_if_collision, residual=None, **kw)

    def get_attr(self, attr_name, indices=None):
        return None  # I:393-394
