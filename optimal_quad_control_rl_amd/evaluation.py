"""On-device policy evaluation: lap times and crash rate of a trained policy (`qr_evaluate_policy`, csrc/quadrace_eval.hip).

What a user of the reference does right after training -- fly the policy deterministically and read gate-passage / lap times
(FP:261-289) and the crash rate (R:4487-4519) -- as one kernel launch per evaluation window: the closed loop, the gate-pass
detection and the lap accounting stay on the device, one 24-int record (+ one 4-float record) per env comes back.

    from optimal_quad_control_rl_amd import evaluate_policy
    r = evaluate_policy(model, eval_env, n_eval_steps=2000, window_steps=1200, seed=99)
    r["window"]["crashes_per_window"], r["total"]["first_lap_seconds"], r["total"]["flying_lap_seconds"]

All times inside the records are integer step counts; seconds appear only here (steps x env.dt).
"""
import math

import numpy as np

REC_INTS, MAX_LAPS, REC_FLOATS = 24, 8, 4   # QR_EVAL_REC_INTS, QR_EVAL_MAX_LAPS, QR_EVAL_REC_FLOATS of include/quadrace.h


def _host(a):
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def summarize_eval(rec, recf, dt, gates_per_lap):
    """Summary of evaluation records (`rec` [N, 24] int32, `recf` [N, 4] float32 or None; tensors or arrays) as a dict:
    gates / crashes / timeouts / episodes (totals over the envs), gates_per_env / crashes_per_env (per-env means), lap_seconds (mean
    duration of lap 1..8 since a (re)start, None where no lap was counted), laps_counted, first_lap_seconds, flying_lap_seconds
    (laps 2..8 pooled), mean_reward / std_reward of the finished episodes (None without episodes or without `recf`)."""
    rec = _host(rec).astype(np.int64)
    assert rec.ndim == 2 and rec.shape[1] == REC_INTS, rec.shape
    n, dt = rec.shape[0], float(dt)
    lap_sum, lap_cnt = rec[:, 6:6 + MAX_LAPS].sum(axis=0), rec[:, 14:14 + MAX_LAPS].sum(axis=0)
    lap_seconds = [float(s) * dt / int(c) if c > 0 else None for s, c in zip(lap_sum, lap_cnt)]
    fly_sum, fly_cnt = int(lap_sum[1:].sum()), int(lap_cnt[1:].sum())
    gates, crashes, timeouts = int(rec[:, 0].sum()), int(rec[:, 1].sum()), int(rec[:, 2].sum())
    episodes = crashes + timeouts
    mean_reward = std_reward = None
    recf = _host(recf)
    if recf is not None and episodes > 0:
        assert recf.shape == (n, REC_FLOATS), recf.shape
        s1, s2 = float(recf[:, 1].astype(np.float64).sum()), float(recf[:, 2].astype(np.float64).sum())
        mean_reward = s1 / episodes
        std_reward = math.sqrt(max(s2 / episodes - mean_reward * mean_reward, 0.0))
    return dict(envs=n, steps=int(rec[:, 5].max()) if n else 0, gates_per_lap=int(gates_per_lap),
                gates=gates, crashes=crashes, timeouts=timeouts, episodes=episodes,
                gates_per_env=gates / n if n else 0.0, crashes_per_env=crashes / n if n else 0.0,
                lap_seconds=lap_seconds, laps_counted=[int(c) for c in lap_cnt],
                first_lap_seconds=lap_seconds[0], flying_lap_seconds=fly_sum * dt / fly_cnt if fly_cnt > 0 else None,
                mean_reward=mean_reward, std_reward=std_reward)


def default_gates_per_lap(env):
    """The env's gate count, halved when the second half of the gate list repeats the first (square_track() lists its four gates
    twice so that `gates_ahead` can look across the lap boundary)."""
    g = int(env.num_gates)
    if g % 2 == 0 and g >= 2:
        h = g // 2
        if np.array_equal(env.gate_pos[:h], env.gate_pos[h:]) and np.array_equal(env.gate_yaw[:h], env.gate_yaw[h:]):
            return h
    return g


def _actor(model):
    """the torch actor (Linear, ReLU, ..., Linear) of the SB3-shaped PPO (sb3.PPO) or of the native trainer (ppo.PPO)"""
    net = getattr(model, "_net", None)
    if net is None:
        net = model.policy
    net = getattr(net, "net", net)   # sb3.ActorCriticPolicy wraps the ActorCritic
    return net.pi


def evaluate_policy(model, env, n_eval_steps=2000, window_steps=1200, gates_per_lap=None, precision=None, seed=None):
    """Deterministic evaluation of `model`'s current policy on `env` (a race env of this package, possibly inside a VecMonitor), as
    two kernel launches: `window_steps` (the "per 12 s" window of the crash / gate rates), then the rest of `n_eval_steps` (lap times
    need the longer flight).  Returns {"window": summary after the first call, "total": summary after both} (summarize_eval), the
    window with `crashes_per_window` / `gates_per_window` (per-env means).  `seed`: reseed and reset the env first, so that two
    evaluations see the same starts; None continues from the env's current state.  `precision`: "f16-operands" | "f32" (None: the
    model's own collect precision).  `env` keeps flying from where the evaluation left it."""
    import torch

    from .policy import MfmaPolicy
    from .sb3 import _unwrap

    core = _unwrap(env)
    if precision is None:
        f32 = getattr(model, "precision", None) in ("f32", "f32-collect") or getattr(model, "policy_forward", None) == "f32class"
        precision = "f32" if f32 else "f16-operands"
    n_eval_steps, window_steps = int(n_eval_steps), int(window_steps)
    if not 1 <= window_steps <= n_eval_steps:
        raise ValueError("need 1 <= window_steps <= n_eval_steps")
    gpl = default_gates_per_lap(core) if gates_per_lap is None else int(gates_per_lap)
    policy = MfmaPolicy(core.state_len, core.device.index).load_torch(_actor(model))
    try:
        if seed is not None:
            core.seed(seed)
            core.reset_device()
        rec = torch.zeros((core.num_envs, REC_INTS), dtype=torch.int32, device=core.device)
        recf = torch.zeros((core.num_envs, REC_FLOATS), dtype=torch.float32, device=core.device)
        core.evaluate_device(policy, window_steps, gpl, rec, recf, precision=precision)
        window = summarize_eval(rec, recf, core.dt, gpl)
        window["crashes_per_window"], window["gates_per_window"] = window["crashes_per_env"], window["gates_per_env"]
        if n_eval_steps > window_steps:
            core.evaluate_device(policy, n_eval_steps - window_steps, gpl, rec, recf, precision=precision)
        total = summarize_eval(rec, recf, core.dt, gpl)
    finally:
        torch.cuda.current_stream(core.device).synchronize()
        policy.close()
    return {"window": window, "total": total}
