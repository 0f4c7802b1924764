"""On-device policy evaluation: lap times and crash rate of a trained policy (`qr_evaluate_policy`, csrc/quadrace_eval.hip).

What a user of the reference does right after training -- fly the policy deterministically and read gate-passage / lap times
(FP:261-289) and the crash rate (R:4487-4519) -- as one kernel launch per evaluation window: the closed loop, the gate-pass
detection and the lap accounting stay on the device, one 24-int record (+ one 4-float record) per env comes back.

    from optimal_quad_control_rl_amd import evaluate_policy
    r = evaluate_policy(model, eval_env, n_eval_steps=2000, window_steps=1200, seed=99)
    r["window"]["crashes_per_window"], r["total"]["first_lap_seconds"], r["total"]["flying_lap_seconds"]

Many policies -- the checkpoints of a run, the seeds of a sweep -- are evaluated `env.num_envs // envs_per_policy` at a time in ONE launch
(`qr_evaluate_policy_bank`, csrc/quadrace_eval_bank.hip), every one of them on the same starts, disturbances and restarts:

    from optimal_quad_control_rl_amd import evaluate_policies, rank_policies
    results = evaluate_policies(["run/model_10.zip", "run/model_20.zip", model], eval_env, envs_per_policy=256, seed=0)
    best = rank_policies(results)[0]

A policy under conditions it did not train under -- other disturbance scales or ranges, another track, another time limit -- is a GRID
of policies x conditions, flown `env.num_envs // envs_per_cell` cells per launch on the same random numbers (`qr_evaluate_policy_grid`,
csrc/quadrace_eval_grid.hip):

    from optimal_quad_control_rl_amd import evaluate_grid, disturbance_sweep
    conds = disturbance_sweep(eval_env, [0, 0.5, 1, 2, 3])
    results = evaluate_grid([model], conds, eval_env, envs_per_cell=256, seed=0)      # results[p][c]
    rows = robustness_table(results, [c.name for c in conds])

The predecessor envs of "3D quad.ipynb" (quad3d.Quadcopter3DVec, Quadcopter3DVecGates) have outcomes of their own -- goal reached / track
finished, out of bounds, ground, gate collision, time limit -- counted by `q3_evaluate_policy` / `q3_evaluate_policy_bank` (csrc/quad3d.hip):

    from optimal_quad_control_rl_amd import evaluate_q3_policy, evaluate_q3_policies
    s = evaluate_q3_policy(model, eval_env, n_eval_steps=2000, seed=1)
    s["success_rate"], s["mean_success_seconds"], s["collisions"]
    curve = evaluate_q3_policies(checkpoints, eval_env, envs_per_policy=256, seed=1)   # one summary per checkpoint, same starts

All times inside the records are integer step counts; seconds appear only here (steps x env.dt).
"""
import math

import numpy as np

REC_INTS, MAX_LAPS, REC_FLOATS = 24, 8, 4   # QR_EVAL_REC_INTS, QR_EVAL_MAX_LAPS, QR_EVAL_REC_FLOATS of include/quadrace.h
Q3_REC_INTS, Q3_REC_FLOATS = 12, 4          # Q3_EVAL_REC_INTS, Q3_EVAL_REC_FLOATS of include/quad3d.h


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


def plan_policy_batches(num_policies, slots):
    """How evaluate_policies spreads `num_policies` policies over launches of `slots` policies each: a list of batches, each a list of
    exactly `slots` policy indices.  The last batch is padded by repeating its last policy (a launch always flies every group of the
    env); `kept` = how many leading slots of the batch are real.  Returns [(indices, kept), ...]; pure arithmetic, no device."""
    num_policies, slots = int(num_policies), int(slots)
    if num_policies < 1:
        raise ValueError("need at least one policy")
    if slots < 1:
        raise ValueError("the env holds no complete group: num_envs < envs_per_policy")
    plan = []
    for first in range(0, num_policies, slots):
        real = list(range(first, min(first + slots, num_policies)))
        plan.append((real + [real[-1]] * (slots - len(real)), len(real)))
    return plan


def _as_actor(entry):
    """(torch actor, model or None) of one entry of evaluate_policies: a checkpoint path written by `model.save`, an SB3-shaped PPO,
    a native trainer, or a bare torch actor (Linear, ReLU, ..., Linear)."""
    import os

    import torch

    if isinstance(entry, (str, os.PathLike)):
        from .sb3 import PPO

        entry = PPO.load(os.fspath(entry))   # needs no env
    if isinstance(entry, torch.nn.Module) and not hasattr(entry, "pi") and not hasattr(entry, "net"):
        return entry, None
    return _actor(entry), entry


def evaluate_policies(policies, env, envs_per_policy=256, n_eval_steps=2000, window_steps=1200, gates_per_lap=None, precision=None, seed=0):
    """evaluate_policy for a LIST of policies, `env.num_envs // envs_per_policy` of them per launch (qr_evaluate_policy_bank): policy p
    of a batch flies envs [p E, (p + 1) E) of `env`.  Every batch starts from `seed(seed); reset_device(); share_starts(E)` and the
    kernel keys restarts by the env's index within its group, so ALL policies -- within a batch and across batches -- see bit-identical
    starts, disturbances and restarts for as long as their own flying allows, the ones an E-env handle sees under
    evaluate_policy(..., seed=seed).  Entries: a checkpoint path written by `model.save` (loaded with PPO.load), an SB3-shaped PPO, a
    native trainer, or a torch actor.  envs_per_policy: a multiple of 256; env.num_envs must be a multiple of it.  precision: None =
    "f32" if any model collects in f32, else "f16-operands" (one launch has one precision).  Returns one {"window", "total"} dict per
    policy, in order, each what evaluate_policy returns for that policy on an E-env handle."""
    import torch

    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap

    core = _unwrap(env)
    E, n = int(envs_per_policy), core.num_envs
    if E < 256 or E % 256 != 0:
        raise ValueError("envs_per_policy must be a multiple of 256 (one workgroup serves one policy)")
    if n % E != 0:
        raise ValueError("env.num_envs must be a multiple of envs_per_policy")
    n_eval_steps, window_steps = int(n_eval_steps), int(window_steps)
    if not 1 <= window_steps <= n_eval_steps:
        raise ValueError("need 1 <= window_steps <= n_eval_steps")
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        f32 = any(getattr(m, "precision", None) in ("f32", "f32-collect") or getattr(m, "policy_forward", None) == "f32class" for _, m in actors)
        precision = "f32" if f32 else "f16-operands"
    gpl = default_gates_per_lap(core) if gates_per_lap is None else int(gates_per_lap)
    slots = n // E
    results = [None] * len(actors)
    bank = MfmaPolicyBank(core.state_len, slots, core.device.index)
    try:
        for indices, kept in plan_policy_batches(len(actors), slots):
            for slot, idx in enumerate(indices):
                bank.load_torch(slot, actors[idx][0])
            core.seed(seed)
            core.reset_device()
            core.share_starts(E)
            rec = torch.zeros((n, REC_INTS), dtype=torch.int32, device=core.device)
            recf = torch.zeros((n, REC_FLOATS), dtype=torch.float32, device=core.device)
            core.evaluate_bank_device(bank, slots, E, window_steps, gpl, rec, recf, precision=precision)
            windows = []
            for slot in range(kept):
                w = summarize_eval(rec[slot * E:(slot + 1) * E], recf[slot * E:(slot + 1) * E], core.dt, gpl)
                w["crashes_per_window"], w["gates_per_window"] = w["crashes_per_env"], w["gates_per_env"]
                windows.append(w)
            if n_eval_steps > window_steps:
                core.evaluate_bank_device(bank, slots, E, n_eval_steps - window_steps, gpl, rec, recf, precision=precision)
            for slot in range(kept):
                total = summarize_eval(rec[slot * E:(slot + 1) * E], recf[slot * E:(slot + 1) * E], core.dt, gpl)
                results[indices[slot]] = {"window": windows[slot], "total": total}
    finally:
        torch.cuda.current_stream(core.device).synchronize()
        bank.close()
    return results


def plan_grid_batches(num_policies, num_conditions, slots):
    """How evaluate_grid spreads the num_policies x num_conditions cells over launches of `slots` groups each: cells in row-major
    order (policy-major: cell k = (k // num_conditions, k % num_conditions)), each batch a list of exactly `slots` (policy,
    condition) pairs.  The last batch is padded by repeating its last cell (a launch always flies every group of the env); `kept` =
    how many leading groups of the batch are real.  Returns [(cells, kept), ...]; pure arithmetic, no device."""
    num_policies, num_conditions, slots = int(num_policies), int(num_conditions), int(slots)
    if num_policies < 1 or num_conditions < 1:
        raise ValueError("need at least one policy and one condition")
    if slots < 1:
        raise ValueError("the env holds no complete group: num_envs < envs_per_cell")
    total = num_policies * num_conditions
    plan = []
    for first in range(0, total, slots):
        real = [(k // num_conditions, k % num_conditions) for k in range(first, min(first + slots, total))]
        plan.append((real + [real[-1]] * (slots - len(real)), len(real)))
    return plan


def evaluate_grid(policies, conditions, env, envs_per_cell=256, n_eval_steps=2000, window_steps=1200, precision=None, seed=0):
    """evaluate_policy for every cell of `policies` x `conditions` (conditions.Condition), `env.num_envs // envs_per_cell` cells per
    launch (qr_evaluate_policy_grid): each group of E = envs_per_cell envs flies one policy under one condition -- the condition's
    track, start, disturbance ranges and scale, max_steps and gates_per_lap; `env`'s residual weights, dt and gates_ahead.  Every
    batch starts from `env.condition_starts(..., seed=seed)` and the kernel keys restarts by the env's index within its group, so
    all cells see the same uniform draws (only the condition's own scaling of them differs), and cell (p, c) is what an E-env
    handle configured with condition c sees under evaluate_policy(policies[p], ..., seed=seed).  Entries of `policies` and
    `precision`: as evaluate_policies.  Returns results[p][c], each a {"window", "total"} dict.  `env` keeps its own configuration."""
    import torch

    from .conditions import ConditionBank
    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap

    core = _unwrap(env)
    E, n = int(envs_per_cell), core.num_envs
    if E < 256 or E % 256 != 0:
        raise ValueError("envs_per_cell must be a multiple of 256 (one workgroup serves one cell)")
    if n % E != 0:
        raise ValueError("env.num_envs must be a multiple of envs_per_cell")
    n_eval_steps, window_steps = int(n_eval_steps), int(window_steps)
    if not 1 <= window_steps <= n_eval_steps:
        raise ValueError("need 1 <= window_steps <= n_eval_steps")
    conditions = list(conditions)
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        f32 = any(getattr(m, "precision", None) in ("f32", "f32-collect") or getattr(m, "policy_forward", None) == "f32class" for _, m in actors)
        precision = "f32" if f32 else "f16-operands"
    slots = n // E
    results = [[None] * len(conditions) for _ in actors]
    pbank = MfmaPolicyBank(core.state_len, len(actors), core.device.index)
    cbank = ConditionBank(core.VARIANT, len(conditions), core.device.index)
    try:
        for p, (actor, _) in enumerate(actors):
            pbank.load_torch(p, actor)
        for c, cond in enumerate(conditions):
            cbank.set(c, cond)
        for cells, kept in plan_grid_batches(len(actors), len(conditions), slots):
            pol, cog = [p for p, _ in cells], [c for _, c in cells]
            core.condition_starts(conditions, cog, E, seed=seed)
            rec = torch.zeros((n, REC_INTS), dtype=torch.int32, device=core.device)
            recf = torch.zeros((n, REC_FLOATS), dtype=torch.float32, device=core.device)
            core.evaluate_grid_device(pbank, cbank, pol, cog, E, window_steps, rec, recf, precision=precision)
            windows = []
            for g in range(kept):
                w = summarize_eval(rec[g * E:(g + 1) * E], recf[g * E:(g + 1) * E], core.dt, conditions[cog[g]].gates_per_lap)
                w["crashes_per_window"], w["gates_per_window"] = w["crashes_per_env"], w["gates_per_env"]
                windows.append(w)
            if n_eval_steps > window_steps:
                core.evaluate_grid_device(pbank, cbank, pol, cog, E, n_eval_steps - window_steps, rec, recf, precision=precision)
            for g in range(kept):
                total = summarize_eval(rec[g * E:(g + 1) * E], recf[g * E:(g + 1) * E], core.dt, conditions[cog[g]].gates_per_lap)
                results[pol[g]][cog[g]] = {"window": windows[g], "total": total}
    finally:
        torch.cuda.current_stream(core.device).synchronize()
        pbank.close()
        cbank.close()
    return results


def robustness_table(results, names):
    """evaluate_grid's results[p][c] as one table per policy: a list (per policy) of rows (condition name, crashes per window,
    flying-lap seconds or None, gates per window), in the order of `names` (one name per condition)."""
    names = list(names)
    tables = []
    for per_policy in results:
        if len(per_policy) != len(names):
            raise ValueError("one name per condition is needed")
        tables.append([(name, float(r["window"]["crashes_per_window"]), r["total"]["flying_lap_seconds"], float(r["window"]["gates_per_window"]))
                       for name, r in zip(names, per_policy)])
    return tables


def rank_policies(results, max_crashes_per_window=0.1):
    """Indices of `results` (evaluate_policies / evaluate_policy dicts), best first.  First the policies that crash at most
    `max_crashes_per_window` times per env and window AND have a flying lap, by flying-lap time (ties: fewer crashes, then the
    index); then everything else -- no flying lap, or over the crash bound -- by crash rate (ties: the index).  0.1 crashes per 12 s
    window is the band the project states for a policy worth keeping."""
    def crashes(r):
        return float(r["window"]["crashes_per_window"])

    def fly(r):
        return r["total"]["flying_lap_seconds"]

    good = [i for i, r in enumerate(results) if fly(r) is not None and crashes(r) <= max_crashes_per_window]
    rest = [i for i in range(len(results)) if i not in set(good)]
    good.sort(key=lambda i: (fly(results[i]), crashes(results[i]), i))
    rest.sort(key=lambda i: (crashes(results[i]), i))
    return good + rest


# ---- the predecessor envs (quad3d.py): how episodes end, and how long the successful ones take ------------------------------------
def summarize_q3_eval(rec, recf, dt):
    """Summary of q3 evaluation records (`rec` [N, 12] int32, `recf` [N, 4] float32 or None; tensors or arrays; layout: include/quad3d.h)
    as a dict: envs, steps (per env), episodes (ended ones), successes / timeouts / out_of_bounds / ground / collisions (totals over the
    envs; the causes are exclusive and add up to `episodes`), success_rate (None without episodes), mean_success_seconds /
    best_success_seconds (None without a success), mean_episode_seconds and gates_per_episode = (passes + successes) / episodes (None
    without episodes; a success is the pass of the final gate), mean_reward / std_reward of the finished episodes (None without
    episodes or without `recf`)."""
    rec = _host(rec).astype(np.int64)
    assert rec.ndim == 2 and rec.shape[1] == Q3_REC_INTS, rec.shape
    n, dt = rec.shape[0], float(dt)
    tot = rec.sum(axis=0)
    successes, timeouts, oob, ground, collisions = (int(tot[c]) for c in (1, 2, 3, 4, 5))
    episodes = successes + timeouts + oob + ground + collisions
    best = rec[:, 9][rec[:, 9] > 0]
    mean_reward = std_reward = None
    recf = _host(recf)
    if recf is not None and episodes > 0:
        assert recf.shape == (n, Q3_REC_FLOATS), recf.shape
        s1, s2 = float(recf[:, 1].astype(np.float64).sum()), float(recf[:, 2].astype(np.float64).sum())
        mean_reward = s1 / episodes
        std_reward = math.sqrt(max(s2 / episodes - mean_reward * mean_reward, 0.0))
    return dict(envs=n, steps=int(rec[:, 0].max()) if n else 0, episodes=episodes,
                successes=successes, timeouts=timeouts, out_of_bounds=oob, ground=ground, collisions=collisions,
                success_rate=successes / episodes if episodes else None,
                mean_success_seconds=int(tot[6]) * dt / successes if successes else None,
                best_success_seconds=int(best.min()) * dt if best.size else None,
                mean_episode_seconds=int(tot[7]) * dt / episodes if episodes else None,
                gates_per_episode=(int(tot[8]) + successes) / episodes if episodes else None,
                mean_reward=mean_reward, std_reward=std_reward)


def _model_precision(models):
    f32 = any(getattr(m, "precision", None) in ("f32", "f32-collect") or getattr(m, "policy_forward", None) == "f32class" for m in models)
    return "f32" if f32 else "f16-operands"


def evaluate_q3_policy(model, env, n_eval_steps=2000, precision=None, seed=None):
    """Deterministic evaluation of `model`'s current policy on `env` (a Quadcopter3DVec / Quadcopter3DVecGates, possibly inside a
    VecMonitor) as ONE kernel launch of `n_eval_steps` steps (q3_evaluate_policy).  Returns summarize_q3_eval's dict.  `model`: what
    evaluate_q3_policies accepts as an entry.  `seed`: reseed and reset the env first, so that two evaluations see the same starts; None
    continues from the env's current state.  `precision`: "f16-operands" | "f32" (None: the model's own collect precision).  `env`
    keeps flying from where the evaluation left it."""
    import torch

    from .policy import MfmaPolicy
    from .sb3 import _unwrap

    core = _unwrap(env)
    n_eval_steps = int(n_eval_steps)
    if n_eval_steps < 1:
        raise ValueError("need n_eval_steps >= 1")
    actor, owner = _as_actor(model)
    if precision is None:
        precision = _model_precision([owner])
    policy = MfmaPolicy(core.state_len, core.device.index).load_torch(actor)
    try:
        if seed is not None:
            core.seed(seed)
            core.reset_device()
        rec = torch.zeros((core.num_envs, Q3_REC_INTS), dtype=torch.int32, device=core.device)
        recf = torch.zeros((core.num_envs, Q3_REC_FLOATS), dtype=torch.float32, device=core.device)
        core.evaluate_device(policy, n_eval_steps, rec, recf, precision=precision)
        return summarize_q3_eval(rec, recf, core.dt)
    finally:
        torch.cuda.current_stream(core.device).synchronize()
        policy.close()


def evaluate_q3_policies(policies, env, envs_per_policy=256, n_eval_steps=2000, precision=None, seed=0):
    """evaluate_q3_policy for a LIST of policies, `env.num_envs // envs_per_policy` of them per launch (q3_evaluate_policy_bank): policy
    p of a batch flies envs [p E, (p + 1) E) of `env`.  Every batch starts from `seed(seed); reset_device(); share_starts(E)` and the
    kernel keys restarts by the env's index within its group, so ALL policies -- within a batch and across batches -- see bit-identical
    starts and restarts for as long as their own flying allows, the ones an E-env handle sees under evaluate_q3_policy(..., seed=seed).
    Entries: a checkpoint path written by `model.save`, an SB3-shaped PPO, a native trainer, or a torch actor.  envs_per_policy: a
    multiple of 256; env.num_envs must be a multiple of it.  precision: None = "f32" if any model collects in f32, else "f16-operands".
    The last batch is padded by repeating its last policy.  Returns one summarize_q3_eval dict per policy, in order."""
    from .sb3 import _unwrap

    core = _unwrap(env)
    E, n = int(envs_per_policy), int(core.num_envs)
    if E < 256 or E % 256 != 0:
        raise ValueError("envs_per_policy must be a multiple of 256 (one workgroup serves one policy)")
    if n % E != 0:
        raise ValueError("env.num_envs must be a multiple of envs_per_policy")
    n_eval_steps = int(n_eval_steps)
    if n_eval_steps < 1:
        raise ValueError("need n_eval_steps >= 1")
    policies = list(policies)
    slots = n // E
    plan = plan_policy_batches(len(policies), slots)

    import torch

    from .policy import MfmaPolicyBank

    actors = [_as_actor(p) for p in policies]
    if precision is None:
        precision = _model_precision([m for _, m in actors])
    results = [None] * len(actors)
    bank = MfmaPolicyBank(core.state_len, slots, core.device.index)
    try:
        for indices, kept in plan:
            for slot, idx in enumerate(indices):
                bank.load_torch(slot, actors[idx][0])
            core.seed(seed)
            core.reset_device()
            core.share_starts(E)
            rec = torch.zeros((n, Q3_REC_INTS), dtype=torch.int32, device=core.device)
            recf = torch.zeros((n, Q3_REC_FLOATS), dtype=torch.float32, device=core.device)
            core.evaluate_bank_device(bank, slots, E, n_eval_steps, rec, recf, precision=precision)
            for slot in range(kept):
                results[indices[slot]] = summarize_q3_eval(rec[slot * E:(slot + 1) * E], recf[slot * E:(slot + 1) * E], core.dt)
    finally:
        torch.cuda.current_stream(core.device).synchronize()
        bank.close()
    return results
