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
import copy
import math

import numpy as np

from ._closed_loop import _actor, _as_actor, _host, _model_precision, fly_batches, flying_policy, group_size, zero_records  # noqa: F401 (_actor: tools/)

REC_INTS, MAX_LAPS, REC_FLOATS = 24, 8, 4   # QR_EVAL_REC_INTS, QR_EVAL_MAX_LAPS, QR_EVAL_REC_FLOATS of include/quadrace.h
Q3_REC_INTS, Q3_REC_FLOATS = 12, 4          # Q3_EVAL_REC_INTS, Q3_EVAL_REC_FLOATS of include/quad3d.h


def _reward_stats(recf, n, episodes):
    """(mean, std) of the finished episodes' rewards from `recf` [n, 4] (either kind of record: columns 1, 2 = sum, sum of squares);
    (None, None) without episodes or without `recf`"""
    recf = _host(recf)
    if recf is None or episodes <= 0:
        return None, None
    assert recf.shape == (n, REC_FLOATS) and REC_FLOATS == Q3_REC_FLOATS, recf.shape
    s1, s2 = float(recf[:, 1].astype(np.float64).sum()), float(recf[:, 2].astype(np.float64).sum())
    mean = s1 / episodes
    return mean, math.sqrt(max(s2 / episodes - mean * mean, 0.0))


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
    mean_reward, std_reward = _reward_stats(recf, n, episodes)
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


def _phases(n_eval_steps, window_steps):
    """[window, rest] of an evaluation, the rest dropped when it is 0"""
    n_eval_steps, window_steps = int(n_eval_steps), int(window_steps)
    if not 1 <= window_steps <= n_eval_steps:
        raise ValueError("need 1 <= window_steps <= n_eval_steps")
    return [window_steps, n_eval_steps - window_steps][:2 if n_eval_steps > window_steps else 1]


def _window_total(summaries):
    """{"window", "total"} of the per-phase summaries of one policy: the first with the per-window names of its rates, the last"""
    window = copy.deepcopy(summaries[0])
    window["crashes_per_window"], window["gates_per_window"] = window["crashes_per_env"], window["gates_per_env"]
    return {"window": window, "total": summaries[-1]}


def evaluate_policy(model, env, n_eval_steps=2000, window_steps=1200, gates_per_lap=None, precision=None, seed=None):
    """Deterministic evaluation of `model`'s current policy on `env` (a race env of this package, possibly inside a VecMonitor), as
    two kernel launches: `window_steps` (the "per 12 s" window of the crash / gate rates), then the rest of `n_eval_steps` (lap times
    need the longer flight).  Returns {"window": summary after the first call, "total": summary after both} (summarize_eval), the
    window with `crashes_per_window` / `gates_per_window` (per-env means).  `model`: what evaluate_policies accepts as an entry.
    `seed`: reseed and reset the env first, so that two evaluations see the same starts; None continues from the env's current state.
    `precision`: "f16-operands" | "f32" (None: the model's own collect precision).  `env` keeps flying from where the evaluation left
    it."""
    phases = _phases(n_eval_steps, window_steps)
    with flying_policy(model, env, precision, seed) as (core, policy, precision, _):
        gpl = default_gates_per_lap(core) if gates_per_lap is None else int(gates_per_lap)
        rec, recf = zero_records(core.num_envs, (REC_INTS, REC_FLOATS), core.device)
        summaries = []
        for steps in phases:
            core.evaluate_device(policy, steps, gpl, rec, recf, precision=precision)
            summaries.append(summarize_eval(rec, recf, core.dt, gpl))
    return _window_total(summaries)


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


def _shared_starts(core, bank, actors, E, seed):
    """the per-batch step of the two bank evaluators: the batch's policies into the bank's slots, then the same starts for every group"""
    def start(indices):
        for slot, idx in enumerate(indices):
            bank.load_torch(slot, actors[idx][0])
        core.seed(seed)
        core.reset_device()
        core.share_starts(E)
    return start


def _sync_and_close(core, *banks):
    import torch

    torch.cuda.current_stream(core.device).synchronize()
    for bank in banks:
        bank.close()


def evaluate_policies(policies, env, envs_per_policy=256, n_eval_steps=2000, window_steps=1200, gates_per_lap=None, precision=None, seed=0):
    """evaluate_policy for a LIST of policies, `env.num_envs // envs_per_policy` of them per launch (qr_evaluate_policy_bank): policy p
    of a batch flies envs [p E, (p + 1) E) of `env`.  Every batch starts from `seed(seed); reset_device(); share_starts(E)` and the
    kernel keys restarts by the env's index within its group, so ALL policies -- within a batch and across batches -- see bit-identical
    starts, disturbances and restarts for as long as their own flying allows, the ones an E-env handle sees under
    evaluate_policy(..., seed=seed).  Entries: a checkpoint path written by `model.save` (loaded with PPO.load), an SB3-shaped PPO, a
    native trainer, or a torch actor.  envs_per_policy: a multiple of 256; env.num_envs must be a multiple of it.  precision: None =
    "f32" if any model collects in f32, else "f16-operands" (one launch has one precision).  Returns one {"window", "total"} dict per
    policy, in order, each what evaluate_policy returns for that policy on an E-env handle."""
    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap

    core = _unwrap(env)
    E, slots = group_size(envs_per_policy, core.num_envs, "envs_per_policy", "policy")
    phases = _phases(n_eval_steps, window_steps)
    policies = list(policies)
    plan = plan_policy_batches(len(policies), slots)
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        precision = _model_precision([m for _, m in actors])
    gpl = default_gates_per_lap(core) if gates_per_lap is None else int(gates_per_lap)
    results = [None] * len(actors)
    bank = MfmaPolicyBank(core.state_len, slots, core.device.index)

    def launch(_, steps, rec, recf):
        core.evaluate_bank_device(bank, slots, E, steps, gpl, rec, recf, precision=precision)

    def summarise(_, rec, recf):
        return summarize_eval(rec, recf, core.dt, gpl)

    try:
        for idx, summaries in fly_batches(plan, _shared_starts(core, bank, actors, E, seed), launch, phases, (REC_INTS, REC_FLOATS), summarise,
                                          core.num_envs, E, core.device):
            results[idx] = _window_total(summaries)
    finally:
        _sync_and_close(core, bank)
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
    from .conditions import ConditionBank
    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap

    core = _unwrap(env)
    E, slots = group_size(envs_per_cell, core.num_envs, "envs_per_cell", "cell")
    phases = _phases(n_eval_steps, window_steps)
    conditions, policies = list(conditions), list(policies)
    plan = plan_grid_batches(len(policies), len(conditions), slots)
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        precision = _model_precision([m for _, m in actors])
    results = [[None] * len(conditions) for _ in actors]
    pbank = MfmaPolicyBank(core.state_len, len(actors), core.device.index)
    cbank = ConditionBank(core.VARIANT, len(conditions), core.device.index)

    def start(cells):
        core.condition_starts(conditions, [c for _, c in cells], E, seed=seed)

    def launch(cells, steps, rec, recf):
        core.evaluate_grid_device(pbank, cbank, [p for p, _ in cells], [c for _, c in cells], E, steps, rec, recf, precision=precision)

    def summarise(cell, rec, recf):
        return summarize_eval(rec, recf, core.dt, conditions[cell[1]].gates_per_lap)

    try:
        for p, (actor, _) in enumerate(actors):
            pbank.load_torch(p, actor)
        for c, cond in enumerate(conditions):
            cbank.set(c, cond)
        for (p, c), summaries in fly_batches(plan, start, launch, phases, (REC_INTS, REC_FLOATS), summarise, core.num_envs, E, core.device):
            results[p][c] = _window_total(summaries)
    finally:
        _sync_and_close(core, pbank, cbank)
    return results


def plan_dynamics_batches(num_policies, num_conditions, num_dynamics, slots):
    """How evaluate_dynamics_grid spreads the policies x conditions x vehicles cells over launches of `slots` groups each: cells in
    row-major order (cell k = (k // (C D), (k // D) % C, k % D)), each batch a list of exactly `slots` (policy, condition, dynamics)
    triples, the last batch padded by repeating its last cell; `kept` = how many leading groups of the batch are real.  Returns
    [(cells, kept), ...]; pure arithmetic, no device."""
    P, Cn, D, slots = int(num_policies), int(num_conditions), int(num_dynamics), int(slots)
    if P < 1 or Cn < 1 or D < 1:
        raise ValueError("need at least one policy, one condition and one vehicle")
    if slots < 1:
        raise ValueError("the env holds no complete group: num_envs < envs_per_cell")
    total = P * Cn * D
    plan = []
    for first in range(0, total, slots):
        real = [(k // (Cn * D), (k // D) % Cn, k % D) for k in range(first, min(first + slots, total))]
        plan.append((real + [real[-1]] * (slots - len(real)), len(real)))
    return plan


def evaluate_dynamics_grid(policies, conditions, dynamics, env, envs_per_cell=256, n_eval_steps=2000, window_steps=1200, precision=None, seed=0):
    """evaluate_grid with a third axis: every cell of `policies` x `conditions` x `dynamics` (dynamics.DynamicsParams: the coefficients
    of the equations of motion), `env.num_envs // envs_per_cell` cells per launch (qr_evaluate_policy_dynamics_grid).  Starts, restarts,
    entries of `policies`, `precision` and the summaries are evaluate_grid's: all cells see the same uniform draws, and a cell whose
    vehicle is DynamicsParams.nominal flies what evaluate_grid's cell (p, c) flies.  The residual networks and the observation are
    `env`'s.  Returns results[p][c][d], each a {"window", "total"} dict.  `env` keeps its own configuration."""
    from .conditions import ConditionBank
    from .dynamics import DynamicsBank
    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap

    core = _unwrap(env)
    E, slots = group_size(envs_per_cell, core.num_envs, "envs_per_cell", "cell")
    phases = _phases(n_eval_steps, window_steps)
    conditions, policies, dynamics = list(conditions), list(policies), list(dynamics)
    plan = plan_dynamics_batches(len(policies), len(conditions), len(dynamics), slots)
    for d in dynamics:
        if d.variant != core.VARIANT:
            raise ValueError("DynamicsParams of another variant than the env")
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        precision = _model_precision([m for _, m in actors])
    results = [[[None] * len(dynamics) for _ in conditions] for _ in actors]
    pbank = MfmaPolicyBank(core.state_len, len(actors), core.device.index)
    cbank = ConditionBank(core.VARIANT, len(conditions), core.device.index)
    dbank = DynamicsBank(core.VARIANT, len(dynamics), core.device.index)

    def start(cells):
        core.condition_starts(conditions, [c for _, c, _ in cells], E, seed=seed)

    def launch(cells, steps, rec, recf):
        core.evaluate_dynamics_grid_device(pbank, cbank, dbank, [p for p, _, _ in cells], [c for _, c, _ in cells], [d for _, _, d in cells], E,
                                           steps, rec, recf, precision=precision)

    def summarise(cell, rec, recf):
        return summarize_eval(rec, recf, core.dt, conditions[cell[1]].gates_per_lap)

    try:
        for p, (actor, _) in enumerate(actors):
            pbank.load_torch(p, actor)
        for c, cond in enumerate(conditions):
            cbank.set(c, cond)
        for d, dyn in enumerate(dynamics):
            dbank.set(d, dyn)
        for (p, c, d), summaries in fly_batches(plan, start, launch, phases, (REC_INTS, REC_FLOATS), summarise, core.num_envs, E, core.device):
            results[p][c][d] = _window_total(summaries)
    finally:
        _sync_and_close(core, pbank, cbank, dbank)
    return results


def check_command_history(command_history, gates_ahead):
    """command_history as an int: 0 (none), or H in 1 .. 4 - gates_ahead -- the row of obs_len + 4 H floats is as long as the observation
    of an env with gates_ahead + H gates ahead, and the policy kernels exist for up to 4."""
    H = int(command_history)
    if H != command_history or H < 0 or (H > 0 and int(gates_ahead) + H > 4):
        raise ValueError("command_history must be 0 or an integer in 1 .. 4 - gates_ahead (gates_ahead=%d: at most %d); got %r"
                         % (int(gates_ahead), 4 - int(gates_ahead), command_history))
    return H


def evaluate_sensing_grid(policies, conditions, sensing, env, dynamics=None, envs_per_cell=256, n_eval_steps=2000, window_steps=1200, precision=None,
                          seed=0, noise_seed=0, command_history=0):
    """evaluate_grid with the sensor as third axis: every cell of `policies` x `conditions` x `sensing` (sensing.SensingParams: noise on
    the observation the policy sees, a command delay of 0..4 steps), `env.num_envs // envs_per_cell` cells per launch
    (qr_evaluate_policy_sensing_grid), all flown as ONE vehicle, `dynamics` (a dynamics.DynamicsParams; default: the nominal one).
    Starts, restarts, entries of `policies`, `precision` and the summaries are evaluate_grid's; all cells see the same uniform draws and,
    keyed by `noise_seed`, the same normal draws, so two columns differ by their sensor alone.  The command queues are zeroed with each
    start and the noise stream's step counter runs on across the phases.  The column of SensingParams.ideal() equals
    evaluate_dynamics_grid's cell for that vehicle.  Returns results[p][c][s], each a {"window", "total"} dict.
    command_history = H > 0 (1 .. 4 - gates_ahead): the policies OBSERVE THEIR LAST H COMMANDS (qr_evaluate_policy_history_grid) -- they have
    obs_len + 4 H inputs and are fed [noisy observation | the last H clipped commands computed in the episode], as
    PPO(command_history=H) trains them.  0 (the default) is the call without it, unchanged."""
    import torch

    from .conditions import ConditionBank
    from .dynamics import DynamicsBank
    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap
    from .sensing import QUEUE_FLOATS, SensingBank

    core = _unwrap(env)
    H = check_command_history(command_history, core.gates_ahead)
    E, slots = group_size(envs_per_cell, core.num_envs, "envs_per_cell", "cell")
    phases = _phases(n_eval_steps, window_steps)
    conditions, policies, sensing = list(conditions), list(policies), list(sensing)
    plan = plan_dynamics_batches(len(policies), len(conditions), len(sensing), slots)   # cells (policy, condition, sensor)
    if dynamics is not None and dynamics.variant != core.VARIANT:
        raise ValueError("DynamicsParams of another variant than the env")
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        precision = _model_precision([m for _, m in actors])
    results = [[[None] * len(sensing) for _ in conditions] for _ in actors]
    pbank = MfmaPolicyBank(core.state_len + 4 * H, len(actors), core.device.index)
    cbank = ConditionBank(core.VARIANT, len(conditions), core.device.index)
    dbank = DynamicsBank(core.VARIANT, 1, core.device.index)
    sbank = SensingBank(len(sensing), core.device.index)
    pending = torch.zeros((core.num_envs, QUEUE_FLOATS), dtype=torch.float32, device=core.device)
    flown = [0]   # steps since the start of the batch: the next launch's first_step

    def start(cells):
        core.condition_starts(conditions, [c for _, c, _ in cells], E, seed=seed)
        pending.zero_()
        flown[0] = 0

    def launch(cells, steps, rec, recf):
        maps = ([p for p, _, _ in cells], [c for _, c, _ in cells], [0] * len(cells), [s for _, _, s in cells])
        if H > 0:
            core.evaluate_history_grid_device(pbank, cbank, dbank, sbank, *maps, H, E, steps, pending, rec, recf, precision=precision,
                                              noise_seed=noise_seed, first_step=flown[0])
        else:
            core.evaluate_sensing_grid_device(pbank, cbank, dbank, sbank, *maps, E, steps, pending, rec, recf, precision=precision,
                                              noise_seed=noise_seed, first_step=flown[0])
        flown[0] += int(steps)

    def summarise(cell, rec, recf):
        return summarize_eval(rec, recf, core.dt, conditions[cell[1]].gates_per_lap)

    try:
        for p, (actor, _) in enumerate(actors):
            pbank.load_torch(p, actor)
        for c, cond in enumerate(conditions):
            cbank.set(c, cond)
        dbank.set(0, dynamics)
        for s, sen in enumerate(sensing):
            sbank.set(s, sen)
        for (p, c, s), summaries in fly_batches(plan, start, launch, phases, (REC_INTS, REC_FLOATS), summarise, core.num_envs, E, core.device):
            results[p][c][s] = _window_total(summaries)
    finally:
        _sync_and_close(core, pbank, cbank, dbank, sbank)
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
    mean_reward, std_reward = _reward_stats(recf, n, episodes)
    return dict(envs=n, steps=int(rec[:, 0].max()) if n else 0, episodes=episodes,
                successes=successes, timeouts=timeouts, out_of_bounds=oob, ground=ground, collisions=collisions,
                success_rate=successes / episodes if episodes else None,
                mean_success_seconds=int(tot[6]) * dt / successes if successes else None,
                best_success_seconds=int(best.min()) * dt if best.size else None,
                mean_episode_seconds=int(tot[7]) * dt / episodes if episodes else None,
                gates_per_episode=(int(tot[8]) + successes) / episodes if episodes else None,
                mean_reward=mean_reward, std_reward=std_reward)


def evaluate_q3_policy(model, env, n_eval_steps=2000, precision=None, seed=None):
    """evaluate_policy for the predecessor envs: deterministic evaluation of `model`'s current policy on `env` (a Quadcopter3DVec /
    Quadcopter3DVecGates, possibly inside a VecMonitor) as ONE kernel launch of `n_eval_steps` steps (q3_evaluate_policy).  Returns
    summarize_q3_eval's dict.  `model`, `seed`, `precision` and where `env` is left: as evaluate_policy."""
    n_eval_steps = int(n_eval_steps)
    if n_eval_steps < 1:
        raise ValueError("need n_eval_steps >= 1")
    with flying_policy(model, env, precision, seed) as (core, policy, precision, _):
        rec, recf = zero_records(core.num_envs, (Q3_REC_INTS, Q3_REC_FLOATS), core.device)
        core.evaluate_device(policy, n_eval_steps, rec, recf, precision=precision)
        return summarize_q3_eval(rec, recf, core.dt)


def evaluate_q3_policies(policies, env, envs_per_policy=256, n_eval_steps=2000, precision=None, seed=0):
    """evaluate_q3_policy for a LIST of policies, `env.num_envs // envs_per_policy` of them per launch (q3_evaluate_policy_bank): policy
    p of a batch flies envs [p E, (p + 1) E) of `env`.  Batches, shared starts and restarts, entries, envs_per_policy, precision and the
    padding of the last batch: as evaluate_policies, so every policy flies what an E-env handle sees under
    evaluate_q3_policy(..., seed=seed).  Returns one summarize_q3_eval dict per policy, in order."""
    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap

    core = _unwrap(env)
    E, slots = group_size(envs_per_policy, core.num_envs, "envs_per_policy", "policy")
    n_eval_steps = int(n_eval_steps)
    if n_eval_steps < 1:
        raise ValueError("need n_eval_steps >= 1")
    policies = list(policies)
    plan = plan_policy_batches(len(policies), slots)
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        precision = _model_precision([m for _, m in actors])
    results = [None] * len(actors)
    bank = MfmaPolicyBank(core.state_len, slots, core.device.index)

    def launch(_, steps, rec, recf):
        core.evaluate_bank_device(bank, slots, E, steps, rec, recf, precision=precision)

    def summarise(_, rec, recf):
        return summarize_q3_eval(rec, recf, core.dt)

    try:
        for idx, (summary,) in fly_batches(plan, _shared_starts(core, bank, actors, E, seed), launch, [n_eval_steps],
                                           (Q3_REC_INTS, Q3_REC_FLOATS), summarise, core.num_envs, E, core.device):
            results[idx] = summary
    finally:
        _sync_and_close(core, bank)
    return results
