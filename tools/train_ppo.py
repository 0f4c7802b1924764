#!/usr/bin/env python3
"""BASELINE config 5: PPO on the MI355X race env (GPU box).

    python tools/train_ppo.py [--variant indi|e2e] [--envs 65536] [--steps 3e8] [--track square|zigzag]
        [--fused --train-scales 0.5,1,2] [--fused --train-tracks square,zigzag]

--train-scales / --train-tracks (with --fused): the collect phase flies a MIX of flight conditions in one launch
(PPO(conditions=...) -> qr_rollout_policy_conditions): one condition per disturbance scale (E2E only), per named track (its own start
and lap length), or per (track, scale) pair when both are given.  The log then carries one line per condition, and --eval-final adds the
final policy's robustness table over the same conditions (evaluate_grid).
--vehicle-spread S [--resample-every R] (with --fused): the collect phase flies an ENSEMBLE of vehicles, one per group of envs, drawn on
the device within 1 +- S of the identified parameters (PPO(dynamics=VehicleRanges(...)) -> qr_rollout_policy_dynamics); --eval-final then
prints the final policy's reality-gap table (evaluate_dynamics_grid over a physical_sweep of three parameters across 1 +- S).
--obs-noise SIGMA[,...8] [--delay D[,D...]] (with --fused): the collect phase flies under observation noise and command delay
(PPO(sensing=...) -> qr_rollout_policy_sensing): one sensor per delay value (default 0), round-robin over the groups, every sensor with
the given sigmas (one value for all eight groups of observation entries, or eight; default none).  The log then carries one line per
sensor, and --eval-final prints the final policy's table over the training sensors plus the ideal one (evaluate_sensing_grid).
--command-history H (with --fused): the policy OBSERVES ITS LAST H COMMANDS (PPO(command_history=H) -> qr_rollout_policy_history): its row is
[observation | the last H clipped commands computed in the episode]; without --obs-noise / --delay the run flies under one ideal sensor.
Every evaluation of the run (the final line, --eval-final, --curve) then goes through evaluate_sensing_grid(..., command_history=H) under
the training sensors -- the first one for the keys of the result line.  --eval-delays D[,D...]: --eval-final's table over the training
sigmas at these delays instead of the training sensors (with or without --command-history).
--privileged-critic (with --fused --native-update): the VALUE network reads the observation before the sensor's noise
(PPO(privileged_critic=True) -> qr_rollout_policy_privileged + qr_ppo_epoch_privileged); the policy keeps reading the noisy row.  Nothing
about the evaluations changes (they fly the actor); --save stores the flag in the checkpoint's metadata, which the loading tools ignore.

Prints training progress and a final deterministic evaluation on the 4-gate square track: gates per 12 s from a standing
start, and lap times the way the reference tabulates them (FP:3474-3488: lap 1 from the start, then the flying laps; its
simulated E2E policy flies 2.97 s then 2.51-2.59 s, INDI 3.20 s then 2.75-2.82 s)."""
import argparse, os, sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from robustness_sweep import condition_name, format_table, parse_scales, parse_tracks   # the sweep tool's argument forms and table
from sensing_sweep import parse_delays, parse_sigma                                      # likewise: --obs-noise is its --base-sigma


def train_conditions(env, variant, scales=None, tracks=None):
    """The conditions of --train-scales / --train-tracks (parsed lists or None) around `env`'s own configuration: None without
    either; one per scale ("scale=<s>", disturbance_sweep); one per track (named after it, with its own start and lap length); the
    product, track-major ("<track> x<s>"), when both are given."""
    from optimal_quad_control_rl_amd import Condition, disturbance_sweep, square_track, zigzag_track

    if scales is None and tracks is None:
        return None
    if scales is not None and variant != "e2e":
        raise SystemExit("--train-scales needs --variant e2e: the INDI variant has no disturbances")
    if tracks is None:
        return disturbance_sweep(env, scales)
    track_of = {"square": square_track, "zigzag": zigzag_track}
    conds = []
    for t in tracks:
        gate_pos, gate_yaw, start_pos = track_of[t]()
        base = Condition.from_env(env, name=t, gate_pos=gate_pos, gate_yaw=gate_yaw, start_pos=start_pos)
        conds += [base] if scales is None else [base.replace(name=condition_name(t, s), disturbance_scale=s) for s in scales]
    return conds


def train_sensors(obs_noise="", delay=""):
    """The sensors of --obs-noise / --delay (their texts, "" = not given): None without either; otherwise one SensingParams per delay
    value (default: 0), each with the sigmas of --obs-noise (default: none), named "d=<delay>"."""
    from optimal_quad_control_rl_amd.sensing import SensingParams

    if not obs_noise and not delay:
        return None
    sigma = parse_sigma(obs_noise) if obs_noise else [0.0] * 8
    delays = parse_delays(delay) if delay else [0]
    return [SensingParams("d=%d" % d, *sigma, delay_steps=d) for d in delays]


def save_checkpoint(model, path, a):
    """--save: the final policy as an SB3-shaped checkpoint that sb3.PPO.load (and with it every tool that takes --load) reads: `data`
    (the metadata, with command_history and privileged_critic of the run beside the keys of sb3.PPO.save) and `policy.pth` (both networks
    under their SB3 names).  A policy checkpoint: no optimiser state, no env state.  Returns the path written."""
    import io
    import zipfile

    import torch
    from optimal_quad_control_rl_amd import sb3

    path = str(path)
    if not os.path.splitext(path)[1]:
        path += ".zip"
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    data = dict(format_version=sb3.FORMAT_VERSION, algo="PPO", policy_class="MlpPolicy", observation_dim=int(model.policy.pi[0].in_features),
                action_dim=4, net_arch=[120, 120, 120], activation_fn="ReLU", log_std_init=0.0, num_timesteps=int(model.num_timesteps),
                seed=int(a.seed), precision="f32" if a.precision == "f32" else "f16-operands", learning_rate=float(a.lr), n_steps=int(a.n_steps),
                batch_size=int(model.batch_size), n_epochs=int(a.epochs), gamma=float(a.gamma), gae_lambda=float(model.lam),
                clip_range=float(model.clip), ent_coef=float(a.ent_coef), vf_coef=float(model.vf_coef), max_grad_norm=float(model.max_grad_norm),
                target_kl=float(a.target_kl), command_history=int(a.command_history), privileged_critic=bool(a.privileged_critic))
    blob = io.BytesIO()
    torch.save({k: v.detach().cpu() for k, v in sb3.ActorCriticPolicy(model.policy).state_dict().items()}, blob)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        z.writestr("data", json.dumps(data, indent=1))
        z.writestr("policy.pth", blob.getvalue())
    return path


def format_condition_stats(per_condition):
    """one line per entry of PPO.stats["per_condition"]"""
    return "\n".join("     %-16s episodes %7d  ep_rew %8.2f  ep_len %7.1f  crashes %7d  time limits %6d"
                     % (c["name"], c["episodes"], c["mean_return"], c["mean_length"], c["crashes"], c["time_limits"]) for c in per_condition)


def main():
    import torch
    from optimal_quad_control_rl_amd import (Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES,
                                             square_track, zigzag_track)
    from optimal_quad_control_rl_amd.ppo import PPO

    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="indi")
    ap.add_argument("--track", default="square")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=float, default=3e8)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--target-kl", type=float, default=0.02)
    ap.add_argument("--lr-final", type=float, default=0.1)
    ap.add_argument("--fused", action="store_true", help="collect with the closed-loop rollout kernel (qr_rollout_policy)")
    ap.add_argument("--native-update", action="store_true", help="minibatch updates in the matrix-core kernels (qr_ppo_minibatch)")
    ap.add_argument("--precision", default="f16-operands", choices=("f16-operands", "f32-collect", "f32"),
                    help="f32: the reference-precision kernels for collect, values and update (needs --fused --native-update); f32-collect: collect only")
    ap.add_argument("--ent-coef", type=float, default=0.0)
    ap.add_argument("--gamma", type=float, default=0.999)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trunc-bootstrap", action="store_true", help="round-1 behaviour: a time-limit truncation is a termination")
    ap.add_argument("--eval-final", action="store_true", help="evaluate the FINAL policy (no best-by-training-statistic checkpoint)")
    ap.add_argument("--save", default="", help="save an SB3-shaped checkpoint (optimal_quad_control_rl_amd.sb3 format) of the final model here")
    ap.add_argument("--curve", type=int, default=0, help="evaluate the current policy every this many rollouts (training clock stopped)")
    ap.add_argument("--lap-target", type=float, default=2.6, help="flying lap (s) that counts as the reference's level for --curve")
    ap.add_argument("--device-eval", action="store_true", help="evaluate with the on-device evaluator (evaluate_policy -> qr_evaluate_policy: two launches, gate passes "
                    "detected from the target gate) instead of the per-step loop below; opt-in, because committed profiles quote the loop's numbers")
    ap.add_argument("--train-scales", default="", help="with --fused: train on one condition per disturbance scale, e.g. 0.5,1,2 (E2E only)")
    ap.add_argument("--train-tracks", default="", help="with --fused: train on one condition per named track, e.g. square,zigzag; with --train-scales: the product")
    ap.add_argument("--envs-per-group", type=int, default=256, help="envs per group of the condition mix (a multiple of 256)")
    ap.add_argument("--vehicle-spread", type=float, default=0.0,
                    help="with --fused: train on an ensemble of vehicles, one per group, every physical parameter drawn within 1 +- S of its "
                         "identified value (PPO(dynamics=VehicleRanges(variant, S)) -> qr_rollout_policy_dynamics)")
    ap.add_argument("--resample-every", type=int, default=0,
                    help="with --vehicle-spread: draw the ensemble again before every R-th rollout (envs mid-episode change vehicle); 0: drawn once")
    ap.add_argument("--obs-noise", default="", metavar="SIGMA[,...8]",
                    help="with --fused: train under white Gaussian noise on the observation the policy sees, one sigma for all eight groups of "
                         "entries or eight (position, velocity, attitude, body rates, actuator state, gate position, gate yaw, disturbances)")
    ap.add_argument("--delay", default="", metavar="D[,D...]",
                    help="with --fused: train under a command delay of D control steps (0..4); a list gives one sensor per value, round-robin "
                         "over the groups (PPO(sensing=...) -> qr_rollout_policy_sensing)")
    ap.add_argument("--command-history", type=int, default=0, metavar="H",
                    help="with --fused: the policy observes its last H clipped commands, 1 .. 4 - gates_ahead (PPO(command_history=H) -> "
                         "qr_rollout_policy_history); evaluations go through evaluate_sensing_grid(..., command_history=H)")
    ap.add_argument("--privileged-critic", action="store_true",
                    help="with --fused --native-update: the value network reads the observation before the sensor's noise "
                         "(PPO(privileged_critic=True) -> qr_rollout_policy_privileged, qr_ppo_epoch_privileged); stored in --save's metadata")
    ap.add_argument("--eval-delays", default="", metavar="D[,D...]",
                    help="--eval-final's sensor table at these command delays (the training sigmas) instead of at the training sensors")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    # one process per GPU under torchrun (data-parallel PPO: --envs is per GPU, env_id_base = rank * envs keys disjoint reset and
    # action-noise streams; gradients are averaged per minibatch, see MfmaPpoUpdater.minibatch)
    rank, world, local_rank = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("WORLD_SIZE", 1), ("LOCAL_RANK", 0)))
    if "RANK" in os.environ:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        assert a.native_update, "data-parallel training uses the matrix-core update (--native-update)"
    if rank != 0:
        sys.stdout = open(os.devnull, "w")

    trk = square_track() if a.track == "square" else zigzag_track()
    cls = Quadcopter3DGates if a.variant == "e2e" else Quadcopter3DGatesINDI
    env = cls(a.envs, *trk, gates_ahead=1, infos_mode="none", seed=1 + a.seed, env_id_base=rank * a.envs)
    if a.variant == "e2e":
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    conds = train_conditions(env, a.variant, parse_scales(a.train_scales) if a.train_scales else None,
                             parse_tracks(a.train_tracks) if a.train_tracks else None)
    if conds is not None and not a.fused:
        raise SystemExit("--train-scales / --train-tracks need --fused: the mix of conditions exists in the closed-loop kernel only")
    ranges = None
    if a.vehicle_spread > 0.0:
        if not a.fused:
            raise SystemExit("--vehicle-spread needs --fused: the mix of vehicles exists in the closed-loop kernel only")
        from optimal_quad_control_rl_amd.dynamics import VehicleRanges
        ranges = VehicleRanges(env.VARIANT, a.vehicle_spread)
    elif a.resample_every:
        raise SystemExit("--resample-every belongs to --vehicle-spread")
    sensors = train_sensors(a.obs_noise, a.delay)
    if sensors is not None and not a.fused:
        raise SystemExit("--obs-noise / --delay need --fused: the sensor exists in the closed-loop kernel only")
    if a.command_history:
        if not a.fused:
            raise SystemExit("--command-history needs --fused: the row is assembled in the closed-loop kernel only")
        if sensors is None:   # what PPO(command_history=H) flies under without `sensing`; named here for the tables
            from optimal_quad_control_rl_amd.sensing import SensingParams
            sensors = [SensingParams.ideal()]
    if a.privileged_critic:
        if not (a.fused and a.native_update) or a.precision == "f32" or world > 1:
            raise SystemExit("--privileged-critic needs --fused --native-update at f16-operand update precision in one process: the clean row exists "
                             "in the closed-loop kernel only, and the f32-class and data-parallel updates have no privileged-critic form")
        if sensors is None:   # what PPO(privileged_critic=True) flies under without `sensing`; named here for the tables
            from optimal_quad_control_rl_amd.sensing import SensingParams
            sensors = [SensingParams.ideal()]
    model = PPO(env, seed=a.seed, ent_coef=a.ent_coef, gamma=a.gamma, n_steps=a.n_steps, n_epochs=a.epochs, batch_size=a.envs * a.n_steps // a.minibatches, learning_rate=a.lr,
                target_kl=a.target_kl, lr_final_frac=a.lr_final, total_timesteps_hint=int(a.steps) // world, fused_collect=a.fused,
                native_update=a.native_update, truncation_bootstrap=not a.no_trunc_bootstrap,
                policy_forward="f32class" if a.precision != "f16-operands" else "torch", update_precision="f32" if a.precision == "f32" else "f16-operands",
                conditions=conds, envs_per_group=a.envs_per_group, dynamics=ranges, resample_every=a.resample_every or None, sensing=sensors,
                command_history=a.command_history, privileged_critic=a.privileged_critic)
    if "RANK" in os.environ:
        model._updater.broadcast_parameters(0)   # identical start on every rank (the seed already makes it so; this guarantees it)
        model.noise_seed = a.seed                 # same key, different global env ids -> independent action noise per rank
    # deterministic evaluation on a separate env: 2000 steps = 20 s of flight (six laps), crashes auto-reset and restart the lap count
    n_eval = 4096
    ev = cls(n_eval, *trk, gates_ahead=1, infos_mode="none", seed=99)
    if a.variant == "e2e":
        ev.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    ev.max_steps = 10 ** 6
    G = 4 if a.track == "square" else len(trk[0])   # square_track() lists its four gates twice: a lap is four passes
    dt = 0.01


    @torch.no_grad()
    def evaluate(m):
        ev.seed(99)
        obs = ev.reset_device()
        dev = obs.device
        gates12 = torch.zeros(n_eval, device=dev); crashes12 = torch.zeros(n_eval, device=dev)
        passed = torch.zeros(n_eval, device=dev)            # gates passed since this env's last (re)start
        lap_start = torch.zeros(n_eval, device=dev)         # time of the last lap boundary (or restart)
        lap_sum = torch.zeros(7, device=dev); lap_cnt = torch.zeros(7, device=dev)   # laps 1..6 (index 0 unused)
        for k in range(2000):
            obs, rew, done, trunc = ev.step_device(m.act_device(obs).contiguous())
            t = (k + 1) * dt
            g = (rew > 5).float()
            if k < 1200:
                gates12 += g; crashes12 += (done.float() - trunc.float()).clamp(min=0)
            passed += g
            lap_done = (g > 0) & (passed % G == 0) & (passed > 0)
            lap_no = (passed / G).long().clamp(max=6)
            if lap_done.any():
                sel = lap_done & (passed / G <= 6)
                lap_sum.index_add_(0, lap_no[sel], (t - lap_start)[sel])
                lap_cnt.index_add_(0, lap_no[sel], torch.ones_like(lap_start)[sel])
                lap_start = torch.where(lap_done, torch.full_like(lap_start, t), lap_start)
            d = done.bool()
            passed = torch.where(d, torch.zeros_like(passed), passed)
            lap_start = torch.where(d, torch.full_like(lap_start, t), lap_start)
        laps = (lap_sum / lap_cnt.clamp(min=1)).tolist()
        return dict(eval_gates_per_12s=float(gates12.mean()), eval_crashes_per_12s=float(crashes12.mean()),
                    eval_seconds_per_gate=float(1200 * dt / gates12.mean().clamp(min=1e-9)),
                    eval_seconds_per_lap_4gates=float(4 * 1200 * dt / gates12.mean().clamp(min=1e-9)),
                    eval_lap_seconds={f"lap{i}": laps[i] for i in range(1, 7)}, eval_laps_counted=lap_cnt[1:].tolist(),
                    eval_flying_lap_seconds=float(lap_sum[2:].sum() / lap_cnt[2:].sum().clamp(min=1)))


    def evaluate_on_device(m):
        """the same protocol and keys through evaluate_policy: 1 200-step window for the rates, 2 000 steps for the lap times"""
        from optimal_quad_control_rl_amd import evaluate_policy
        r = evaluate_policy(m, ev, n_eval_steps=2000, window_steps=1200, gates_per_lap=G, seed=99)
        w, t = r["window"], r["total"]
        g12 = max(w["gates_per_window"], 1e-9)
        return dict(eval_gates_per_12s=w["gates_per_window"], eval_crashes_per_12s=w["crashes_per_window"], eval_seconds_per_gate=1200 * dt / g12,
                    eval_seconds_per_lap_4gates=4 * 1200 * dt / g12,
                    eval_lap_seconds={f"lap{i}": (t["lap_seconds"][i - 1] or 0.0) for i in range(1, 7)}, eval_laps_counted=[float(c) for c in t["laps_counted"][:6]],
                    eval_flying_lap_seconds=t["flying_lap_seconds"] or 0.0, eval_mean_reward=t["mean_reward"], evaluator="device")


    def sensor_rows(m, ev_sensors):
        """(name, crashes per window, flying lap s or None, gates per window) of m through each sensor, on the evaluation env (nominal vehicle,
        its own configuration)"""
        from optimal_quad_control_rl_amd import Condition, evaluate_sensing_grid
        cells = evaluate_sensing_grid([m], [Condition.from_env(ev)], ev_sensors, ev, envs_per_cell=256, n_eval_steps=2000, window_steps=1200,
                                      seed=99, noise_seed=a.seed, command_history=a.command_history)[0][0]
        return [(s.name, float(r["window"]["crashes_per_window"]), r["total"]["flying_lap_seconds"], float(r["window"]["gates_per_window"]))
                for s, r in zip(ev_sensors, cells)], cells


    def evaluate_with_history(m):
        """the keys of evaluate_on_device through the history evaluator under the FIRST training sensor: a policy with a command history
        cannot be stepped from the host loop above, whose observations lack the history"""
        _, cells = sensor_rows(m, sensors[:1])
        w, t = cells[0]["window"], cells[0]["total"]
        g12 = max(w["gates_per_window"], 1e-9)
        return dict(eval_gates_per_12s=w["gates_per_window"], eval_crashes_per_12s=w["crashes_per_window"], eval_seconds_per_gate=1200 * dt / g12,
                    eval_seconds_per_lap_4gates=4 * 1200 * dt / g12,
                    eval_lap_seconds={f"lap{i}": (t["lap_seconds"][i - 1] or 0.0) for i in range(1, 7)}, eval_laps_counted=[float(c) for c in t["laps_counted"][:6]],
                    eval_flying_lap_seconds=t["flying_lap_seconds"] or 0.0, eval_mean_reward=t["mean_reward"], evaluator="device, sensor " + sensors[0].name,
                    command_history=a.command_history)


    if a.device_eval:
        evaluate = evaluate_on_device
    if a.command_history:
        evaluate = evaluate_with_history

    best = {"gates": -1.0, "state": None}
    def keep_best(m):
        g = m.stats.get("gates_per_episode", 0.0)
        if g > best["gates"] and m.stats.get("ep_len_mean", 0) > 600:
            best["gates"] = g
            best["state"] = {k: v.clone() for k, v in m.policy.state_dict().items()}
    # --curve K: every K rollouts the CURRENT policy is evaluated (clock stopped) -> wall-clock-to-quality curve (BASELINE config 5's metric)
    curve, paused, it_no = [], [0.0], [0]
    def on_rollout(m):
        if not a.eval_final:
            keep_best(m)
        it_no[0] += 1
        if conds is not None and it_no[0] % 20 == 0:   # under the trainer's own log line (log_every=20 below)
            print(format_condition_stats(m.stats["per_condition"]), flush=True)
        if sensors is not None and it_no[0] % 20 == 0:
            print(format_condition_stats(m.stats["per_sensor"]), flush=True)
        if a.curve and it_no[0] % a.curve == 0 and rank == 0:
            torch.cuda.synchronize()
            e0 = time.perf_counter()
            tsec = e0 - t0 - paused[0]
            r = evaluate(m)
            torch.cuda.synchronize()
            paused[0] += time.perf_counter() - e0
            curve.append(dict(train_seconds=tsec, env_steps=m.num_timesteps * world,
                              flying_lap=r["eval_flying_lap_seconds"], crashes_per_12s=r["eval_crashes_per_12s"], gates_per_12s=r["eval_gates_per_12s"]))
    t0 = time.perf_counter()
    model.learn(int(a.steps) // world, log_every=20, callback=on_rollout)   # --steps counts env-steps of the whole job
    if best["state"] is not None and not a.eval_final:
        model.policy.load_state_dict(best["state"])  # evaluate the best checkpoint (the reference saves one every 10 rollouts, R:823)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0 - paused[0]

    final = evaluate(model)
    res = dict(evaluated="final policy" if a.eval_final else "best checkpoint by training statistic", lr_final_frac=a.lr_final,
               world_size=world, fused_collect=a.fused, native_update=a.native_update, variant=a.variant, track=a.track, envs=a.envs,
               gamma=a.gamma, seed=a.seed, n_steps=a.n_steps, epochs=a.epochs, minibatches=a.minibatches, lr=a.lr, target_kl=a.target_kl,
               truncation_bootstrap=not a.no_trunc_bootstrap,
               train_steps=model.num_timesteps * world, train_seconds=train_s,
               train_Msteps_per_s=model.num_timesteps * world / train_s / 1e6,
               **final, **model.stats)
    if conds is not None:
        print(format_condition_stats(model.stats["per_condition"]), flush=True)
        if a.eval_final and rank == 0:
            # the FINAL policy under each training condition, on the evaluation env (its seed and its time limit: episodes end by a crash only)
            from optimal_quad_control_rl_amd import evaluate_grid
            from optimal_quad_control_rl_amd.evaluation import robustness_table
            ev_conds = [c.replace(max_steps=ev.max_steps) for c in conds]
            cells = evaluate_grid([model], ev_conds, ev, envs_per_cell=256, n_eval_steps=2000, window_steps=1200, seed=99)
            rows = robustness_table(cells, [c.name for c in ev_conds])[0]
            print(format_table("final policy", rows), flush=True)
            res["robustness"] = [dict(condition=n, crashes_per_window=cr, flying_lap_seconds=fl, gates_per_window=g) for n, cr, fl, g in rows]
    if ranges is not None:   # one drawn vehicle per group: the result line carries the spread over them, not one entry per group
        pv = [s for s in res.pop("per_vehicle") if s["episodes"]]
        res["per_vehicle_summary"] = dict(vehicles=a.envs // a.envs_per_group, with_episodes=len(pv), resamples=model._resamples,
                                          mean_return_min=min((s["mean_return"] for s in pv), default=None),
                                          mean_return_max=max((s["mean_return"] for s in pv), default=None))
    if ranges is not None and a.eval_final and rank == 0:
        # the reality-gap table of the FINAL policy: k_w, tau (INDI: tau_T) and Izz (INDI: tau_r) over 1 +- S on the evaluation env
        from optimal_quad_control_rl_amd import Condition, evaluate_dynamics_grid, physical_sweep
        factors = [1.0 - a.vehicle_spread, 1.0, 1.0 + a.vehicle_spread]
        parameters = ("k_w", "tau", "Izz") if a.variant == "e2e" else ("k_x", "tau_T", "tau_r")
        vehicles = [v for name in parameters for v in physical_sweep(ev.VARIANT, name, factors)]
        cells = evaluate_dynamics_grid([model], [Condition.from_env(ev)], vehicles, ev, envs_per_cell=256, n_eval_steps=2000, window_steps=1200, seed=99)[0][0]
        print("reality gap of the final policy (crashes / window, flying lap s, gates / window)", flush=True)
        res["reality_gap"] = []
        for v, r in zip(vehicles, cells):
            lap = r["total"]["flying_lap_seconds"]
            print("  %-12s %10.4f %10s %10.2f" % (v.name, float(r["window"]["crashes_per_window"]), "-" if not lap else "%.3f" % lap,
                                                 float(r["window"]["gates_per_window"])), flush=True)
            res["reality_gap"].append(dict(vehicle=v.name, crashes_per_window=float(r["window"]["crashes_per_window"]), flying_lap_seconds=lap,
                                           gates_per_window=float(r["window"]["gates_per_window"])))
    if sensors is not None:
        print(format_condition_stats(model.stats["per_sensor"]), flush=True)
        if a.eval_final and rank == 0:
            # the FINAL policy through each training sensor and the ideal one, on the evaluation env (nominal vehicle, its own configuration)
            from optimal_quad_control_rl_amd import SensingParams
            if a.eval_delays:
                ev_sensors = [sensors[0].with_delay(d, name="d=%d" % d) for d in parse_delays(a.eval_delays)]
            else:
                ev_sensors = sensors + ([] if any(s.is_ideal for s in sensors) else [SensingParams.ideal()])
            rows, _ = sensor_rows(model, ev_sensors)
            print(format_table("final policy, by sensor", rows).replace("condition", "sensor   ", 1), flush=True)
            res["sensing"] = [dict(sensor=n, crashes_per_window=cr, flying_lap_seconds=fl, gates_per_window=g) for n, cr, fl, g in rows]
    sk, up_n = res.get("skipped_nonfinite", 0), res.get("updates", 0)
    if sk > 0.002 * max(1, sk + up_n):   # a handful of skips = diverged sims in a minibatch; more means something is wrong
        print(f"WARNING: {sk} of {sk + up_n} minibatch updates were skipped for a non-finite gradient norm", file=sys.stderr, flush=True)
    if curve:
        # first time the policy flies laps like the reference's (simulated flying laps 2.51-2.59 s, FP:3474-3488) without crashing
        hit = [c for c in curve if 0 < c["flying_lap"] <= a.lap_target and c["crashes_per_12s"] <= 0.1]
        res["curve"] = curve
        res["seconds_to_reference_lap"] = hit[0]["train_seconds"] if hit else None
        res["env_steps_to_reference_lap"] = hit[0]["env_steps"] if hit else None
        res["lap_target"] = a.lap_target
    if a.save and rank == 0:
        res["saved"] = save_checkpoint(model, a.save, a)
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
