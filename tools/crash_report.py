#!/usr/bin/env python3
"""Why does a policy crash, and where?  Fly a checkpoint on the device with the black box armed (blackbox_policy -> qr_blackbox_policy:
one kernel launch, every env keeps its last --window rows and freezes them at its first crash) and print where the crashes happen.

    python tools/crash_report.py CHECKPOINT [--variant e2e|indi] [--track square|zigzag] [--gates-ahead 1] [--scale 1.0] [--num-envs 65536]
                                 [--steps 2000] [--window 64] [--trigger crash|time_limit|any] [--max-steps N] [--stochastic] [--seed 0]
                                 [--precision f16-operands|f32] [--out crashes.npz]
                                 [--obs-noise SIGMA[,...8]] [--delay D] [--vehicle PARAM=SCALE]

CHECKPOINT is what sb3.PPO.save or tools/train_ppo.py --save wrote; the env options are those of tools/robustness_sweep.py (E2E flies
with the training disturbance ranges times --scale).  Prints the cause x target-gate table of the frozen envs, the median time into
the episode and the median speed at the trigger row, and writes the log (CrashLog.save_npz: ring, status, terminal states and the
unrolled flights of the frozen envs, oldest row first, NaN-padded) to --out.

--obs-noise / --delay / --vehicle, or a checkpoint trained with --command-history H (H is read off its input length, as
tools/sensing_sweep.py --load does): the flight is ONE CELL of the sensing-grid evaluator (blackbox_grid -> qr_blackbox_policy_grid) -- that
sensor, that vehicle (one physical parameter scaled, through physical_sweep), the command history, deterministic actions, the evaluator's
starts and noise draws -- so the log belongs to the numbers tools/sensing_sweep.py / tools/reality_gap_sweep.py print for that cell; the
cell's own evaluation summary is printed with it.  Rows then hold the TRUE state and the command FLOWN.  --num-envs must be a multiple of
256 there and --stochastic is refused.  Without any of these, and with a checkpoint without a command history, the call is blackbox_policy's
as before."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimal_quad_control_rl_amd import (PPO, Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES, blackbox_policy, square_track,  # noqa: E402
                                         zigzag_track)
from optimal_quad_control_rl_amd.blackbox import CAUSE_NAMES  # noqa: E402


def report(log, num_gates):
    """the printed lines of a CrashLog"""
    envs = log.frozen_envs()
    lines = ["%d of %d envs froze (window %d rows)" % (len(envs), log.num_envs, log.window)]
    if not len(envs):
        return lines
    table = log.by_gate(num_gates)
    lines.append("%-14s %s  total" % ("cause \\ gate", " ".join("%6d" % g for g in range(num_gates))))
    for (_, name), row in zip(CAUSE_NAMES, table):
        lines.append("%-14s %s %6d" % (name, " ".join("%6d" % c for c in row), row.sum()))
    rows = log.trigger_rows()
    s = log.state_len
    t = rows[:, s + 7] * log.dt
    speed = np.sqrt((rows[:, 3:6].astype(np.float64) ** 2).sum(axis=1))
    lines.append("trigger row: median time into the episode %.2f s (min %.2f, max %.2f), median speed %.2f m/s (max %.2f)"
                 % (np.median(t), t.min(), t.max(), np.median(speed), speed.max()))
    lines.append("rows kept per frozen env: median %d of %d" % (np.median(log.valid[envs]), log.window))
    return lines


def add_cell_options(ap):
    """the options that make the flight one cell of the sensing-grid evaluator (shared with tools/record_flight.py)"""
    ap.add_argument("--obs-noise", default="", metavar="SIGMA[,...8]", help="observation noise: one sigma for all eight groups, or eight")
    ap.add_argument("--delay", type=int, default=None, metavar="D", help="command delay in control steps, 0..4")
    ap.add_argument("--vehicle", default="", metavar="PARAM=SCALE", help="one physical parameter of the vehicle times SCALE (physical_sweep), e.g. Izz=1.25")


def grid_cell(a, env, model):
    """None if the tool's call stays the one-policy call of before; otherwise the cell to fly: dict(condition, sensor, dynamics,
    command_history).  `a`: the parsed options of add_cell_options and --track / --gates-ahead; `model`: the loaded checkpoint."""
    from sensing_sweep import parse_sigma
    from optimal_quad_control_rl_amd import Condition, SensingParams, physical_sweep
    from optimal_quad_control_rl_amd.evaluation import _as_actor, check_command_history

    extra = int(_as_actor(model)[0][0].in_features) - env.state_len
    if extra < 0 or extra % 4:
        raise SystemExit("the checkpoint has %d inputs beyond the env's observation: a command history, a multiple of 4, is needed" % extra)
    history = check_command_history(extra // 4, env.gates_ahead)
    if not (a.obs_noise or a.delay is not None or a.vehicle or history):
        return None
    if getattr(a, "stochastic", False):
        raise SystemExit("--stochastic: a cell of the sensing-grid evaluator flies deterministic actions")
    delay = 0 if a.delay is None else a.delay
    if not 0 <= delay <= 4:
        raise SystemExit("--delay needs an integer in [0, 4], got %r" % a.delay)
    sigma = parse_sigma(a.obs_noise) if a.obs_noise else [0.0] * 8
    dynamics = None
    if a.vehicle:
        name, _, scale = a.vehicle.partition("=")
        try:
            dynamics = physical_sweep(env.VARIANT, name.strip(), [float(scale)])[0]
        except ValueError as err:
            raise SystemExit("--vehicle takes PARAM=SCALE: %s" % err)
    sensor = SensingParams.from_sigma(sigma, delay, "sigma %s d=%d" % (",".join("%g" % x for x in sigma), delay))
    return dict(condition=Condition.from_env(env, name=a.track), sensor=sensor, dynamics=dynamics, command_history=history)


def cell_lines(cell, evaluation):
    """what was flown, and the evaluator's own numbers for it"""
    fly = evaluation["flying_lap_seconds"]
    return ["cell: sensor %s, vehicle %s, command history %d" % (cell["sensor"].name, cell["dynamics"].name if cell["dynamics"] is not None else "nominal",
                                                                 cell["command_history"]),
            "evaluation of the same flight: %.4f crashes per env, %.2f gates per env, flying lap %s s"
            % (float(evaluation["crashes_per_env"]), float(evaluation["gates_per_env"]), "none" if fly is None else "%.3f" % fly)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("--variant", choices=("e2e", "indi"), default="e2e")
    ap.add_argument("--track", choices=("square", "zigzag"), default="square")
    ap.add_argument("--gates-ahead", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="disturbance scale (E2E): the training ranges times this")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--trigger", choices=("crash", "time_limit", "any"), default="crash")
    ap.add_argument("--max-steps", type=int, default=10 ** 6, help="the env's time limit")
    ap.add_argument("--stochastic", action="store_true", help="sample actions with the checkpoint's log_std instead of flying the mean")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", choices=("f16-operands", "f32"), default=None, help="default: f32 if the checkpoint was trained in f32")
    ap.add_argument("--out", default="crashes.npz", help="'' = write nothing")
    add_cell_options(ap)
    a = ap.parse_args()

    trk = square_track() if a.track == "square" else zigzag_track()
    cls = Quadcopter3DGates if a.variant == "e2e" else Quadcopter3DGatesINDI
    env = cls(a.num_envs, *trk, gates_ahead=a.gates_ahead, infos_mode="none", seed=a.seed)
    if a.variant == "e2e":
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        env.disturbance_scale = a.scale
    env.max_steps = a.max_steps
    model = PPO.load(a.checkpoint)
    cell = grid_cell(a, env, model)
    if cell is None:
        log = blackbox_policy(model, env, a.steps, window=a.window, trigger=a.trigger, deterministic=not a.stochastic, seed=a.seed, precision=a.precision)
    else:
        from optimal_quad_control_rl_amd import blackbox_grid

        if a.num_envs % 256:
            raise SystemExit("--num-envs must be a multiple of 256 for a cell of the sensing-grid evaluator")
        log = blackbox_grid([model], [cell["condition"]], [cell["sensor"]], env, dynamics=cell["dynamics"], envs_per_cell=a.num_envs, n_steps=a.steps,
                            window=a.window, trigger=a.trigger, precision=a.precision, seed=a.seed, noise_seed=a.seed,
                            command_history=cell["command_history"])[0][0][0]
    print("# %s: %s %s track, %d envs x %d steps (%.1f s), trigger %s, seed %d"
          % (a.checkpoint, a.variant, a.track, a.num_envs, a.steps, a.steps * float(log.dt), a.trigger, a.seed))
    for line in ([] if cell is None else cell_lines(cell, log.evaluation)) + report(log, len(trk[0])):
        print(line)
    if a.out:
        print("wrote", log.save_npz(a.out))
    env.close()


if __name__ == "__main__":
    main()
