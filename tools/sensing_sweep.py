#!/usr/bin/env python3
"""Which sensing error breaks this policy first, and how many control steps of latency can it fly with?  Every checkpoint flies through
every sensor of a noise-scale x command-delay table: --base-sigma (eight sigmas in the units of the observation the policy sees) times
each of --noise-scales, under each of --delays, all cells on the same random numbers, `num_envs // envs_per_cell` cells per launch
(evaluate_sensing_grid -> qr_evaluate_policy_sensing_grid).  GPU box.

    python tools/sensing_sweep.py --load CKPT [--load OTHER ...] [--noise-scales 0,0.5,1,2] [--delays 0,1,2,3,4]
        [--base-sigma 0.02,0.05,0.02,0.1,0.02,0.02,0.02,0.02] [--variant e2e] [--track square] [--gates-ahead 1] [--envs-per-cell 256]
        [--num-envs 65536] [--steps 2000] [--window 1200] [--seed 0] [--noise-seed 0] [--precision f16-operands] [--out sweep.json]

Prints two tables per checkpoint, a row per noise scale and a column per delay: crashes per window, and flying-lap seconds.  The cell of
the ideal sensor (scale 0, delay 0) is marked with `*`.  --base-sigma is position, velocity, attitude, body rates, actuator state, gate
position, gate yaw, disturbance columns (sensing.SIGMA_FIELDS); one value is taken for all eight.  The vehicle is the nominal one.  The env
is built like robustness_sweep.py builds its own: training disturbance ranges for E2E, no time limit to speak of."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from robustness_sweep import expand, fmt   # the sweep tools share their argument forms

DEFAULT_SIGMA = "0.02,0.05,0.02,0.1,0.02,0.02,0.02,0.02"


def parse_scales(text):
    """"0,0.5,1" -> [0.0, 0.5, 1.0]; order kept, duplicates and negative or non-finite values refused"""
    try:
        scales = [float(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise SystemExit("--noise-scales takes comma-separated numbers, got %r" % text)
    if not scales or any(not (0.0 <= s < float("inf")) for s in scales) or len(set(scales)) != len(scales):
        raise SystemExit("--noise-scales needs distinct finite values >= 0, got %r" % text)
    return scales


def parse_delays(text):
    try:
        delays = [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise SystemExit("--delays takes comma-separated integers, got %r" % text)
    if not delays or any(not 0 <= d <= 4 for d in delays) or len(set(delays)) != len(delays):
        raise SystemExit("--delays needs distinct integers in [0, 4], got %r" % text)
    return delays


def parse_sigma(text):
    try:
        sigma = [float(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise SystemExit("--base-sigma takes comma-separated numbers, got %r" % text)
    if len(sigma) == 1:
        sigma = sigma * 8
    if len(sigma) != 8 or any(not (0.0 <= s < float("inf")) for s in sigma):
        raise SystemExit("--base-sigma needs one or eight finite values >= 0, got %r" % text)
    return sigma


def format_tables(path, scales, delays, cells):
    """the two printed tables of one checkpoint: cells[i][j] = the {"window", "total"} dict of scales[i] under delays[j]"""
    out = []
    for title, value in (("crashes per window", lambda r: "%.4f" % float(r["window"]["crashes_per_window"])),
                         ("flying-lap seconds", lambda r: fmt(r["total"]["flying_lap_seconds"]))):
        out.append("%s  %s" % (path, title))
        out.append("  %-12s" % "noise scale" + "".join("  %10s" % ("d = %d" % d) for d in delays))
        for s, row in zip(scales, cells):
            out.append("  %-12s" % ("x%g" % s) + "".join("  %10s" % (value(r) + ("*" if s == 0.0 and d == 0 else "")) for d, r in zip(delays, row)))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--load", action="append", required=True, metavar="CKPT_OR_DIR", help="a checkpoint written by model.save, or a directory of them; repeatable")
    ap.add_argument("--noise-scales", default="0,0.5,1,2")
    ap.add_argument("--delays", default="0,1,2,3,4")
    ap.add_argument("--base-sigma", default=DEFAULT_SIGMA)
    ap.add_argument("--variant", choices=("e2e", "indi"), default="e2e")
    ap.add_argument("--track", choices=("square", "zigzag"), default="square")
    ap.add_argument("--gates-ahead", type=int, default=1)
    ap.add_argument("--envs-per-cell", type=int, default=256)
    ap.add_argument("--num-envs", type=int, default=65536, help="envs of the evaluation handle; lowered to what the grid needs")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--window", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise-seed", type=int, default=0)
    ap.add_argument("--precision", choices=("f16-operands", "f32"), default=None, help="default: f32 if a checkpoint was trained in f32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    paths, scales, delays, sigma = expand(a.load), parse_scales(a.noise_scales), parse_delays(a.delays), parse_sigma(a.base_sigma)

    from optimal_quad_control_rl_amd import (Condition, Quadcopter3DGates, Quadcopter3DGatesINDI, SensingParams, TRAIN_DISTURBANCE_RANGES,
                                             delay_sweep, evaluate_sensing_grid, noise_sweep, square_track, zigzag_track)

    base = SensingParams("base", *sigma)
    sensors = [s for scaled in noise_sweep(base, scales) for s in delay_sweep(scaled, delays)]      # scale-major
    E = a.envs_per_cell
    n = min(a.num_envs // E, len(paths) * len(sensors)) * E                                        # no more groups than cells
    track = {"square": square_track, "zigzag": zigzag_track}[a.track]()
    if a.variant == "e2e":
        env = Quadcopter3DGates(n, *track, gates_ahead=a.gates_ahead, infos_mode="none", seed=a.seed)
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    else:
        env = Quadcopter3DGatesINDI(n, *track, gates_ahead=a.gates_ahead, infos_mode="none", seed=a.seed)
    env.max_steps = 10 ** 6
    cond = Condition.from_env(env, name=a.track)
    # a checkpoint trained with PPO(command_history=H) has obs_len + 4 H inputs: H is read off the checkpoint's input length, and every
    # checkpoint of one sweep must agree (one bank, one launch per batch of cells)
    from optimal_quad_control_rl_amd.evaluation import _as_actor, check_command_history
    extra = sorted({int(_as_actor(p)[0][0].in_features) - env.state_len for p in paths})
    if len(extra) != 1 or extra[0] < 0 or extra[0] % 4:
        raise SystemExit("the checkpoints have %s inputs beyond the env's observation (gates_ahead %d): one command history, a multiple of 4, is needed"
                         % (extra, a.gates_ahead))
    history = check_command_history(extra[0] // 4, a.gates_ahead)
    results = evaluate_sensing_grid(paths, [cond], sensors, env, envs_per_cell=E, n_eval_steps=a.steps, window_steps=a.window, precision=a.precision,
                                    seed=a.seed, noise_seed=a.noise_seed, command_history=history)
    env.close()
    print("# %d checkpoints x %d noise scales x %d delays, base sigma %s, %s track, %d envs per cell, %d steps (window %d), seed %d, noise seed %d, "
          "%d cells per launch%s" % (len(paths), len(scales), len(delays), ",".join("%g" % s for s in sigma), a.track, E, a.steps, a.window, a.seed,
                                     a.noise_seed, n // E, ", command history %d" % history if history else ""))
    D = len(delays)
    tables = [[per_policy[0][i * D:(i + 1) * D] for i in range(len(scales))] for per_policy in results]
    for path, cells in zip(paths, tables):
        print(format_tables(path, scales, delays, cells))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(args=vars(a), noise_scales=scales, delays=delays, base_sigma=sigma,
                           checkpoints=[dict(path=p, cells=c) for p, c in zip(paths, tables)]), f, indent=1)


if __name__ == "__main__":
    main()
