#!/usr/bin/env python3
"""Which parameter error breaks this policy first, and by how much may the real vehicle differ before lap time or crash rate moves?
Every checkpoint flies the reference's vehicle with ONE physical parameter at a time multiplied by each of --factors, all cells on the same
random numbers, `num_envs // envs_per_cell` cells per launch (evaluate_dynamics_grid -> qr_evaluate_policy_dynamics_grid).  GPU box.

    python tools/reality_gap_sweep.py --load CKPT [--load OTHER ...] [--parameters k_w,tau,Izz] [--factors 0.7,0.85,1,1.15,1.3]
        [--variant e2e] [--track square] [--gates-ahead 1] [--envs-per-cell 256] [--num-envs 65536] [--steps 2000] [--window 1200]
        [--seed 0] [--precision f16-operands] [--out sweep.json]

Prints one table per parameter and checkpoint: a row per factor with crashes per window, flying-lap seconds and gates per window; the
row of the nominal vehicle (factor 1) is marked with `*`.  --parameters defaults to every physical parameter of the variant
(optimal_quad_control_rl_amd.dynamics.PHYSICAL).  The sweep works on PHYSICAL parameters: Izz moves seven coefficients of the equations
of motion, tau three.  The residual networks and the observation stay the env's.  The env is built like robustness_sweep.py builds its
own: training disturbance ranges for E2E, no time limit to speak of."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from robustness_sweep import expand, fmt   # the sweep tools share their argument forms


def parse_factors(text):
    """"0.7,1,1.3" -> [0.7, 1.0, 1.3]; order kept, duplicates and non-positive or non-finite values refused"""
    try:
        factors = [float(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise SystemExit("--factors takes comma-separated numbers, got %r" % text)
    if not factors or any(not (0.0 < f < float("inf")) for f in factors) or len(set(factors)) != len(factors):
        raise SystemExit("--factors needs distinct finite values > 0, got %r" % text)
    return factors


def parse_parameters(text, variant):
    from optimal_quad_control_rl_amd.dynamics import PHYSICAL

    known = list(PHYSICAL[0 if variant == "e2e" else 1])
    if not text:
        return known
    names = [t.strip() for t in text.split(",") if t.strip()]
    if not names or any(n not in known for n in names) or len(set(names)) != len(names):
        raise SystemExit("--parameters takes distinct names out of %s, got %r" % (",".join(known), text))
    return names


def format_table(path, parameter, factors, cells):
    """the printed table of one (checkpoint, parameter): cells = one {"window", "total"} dict per factor"""
    lines = ["%s  %s" % (path, parameter), "  %-10s  %14s  %10s  %12s" % ("factor", "crashes/window", "flying lap", "gates/window")]
    for f, r in zip(factors, cells):
        lines.append("%s %-10s  %14.4f  %10s  %12.2f" % ("*" if f == 1.0 else " ", "x%g" % f, float(r["window"]["crashes_per_window"]),
                                                       fmt(r["total"]["flying_lap_seconds"]), float(r["window"]["gates_per_window"])))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--load", action="append", required=True, metavar="CKPT_OR_DIR", help="a checkpoint written by model.save, or a directory of them; repeatable")
    ap.add_argument("--parameters", default="")
    ap.add_argument("--factors", default="0.7,0.85,1,1.15,1.3")
    ap.add_argument("--variant", choices=("e2e", "indi"), default="e2e")
    ap.add_argument("--track", choices=("square", "zigzag"), default="square")
    ap.add_argument("--gates-ahead", type=int, default=1)
    ap.add_argument("--envs-per-cell", type=int, default=256)
    ap.add_argument("--num-envs", type=int, default=65536, help="envs of the evaluation handle; lowered to what the grid needs")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--window", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", choices=("f16-operands", "f32"), default=None, help="default: f32 if a checkpoint was trained in f32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    paths, factors, parameters = expand(a.load), parse_factors(a.factors), parse_parameters(a.parameters, a.variant)

    from optimal_quad_control_rl_amd import (Condition, Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES, evaluate_dynamics_grid,
                                             physical_sweep, square_track, zigzag_track)

    v = 0 if a.variant == "e2e" else 1
    vehicles = [d for p in parameters for d in physical_sweep(v, p, factors)]      # parameter-major
    E = a.envs_per_cell
    n = min(a.num_envs // E, len(paths) * len(vehicles)) * E                      # no more groups than cells
    track = {"square": square_track, "zigzag": zigzag_track}[a.track]()
    if a.variant == "e2e":
        env = Quadcopter3DGates(n, *track, gates_ahead=a.gates_ahead, infos_mode="none", seed=a.seed)
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    else:
        env = Quadcopter3DGatesINDI(n, *track, gates_ahead=a.gates_ahead, infos_mode="none", seed=a.seed)
    env.max_steps = 10 ** 6
    cond = Condition.from_env(env, name=a.track)
    results = evaluate_dynamics_grid(paths, [cond], vehicles, env, envs_per_cell=E, n_eval_steps=a.steps, window_steps=a.window,
                                     precision=a.precision, seed=a.seed)
    env.close()
    print("# %d checkpoints x %d parameters x %d factors, %s track, %d envs per cell, %d steps (window %d), seed %d, %d cells per launch"
          % (len(paths), len(parameters), len(factors), a.track, E, a.steps, a.window, a.seed, n // E))
    F = len(factors)
    for path, per_policy in zip(paths, results):
        for k, parameter in enumerate(parameters):
            print(format_table(path, parameter, factors, per_policy[0][k * F:(k + 1) * F]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(args=vars(a), parameters=parameters, factors=factors,
                           checkpoints=[dict(path=p, cells={par: r[0][k * F:(k + 1) * F] for k, par in enumerate(parameters)})
                                        for p, r in zip(paths, results)]), f, indent=1)


if __name__ == "__main__":
    main()
