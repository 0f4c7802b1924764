#!/usr/bin/env python3
"""Which checkpoint of a run (or of several seeds) do I keep?  Every checkpoint flies the same starts, disturbances and restarts in
one launch per `num_envs // envs_per_policy` checkpoints (evaluate_policies -> qr_evaluate_policy_bank).  GPU box.

    python tools/rank_checkpoints.py run_dir/ other/model_500.zip [--variant e2e] [--track square] [--gates-ahead 1]
        [--envs-per-policy 256] [--num-envs 65536] [--steps 2000] [--window 1200] [--seed 0] [--precision f16-operands] [--out run.json]

Prints one line per checkpoint in timestep order (timesteps from the checkpoint's `data`, crashes per window, first and flying lap):
the learning curve of the run after the fact; then names the best checkpoint by rank_policies.  --out writes the per-policy dicts.
A directory stands for every *.zip in it.  The env is built like the training tools build theirs: training disturbance ranges for
E2E, no time limit to speak of (10^6 steps), so an episode ends by a crash only."""
import argparse, glob, json, os, sys, zipfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def expand(paths):
    """files as given, directories replaced by their *.zip (sorted by name); duplicates kept out, order kept"""
    out = []
    for p in paths:
        found = sorted(glob.glob(os.path.join(p, "*.zip"))) if os.path.isdir(p) else [p]
        if not found:
            raise SystemExit("no *.zip checkpoint in %s" % p)
        out += [f for f in found if f not in out]
    return out


def timesteps_of(path):
    """num_timesteps from the checkpoint's `data` member (0 when it carries none)"""
    with zipfile.ZipFile(path if os.path.exists(path) else path + ".zip") as z:
        return int(json.loads(z.read("data")).get("num_timesteps", 0))


def fmt(x, spec="%.3f"):
    return "   -  " if x is None else spec % x


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="+", metavar="PATHS_OR_DIR")
    ap.add_argument("--variant", choices=("e2e", "indi"), default="e2e")
    ap.add_argument("--track", choices=("square", "zigzag"), default="square")
    ap.add_argument("--gates-ahead", type=int, default=1)
    ap.add_argument("--envs-per-policy", type=int, default=256)
    ap.add_argument("--num-envs", type=int, default=65536, help="envs of the evaluation handle; lowered to what the checkpoints need")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--window", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", choices=("f16-operands", "f32"), default=None, help="default: f32 if a checkpoint was trained in f32")
    ap.add_argument("--max-crashes", type=float, default=0.1, help="crashes per env and window a ranked checkpoint may have")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from optimal_quad_control_rl_amd import (Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES, evaluate_policies, rank_policies,
                                             square_track, zigzag_track)

    paths = expand(a.paths)
    steps = [timesteps_of(p) for p in paths]
    order = sorted(range(len(paths)), key=lambda i: (steps[i], paths[i]))
    paths, steps = [paths[i] for i in order], [steps[i] for i in order]
    E = a.envs_per_policy
    n = min(a.num_envs // E, len(paths)) * E          # no more groups than checkpoints
    trk = square_track() if a.track == "square" else zigzag_track()
    if a.variant == "e2e":
        env = Quadcopter3DGates(n, *trk, gates_ahead=a.gates_ahead, infos_mode="none", seed=a.seed)
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    else:
        env = Quadcopter3DGatesINDI(n, *trk, gates_ahead=a.gates_ahead, infos_mode="none", seed=a.seed)
    env.max_steps = 10 ** 6
    results = evaluate_policies(paths, env, envs_per_policy=E, n_eval_steps=a.steps, window_steps=a.window, precision=a.precision, seed=a.seed)
    env.close()
    print("# %d checkpoints, %d envs each, %d steps (window %d), seed %d, %d per launch" % (len(paths), E, a.steps, a.window, a.seed, n // E))
    print("# %12s  %14s  %9s  %10s  %s" % ("timesteps", "crashes/window", "first lap", "flying lap", "checkpoint"))
    for p, t, r in zip(paths, steps, results):
        print("  %12d  %14.4f  %9s  %10s  %s" % (t, r["window"]["crashes_per_window"], fmt(r["total"]["first_lap_seconds"]),
                                                 fmt(r["total"]["flying_lap_seconds"]), p))
    ranking = rank_policies(results, max_crashes_per_window=a.max_crashes)
    best = ranking[0]
    ok = results[best]["total"]["flying_lap_seconds"] is not None and results[best]["window"]["crashes_per_window"] <= a.max_crashes
    print("best: %s (timesteps %d, flying lap %s s, %.4f crashes/window)%s" %
          (paths[best], steps[best], fmt(results[best]["total"]["flying_lap_seconds"]).strip(), results[best]["window"]["crashes_per_window"],
           "" if ok else "  -- NO checkpoint is within %.2f crashes/window with a flying lap: this is the least-crashing one" % a.max_crashes))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(args=vars(a), checkpoints=[dict(path=p, timesteps=t, **r) for p, t, r in zip(paths, steps, results)],
                           ranking=[paths[i] for i in ranking]), f, indent=1)


if __name__ == "__main__":
    main()
