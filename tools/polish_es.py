#!/usr/bin/env python3
"""Polish a trained policy on what the evaluator measures: evolution strategies on the policy bank (EvolutionStrategy -> qr_es_*).  GPU box.

    python tools/polish_es.py --load CKPT --generations G [--pairs 128] [--envs-per-policy 256] [--sigma 0.02] [--lr 0.01] [--save OUT]
        [--variant e2e] [--track square] [--gates-ahead 1] [--n-eval-steps 1200] [--eval-seeds fixed|per_generation] [--seed 0]

CKPT is a checkpoint written by `model.save` (optimal_quad_control_rl_amd.PPO).  Every generation flies 2 x pairs perturbed copies of its
actor, `envs_per_policy` envs each, in one launch on shared starts, scores them with fitness="lap" (minus the mean flying-lap steps, minus
a crash penalty; untuned defaults) and takes one Adam ascent step.  One line per generation; at the end `evaluate_policy` of the start and
of the result on the same seed, on a separate evaluation env.  The env is built like the training tools build theirs: training
disturbance ranges for E2E, no time limit to speak of (10^6 steps), so an episode ends by a crash only.  --save writes the polished
model as a checkpoint of the same kind."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fmt(x, spec="%.3f"):
    return "  -  " if x is None else spec % x


def summary_line(name, r):
    w, t = r["window"], r["total"]
    return "%-8s crashes / 12 s %.4f   gates / 12 s %7.3f   first lap %s s   flying lap %s s   (laps counted %s)" % (
        name, w["crashes_per_window"], w["gates_per_window"], fmt(t["first_lap_seconds"]), fmt(t["flying_lap_seconds"]), t["laps_counted"][:6])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--load", required=True, help="checkpoint written by model.save")
    ap.add_argument("--generations", type=int, required=True)
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--envs-per-policy", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--save", default="")
    ap.add_argument("--variant", choices=("e2e", "indi"), default="e2e")
    ap.add_argument("--track", choices=("square", "zigzag"), default="square")
    ap.add_argument("--gates-ahead", type=int, default=1)
    ap.add_argument("--n-eval-steps", type=int, default=1200)
    ap.add_argument("--eval-seeds", choices=("fixed", "per_generation"), default="fixed")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch
    from optimal_quad_control_rl_amd import (EvolutionStrategy, PPO, Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES, evaluate_policy,
                                             square_track, zigzag_track)

    trk = square_track() if a.track == "square" else zigzag_track()
    cls = Quadcopter3DGates if a.variant == "e2e" else Quadcopter3DGatesINDI

    def make(n, seed):
        env = cls(n, *trk, gates_ahead=a.gates_ahead, infos_mode="none", seed=seed)
        if a.variant == "e2e":
            env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        env.max_steps = 10 ** 6
        return env

    model = PPO.load(a.load)
    env, ev = make(2 * a.pairs * a.envs_per_policy, a.seed), make(4096, 99)
    before = evaluate_policy(model, ev, n_eval_steps=2000, window_steps=1200, seed=99)
    es = EvolutionStrategy(env, model, pairs=a.pairs, envs_per_policy=a.envs_per_policy, sigma=a.sigma, lr=a.lr, n_eval_steps=a.n_eval_steps,
                           seed=a.seed, eval_seeds=a.eval_seeds)
    print("ES: %d members x %d envs, %d steps per generation, sigma %g, lr %g, fitness 'lap' %s, %s evaluation seeds"
          % (es.P, es.E, es.n_eval_steps, es.sigma, es.lr, es.weights, a.eval_seeds), flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()

    def line(es, s):
        print("gen %4d  score best %10.3f mean %10.3f worst %10.3f   best member %3d: flying lap %s s, crashes / env %.4f"
              % (s["generation"], s["best"], s["mean"], s["worst"], s["best_member"], fmt(s["best_flying_lap_seconds"]), s["best_crashes_per_env"]),
              flush=True)

    es.learn(a.generations, callback=line)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    es.write_back(model)
    after = evaluate_policy(model, ev, n_eval_steps=2000, window_steps=1200, seed=99)
    print("%d generations in %.2f s (%.1f ms per generation, host read and this log included)" % (a.generations, seconds, 1e3 * seconds / max(1, a.generations)))
    print("evaluate_policy on 4096 fresh envs, seed 99, 2000 steps (rates over the first 1200):")
    print(summary_line("start", before))
    print(summary_line("result", after))
    if a.save:
        print("saved", model.save(a.save))
    es.close()


if __name__ == "__main__":
    main()
