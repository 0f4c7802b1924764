#!/usr/bin/env python3
"""PPO on the predecessor envs of the reference's "3D quad.ipynb", on the device (GPU box).

    python tools/train_quad3d.py --env hover|gates [--envs 100] [--n-steps N] [--rollouts 40] [--log-every 5] [--seed 0]
        [--precision f16-operands|f32|f32-collect] [--save PATH] [--eval-final [STEPS]] [--eval-envs 4096] [--curve R]

Defaults are the notebook's recipe (Q3 cell 10 / cell 19): 100 envs, n_steps 500 (hover) / 1000 (gates), batch_size 5000, 10 epochs,
3 x 120 ReLU networks for policy and value, log_std_init 0, everything else SB3's default (gamma 0.99, lr 3e-4, GAE 0.95, clip 0.2).
The gates env flies the notebook's track (cell 16: the four-gate figure listed twice, start at (-4, -2, -1.5)).
Not reproduced: the notebook appends a Tanh to SB3's action net after construction; the networks here are the plain MlpPolicy.

Every --log-every rollouts it prints the mean episode reward and length over the episodes that finished in those rollouts.  Collection
is one closed-loop kernel per rollout (q3_rollout_policy), the update runs in the matrix-core PPO kernels.

--eval-final flies the final policy deterministically on a fresh env of the same kind (--eval-envs envs, STEPS steps each, default 2000)
in one kernel (q3_evaluate_policy) and prints how its episodes ended.  --curve R keeps a copy of the actor every R rollouts and, after
training, evaluates all copies on the same starts, 16 per launch at the default --eval-envs (q3_evaluate_policy_bank): one row per copy."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def notebook_track():
    """Q3 cell 16 (data)."""
    gate_pos = np.array([[-1.5, -2, -1.5], [1.5, 2, -1.5], [1.5, -2, -1.5], [-1.5, 2, -1.5]] * 2, dtype=np.float64)
    gate_yaw = np.array([0, 0, np.pi, np.pi] * 2)
    start_pos = np.array([-4, -2, -1.5], dtype=np.float64)
    return gate_pos, gate_yaw, start_pos


def _pct(k, n):
    return "%5.1f %%" % (100.0 * k / n) if n else "    - %"


def _sec(x):
    return "%6.2f s" % x if x is not None else "      - "


def print_outcomes(title, s, gates=False):
    """The outcome table of one evaluation summary (evaluation.summarize_q3_eval)."""
    n = s["episodes"]
    print(title)
    print("  envs %d  steps per env %d  episodes ended %d" % (s["envs"], s["steps"], n))
    for label, key in (("success", "successes"), ("time limit", "timeouts"), ("out of bounds", "out_of_bounds"), ("ground", "ground"),
                       ("gate collision", "collisions")):
        print("  %-15s %8d  %s" % (label, s[key], _pct(s[key], n)))
    print("  time to success: mean %s  best %s    mean episode %s" % (_sec(s["mean_success_seconds"]), _sec(s["best_success_seconds"]),
                                                                     _sec(s["mean_episode_seconds"])))
    if gates and s["gates_per_episode"] is not None:
        print("  gates passed per episode %.2f" % s["gates_per_episode"])
    if s["mean_reward"] is not None:
        print("  episode return: mean %.3f  std %.3f" % (s["mean_reward"], s["std_reward"]), flush=True)


def print_curve(rollouts, summaries):
    print("rollout   episodes   success   time to success   crashed   time limit")
    for r, s in zip(rollouts, summaries):
        n = s["episodes"]
        crashed = s["out_of_bounds"] + s["ground"] + s["collisions"]
        print("%7d  %9d  %s    %s        %s    %s" % (r, n, _pct(s["successes"], n), _sec(s["mean_success_seconds"]), _pct(crashed, n),
                                                       _pct(s["timeouts"], n)), flush=True)


def main():
    import copy

    import torch
    from optimal_quad_control_rl_amd import PPO, VecMonitor, evaluate_q3_policies, evaluate_q3_policy
    from optimal_quad_control_rl_amd.evaluation import _actor, _model_precision
    from optimal_quad_control_rl_amd.quad3d import Quadcopter3DVec, Quadcopter3DVecGates

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--env", choices=("hover", "gates"), required=True)
    ap.add_argument("--envs", type=int, default=100)
    ap.add_argument("--n-steps", type=int, default=None, help="default: 500 (hover) / 1000 (gates)")
    ap.add_argument("--batch-size", type=int, default=5000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--rollouts", type=int, default=40, help="rollouts to train for")
    ap.add_argument("--log-every", type=int, default=5, help="print the episode statistics every N rollouts")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", choices=("f16-operands", "f32", "f32-collect"), default="f16-operands")
    ap.add_argument("--save", default=None, help="write the final model here (SB3-shaped zip)")
    ap.add_argument("--eval-final", type=int, nargs="?", const=2000, default=None, metavar="STEPS",
                    help="after training, fly the final policy deterministically for STEPS steps (default 2000) and print how its episodes ended")
    ap.add_argument("--eval-envs", type=int, default=4096, help="envs of the evaluation env (a multiple of 256 for --curve)")
    ap.add_argument("--curve", type=int, default=None, metavar="R", help="keep the actor every R rollouts; evaluate all copies after training")
    a = ap.parse_args()
    if a.curve is not None and (a.curve < 1 or a.eval_envs % 256 != 0):
        ap.error("--curve needs R >= 1 and --eval-envs a multiple of 256")
    n_steps = a.n_steps or (500 if a.env == "hover" else 1000)
    core = Quadcopter3DVec(a.envs, seed=a.seed) if a.env == "hover" else Quadcopter3DVecGates(a.envs, *notebook_track(), seed=a.seed)
    env = VecMonitor(core)
    pk = dict(activation_fn=torch.nn.ReLU, net_arch=[dict(pi=[120, 120, 120], vf=[120, 120, 120])], log_std_init=0)
    model = PPO("MlpPolicy", env, policy_kwargs=pk, verbose=0, n_steps=n_steps, batch_size=a.batch_size, n_epochs=a.epochs, seed=a.seed,
                precision=a.precision)
    tr = model._trainer
    print("env %s  envs %d  n_steps %d  batch_size %d  epochs %d  seed %d  precision %s  fused_collect %s  native_update %s"
          % (a.env, a.envs, n_steps, a.batch_size, a.epochs, a.seed, a.precision, tr.fused_collect, tr.native_update), flush=True)
    acc = dict(ret=0.0, len=0.0, n=0.0)
    kept = []     # --curve: (rollout, copy of the actor)

    def after_rollout(trainer):
        s = trainer.stats
        if s.get("episodes", 0):
            acc["ret"] += s["ep_rew_mean"] * s["episodes"]; acc["len"] += s["ep_len_mean"] * s["episodes"]; acc["n"] += s["episodes"]
        return True

    t0 = time.perf_counter()
    per_rollout = a.envs * n_steps
    for r in range(1, a.rollouts + 1):
        tr.stats.pop("episodes", None)           # only the episodes that finish in this rollout count
        model.learn(total_timesteps=per_rollout, reset_num_timesteps=False, callback=after_rollout)
        if r % a.log_every == 0 or r == a.rollouts:
            torch.cuda.synchronize()
            n = acc["n"]
            print("rollout %4d  steps %9d  episodes %6d  ep_rew_mean %10.3f  ep_len_mean %8.1f  std %.3f  %.1f s"
                  % (r, model.num_timesteps, int(n), acc["ret"] / n if n else float("nan"), acc["len"] / n if n else float("nan"),
                     tr.stats.get("std", float("nan")), time.perf_counter() - t0), flush=True)
            acc.update(ret=0.0, len=0.0, n=0.0)
        if a.curve and (r % a.curve == 0 or r == a.rollouts):
            kept.append((r, copy.deepcopy(_actor(model))))
    if a.save:
        print("saved", model.save(a.save))
    if a.eval_final is not None or a.curve:
        steps, eval_seed = a.eval_final or 2000, a.seed + 1000
        ev = Quadcopter3DVec(a.eval_envs, seed=eval_seed) if a.env == "hover" else Quadcopter3DVecGates(a.eval_envs, *notebook_track(), seed=eval_seed)
        if a.eval_final is not None:
            print_outcomes("final policy, deterministic, on a fresh %s env (seed %d):" % (a.env, eval_seed),
                           evaluate_q3_policy(model, ev, n_eval_steps=steps, seed=eval_seed), gates=a.env == "gates")
        if a.curve:
            print("learning curve after the fact: %d copies of the actor, each on the same 256 starts, %d steps per env, %d per launch"
                  % (len(kept), steps, a.eval_envs // 256))
            print_curve([r for r, _ in kept], evaluate_q3_policies([p for _, p in kept], ev, envs_per_policy=256, n_eval_steps=steps,
                                                                  precision=_model_precision([model]), seed=eval_seed))


if __name__ == "__main__":
    main()
