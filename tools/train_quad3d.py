#!/usr/bin/env python3
"""PPO on the predecessor envs of the reference's "3D quad.ipynb", on the device (GPU box).

    python tools/train_quad3d.py --env hover|gates [--envs 100] [--n-steps N] [--rollouts 40] [--log-every 5] [--seed 0]
        [--precision f16-operands|f32|f32-collect] [--save PATH]

Defaults are the notebook's recipe (Q3 cell 10 / cell 19): 100 envs, n_steps 500 (hover) / 1000 (gates), batch_size 5000, 10 epochs,
3 x 120 ReLU networks for policy and value, log_std_init 0, everything else SB3's default (gamma 0.99, lr 3e-4, GAE 0.95, clip 0.2).
The gates env flies the notebook's track (cell 16: the four-gate figure listed twice, start at (-4, -2, -1.5)).
Not reproduced: the notebook appends a Tanh to SB3's action net after construction; the networks here are the plain MlpPolicy.

Every --log-every rollouts it prints the mean episode reward and length over the episodes that finished in those rollouts.  Collection
is one closed-loop kernel per rollout (q3_rollout_policy), the update runs in the matrix-core PPO kernels."""
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


def main():
    import torch
    from optimal_quad_control_rl_amd import PPO, VecMonitor
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
    a = ap.parse_args()
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
    if a.save:
        print("saved", model.save(a.save))


if __name__ == "__main__":
    main()
