#!/usr/bin/env python3
"""Record the flights of a trained policy on the device (record_policy -> qr_record_policy: one kernel launch) and write them in the
reference's log format.

    python tools/record_flight.py CHECKPOINT [--variant e2e|indi] [--track square|zigzag] [--envs 16] [--steps 2000] [--stochastic]
                                  [--seed 99] [--npz flight.npz] [--env-index 0] [--episode N] [--out record.npz]
                                  [--obs-noise SIGMA[,...8]] [--delay D] [--vehicle PARAM=SCALE] [--scale S]

CHECKPOINT is what sb3.PPO.save or tools/train_ppo.py --save wrote.  The eval env is the one of tools/train_ppo.py (gates_ahead 1,
training disturbance ranges for E2E, no time limit to speak of).  Per env and episode one line: gates passed, how the episode ended,
lap times from the rows.  --npz: env --env-index (one episode with --episode) with the keys of the reference's logging cell (t x y z vx
vy vz V phi theta psi u1..u4 u), so it opens in the reference's analysis cells; --out: the whole record (rows [K][M][R], dt,
final_target).  A row pairs the state with the command applied IN that state (the reference's cell pairs the state after the step).

--obs-noise / --delay / --vehicle, or a checkpoint trained with --command-history H (read off its input length): the flight is ONE CELL of
the sensing-grid evaluator (record_grid -> qr_blackbox_policy_grid with a ring as long as the flight), as in tools/crash_report.py: the first
--envs envs of a 256-env cell under that sensor, vehicle and command history, deterministic actions; rows hold the TRUE state and the command
FLOWN.  --scale: the disturbance scale (E2E).  Without any of these the call is record_policy's as before."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimal_quad_control_rl_amd import (PPO, Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES, record_policy, square_track,  # noqa: E402
                                         zigzag_track)
from optimal_quad_control_rl_amd.evaluation import default_gates_per_lap  # noqa: E402
from crash_report import add_cell_options, cell_lines, grid_cell  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("checkpoint")
ap.add_argument("--variant", default="indi", choices=("e2e", "indi"))
ap.add_argument("--track", default="square", choices=("square", "zigzag"))
ap.add_argument("--envs", type=int, default=16)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--stochastic", action="store_true", help="sample actions with the checkpoint's log_std instead of flying the mean")
ap.add_argument("--seed", type=int, default=99)
ap.add_argument("--max-steps", type=int, default=10 ** 6, help="the env's time limit")
ap.add_argument("--npz", default="flight.npz", help="reference-format log of one env ('' = none)")
ap.add_argument("--env-index", type=int, default=0)
ap.add_argument("--episode", type=int, default=None)
ap.add_argument("--out", default="", help="the whole record: rows, dt, final_target")
ap.add_argument("--scale", type=float, default=None, help="disturbance scale (E2E): the training ranges times this")
add_cell_options(ap)
a = ap.parse_args()
a.gates_ahead = 1

trk = square_track() if a.track == "square" else zigzag_track()
cls = Quadcopter3DGates if a.variant == "e2e" else Quadcopter3DGatesINDI
env = cls(a.envs, *trk, gates_ahead=1, infos_mode="none", seed=a.seed)
if a.variant == "e2e":
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
env.max_steps = a.max_steps
if a.variant == "e2e" and a.scale is not None:
    env.disturbance_scale = a.scale
model = PPO.load(a.checkpoint)
cell = grid_cell(a, env, model)
if cell is None:
    rec = record_policy(model, env, a.steps, deterministic=not a.stochastic, seed=a.seed)
else:
    from optimal_quad_control_rl_amd import record_grid

    if not 1 <= a.envs <= 256:
        raise SystemExit("--envs must be in 1..256 for a cell of the sensing-grid evaluator (the first envs of one 256-env cell are recorded)")
    env.close()
    env = cls(256, *trk, gates_ahead=1, infos_mode="none", seed=a.seed)
    if a.variant == "e2e":
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        if a.scale is not None:
            env.disturbance_scale = a.scale
    env.max_steps = a.max_steps
    cell = grid_cell(a, env, model)
    rec = record_grid([model], [cell["condition"]], [cell["sensor"]], env, dynamics=cell["dynamics"], envs_per_cell=256, n_steps=a.steps,
                      rec_per_cell=a.envs, seed=a.seed, noise_seed=a.seed, command_history=cell["command_history"])[0][0][0]
    for line in cell_lines(cell, rec.evaluation):
        print(line)
gpl, dt = default_gates_per_lap(env), float(rec.dt)
ends = {0.0: "still flying", 1.0: "crash", 2.0: "time limit"}
for i in range(rec.num_envs):
    passes = rec.gate_passes(i)
    for e, (lo, hi) in enumerate(rec.episodes(i)):
        p = passes[(passes >= lo) & (passes < hi)]
        laps = np.diff(np.concatenate([[lo - 1], p])[::gpl]) * dt      # every gates_per_lap-th passage time, differenced (FP:261-289)
        print("env %d episode %d: rows %d..%d (%.2f s), %d gates, %s, laps [%s] s"
              % (i, e, lo, hi, (hi - lo) * dt, p.size, ends[float(rec.end[hi - 1, i])], ", ".join("%.2f" % x for x in laps)))
c = rec.counts().sum(axis=0)
print("total: %d envs x %d steps, %d gates, %d crashes, %d time-limit ends" % (rec.num_envs, rec.num_steps, c[0], c[1], c[2]))
if a.npz:
    print("wrote", rec.save_npz(a.npz, a.env_index, a.episode))
if a.out:
    extra = {} if rec.final_target is None else dict(final_target=rec.final_target)   # (a cell's record carries no final target)
    np.savez(a.out, rows=rec.rows, dt=rec.dt, **extra)
    print("wrote", a.out)
env.close()
