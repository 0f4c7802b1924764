#!/usr/bin/env python3
"""What a population buys, measured (GPU box; DESIGN section 8, profiles/r14_population.txt):

    python tools/bench_population.py [out.json]

1. one PopulationPPO round (P = 10 members x E = 256 envs, E2E + residual MLPs, the reference recipe's shape: n_steps 1000, 10 epochs,
   20 minibatches, native update) split into bank load, collect call, launch, slice copies + values, updates;
2. ten standalone rounds: ten 256-env handles, ten ppo.PPO, ten collect launches (the path without a population);
3. the launch alone at N = 65 536 = 256 groups x 256, K = 64, us per step, both forwards: 256 distinct bank slots, every group on ONE slot,
   and qr_rollout_policy_conditions on the same handle (is a ratio the kernel or the distinct weight images?).
Medians after a warm-up; the raw rows are in the JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimal_quad_control_rl_amd import PopulationPPO, Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
from optimal_quad_control_rl_amd.conditions import Condition, ConditionBank
from optimal_quad_control_rl_amd.policy import MfmaPolicy, MfmaPolicyBank
from optimal_quad_control_rl_amd.ppo import PPO, ActorCritic

P, E, T = 10, 256, 1000
HYPER = dict(n_steps=T, n_epochs=10, batch_size=E * T // 20, gamma=0.999, native_update=True)
ROUNDS = 4   # the first is a warm-up (graph capture, allocations)


def make_env(n, base=0):
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=1, env_id_base=base)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    return env


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


res = {}
# ---- population round
env = make_env(P * E)
pop = PopulationPPO(env, [dict(seed=s) for s in range(P)], envs_per_member=E, **HYPER)
rows = []
for r in range(ROUNDS):
    t0 = sync()
    pop.load_bank()
    t1 = sync()
    pop.collect()            # loads the bank again (as a round does) and launches
    t2 = sync()
    launch_ms = env.last_rollout_ms()
    t_values = t_update = 0.0
    for m in pop.members:
        a = sync()
        m.collect_fused()    # slice copies, the member's own MfmaPolicy load, values
        b = sync()
        m.train()
        c = sync()
        t_values += b - a
        t_update += c - b
    pop._launch = None
    if r:
        rows.append(dict(bank_load_ms=(t1 - t0) * 1e3, collect_call_ms=(t2 - t1) * 1e3, launch_ms=launch_ms, slices_values_ms=t_values * 1e3,
                         updates_ms=t_update * 1e3, round_ms=((t2 - t1) + t_values + t_update) * 1e3))
res["population_round"] = {k: statistics.median(x[k] for x in rows) for k in rows[0]}
res["population_rounds_raw"] = rows
pop.close(); env.close()
print(json.dumps(res["population_round"]), flush=True)

# ---- ten standalone rounds
solos = []
for p in range(P):
    e = make_env(E, base=p * E)
    solos.append((e, PPO(e, seed=p, fused_collect=True, **HYPER)))
rows = []
for r in range(ROUNDS):
    t_collect = t_update = launch = 0.0
    for e, m in solos:
        a = sync()
        m.collect()
        b = sync()
        launch += e.last_rollout_ms()
        m.train()
        c = sync()
        t_collect += b - a
        t_update += c - b
    if r:
        rows.append(dict(collect_ms=t_collect * 1e3, launches_ms=launch, updates_ms=t_update * 1e3, round_ms=(t_collect + t_update) * 1e3))
res["ten_standalone_rounds"] = {k: statistics.median(x[k] for x in rows) for k in rows[0]}
res["ten_standalone_rounds_raw"] = rows
for e, m in solos:
    e.close()
print(json.dumps(res["ten_standalone_rounds"]), flush=True)

# ---- launch level, N = 65 536: distinct slots against one slot in every group, both precisions
n, Kc = 65536, 64
G = n // E
env = make_env(n)
cbank = ConditionBank(0, 1)
cbank.set(0, Condition.from_env(env))
pbank, pol = MfmaPolicyBank(env.state_len, G), MfmaPolicy(env.state_len)
for slot in range(G):
    torch.manual_seed(slot)
    actor = ActorCritic(env.state_len, 4).pi
    pbank.load_torch(slot, actor)
    if slot == 0:
        pol.load_torch(actor)
dev = env.device
out = (torch.empty((Kc, n, env.state_len), device=dev), torch.empty((Kc, n, 4), device=dev), torch.empty((Kc, n), device=dev),
       torch.empty((Kc, n), device=dev), torch.empty((Kc, n), dtype=torch.uint8, device=dev), torch.empty((Kc, n), dtype=torch.uint8, device=dev))
ls1, lsg, seeds, cog = np.zeros(4, np.float32), np.zeros((G, 4), np.float32), list(range(1, G + 1)), [0] * G
launch = {}
for precision in ("f16-operands", "f32"):
    t = dict(distinct=[], one_slot=[], conditions=[])
    for rep in range(10):
        for name in t:
            env.seed(99); env.reset_device()
            if name == "conditions":
                env.rollout_policy_conditions_device(pol, cbank, cog, E, Kc, ls1, noise_seed=1, out=out, precision=precision)
            else:
                env.rollout_policy_population_device(pbank, list(range(G)) if name == "distinct" else [0] * G, cbank, cog, E, Kc, lsg, seeds,
                                                     out=out, precision=precision)
            if rep:
                t[name].append(env.last_rollout_ms() * 1e3 / Kc)
    launch[precision] = {k: statistics.median(v) for k, v in t.items()}
    launch[precision]["raw"] = t
res["launch_us_per_step"] = launch
print(json.dumps({p: {k: v for k, v in d.items() if k != "raw"} for p, d in launch.items()}), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
