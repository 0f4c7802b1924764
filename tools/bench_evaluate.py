#!/usr/bin/env python3
"""Time of the on-device evaluator (qr_evaluate_policy) against (a) the closed-loop rollout kernel it is a subset of
(qr_rollout_policy, deterministic) and (b) the per-step Python evaluation loop of tools/reference_recipe_run.py.  GPU box.

    python tools/bench_evaluate.py [--steps 2000] [--reps 5] [--out profiles/r08_evaluate.txt]

(a) E2E + residual MLPs + training disturbances, square track, gates_ahead 1, f16 operands, N = 65 536 and 4 096: the two kernels
    ALTERNATE on one box from the same seeded start with the same (untrained, seeded) policy, `reps` times each after one warm-up
    pair; the time of a launch is the hipEvent bracket of qr_last_step_many_ms; medians are compared.
(b) wall time (host clock around work that ends in a synchronise) of one full evaluation, 4 096 envs x `steps`: evaluate_policy
    (two launches + two small copies; the time INCLUDES what evaluate_policy does per call and the loop leg does not: creating an
    MfmaPolicy, loading the actor's weights into it, reseeding) and the tools' loop (policy launch, step launch, ~20 small torch ops
    and a host synchronisation per step).  tools_loop() below is a COPY of evaluate() of tools/reference_recipe_run.py -- that tool
    trains for 1e9 steps before it evaluates, so it cannot be timed itself; tests/test_eval_host.py compares the two loop bodies
    line by line so that the copy cannot drift."""
import argparse, json, os, statistics, subprocess, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, evaluate_policy, square_track
from optimal_quad_control_rl_amd.policy import MfmaPolicy
from optimal_quad_control_rl_amd.ppo import PPO

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--commit", default="", help="commit to name in the output when the tree that runs has no git metadata")
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


trk = square_track()
K = a.steps
try:
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True,
                                     cwd=os.path.dirname(os.path.abspath(__file__))).strip()
except Exception:
    commit = "working tree (no git metadata on the box)"
say("# tools/bench_evaluate.py --steps %d --reps %d" % (K, a.reps))
say("# commit %s; device %s; host %s; torch %s" % (commit, torch.cuda.get_device_name(0), os.uname().nodename, torch.__version__))


def make(n):
    env = Quadcopter3DGates(n, *trk, gates_ahead=1, infos_mode="none", seed=99)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = 10 ** 6
    return env


small = make(256)
model = PPO(small, seed=0, n_steps=8, batch_size=256, n_epochs=1)   # an untrained, seeded actor: the same network for every leg
result = {}
for n in (65536, 4096):
    env = make(n)
    pol = MfmaPolicy(env.state_len).load_torch(model.policy.pi)
    rec = torch.zeros((n, 24), dtype=torch.int32, device=env.device)
    recf = torch.zeros((n, 4), dtype=torch.float32, device=env.device)
    dev = env.device
    out = (torch.empty((K, n, env.state_len), device=dev), torch.empty((K, n, 4), device=dev), torch.empty((K, n), device=dev),
           torch.empty((K, n), device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev))
    t_eval, t_roll = [], []
    for rep in range(a.reps + 1):
        env.seed(99); env.reset_device(); rec.zero_(); recf.zero_()
        env.evaluate_device(pol, K, 4, rec, recf)
        ms_e = env.last_rollout_ms()
        env.seed(99); env.reset_device()
        env.rollout_policy_device(pol, K, torch.zeros(4), deterministic=True, out=out)
        ms_r = env.last_rollout_ms()
        if rep:   # rep 0 = warm-up pair
            t_eval.append(ms_e * 1e3 / K); t_roll.append(ms_r * 1e3 / K)
        say("n %6d rep %d%s  qr_evaluate_policy %.4f us/step   qr_rollout_policy %.4f us/step" % (n, rep, " (warm-up)" if not rep else "", ms_e * 1e3 / K, ms_r * 1e3 / K))
    me, mr = statistics.median(t_eval), statistics.median(t_roll)
    say("n %6d MEDIAN of %d  qr_evaluate_policy %.4f us/step   qr_rollout_policy %.4f us/step   ratio %.4f (requirement <= 1.03)   crashes %d gates %d" %
        (n, a.reps, me, mr, me / mr, int(rec[:, 1].sum()), int(rec[:, 0].sum())))
    result["n%d" % n] = dict(evaluate_us_per_step=me, rollout_us_per_step=mr, ratio=me / mr, runs_evaluate=t_eval, runs_rollout=t_roll)
    del out
    env.close(); pol.close()

# (b) one full evaluation, 4 096 envs
n_eval, G, dt = 4096, 4, 0.01
ev = make(n_eval)
tr = model


@torch.no_grad()
def tools_loop():
    """copy of evaluate() of tools/reference_recipe_run.py (kept equal by tests/test_eval_host.py)"""
    ev.seed(99)
    obs = ev.reset_device()
    dev = obs.device
    gates12 = torch.zeros(n_eval, device=dev); crashes12 = torch.zeros(n_eval, device=dev)
    passed = torch.zeros(n_eval, device=dev); lap_start = torch.zeros(n_eval, device=dev)
    lap_sum = torch.zeros(7, device=dev); lap_cnt = torch.zeros(7, device=dev)
    for k in range(K):
        obs, rew, done, trunc = ev.step_device(tr.act_device(obs).contiguous())
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
    return dict(gates_per_12s=float(gates12.mean()), crashes_per_12s=float(crashes12.mean()))


wall = {"evaluate_policy": [], "tools_loop": []}
for rep in range(4):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r_dev = evaluate_policy(model, ev, n_eval_steps=K, window_steps=min(1200, K), seed=99)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    r_loop = tools_loop()
    torch.cuda.synchronize(); t2 = time.perf_counter()
    if rep:
        wall["evaluate_policy"].append(t1 - t0); wall["tools_loop"].append(t2 - t1)
    say("full evaluation 4096 x %d rep %d%s  evaluate_policy %.4f s   tools loop %.4f s   (crashes/window %.4f vs %.4f, gates/window %.4f vs %.4f)" %
        (K, rep, " (warm-up)" if not rep else "", t1 - t0, t2 - t1, r_dev["window"]["crashes_per_window"], r_loop["crashes_per_12s"],
         r_dev["window"]["gates_per_window"], r_loop["gates_per_12s"]))
we, wl = statistics.median(wall["evaluate_policy"]), statistics.median(wall["tools_loop"])
say("full evaluation MEDIAN of 3  evaluate_policy %.4f s (incl. policy handle creation + weight load per call)   tools loop %.4f s (a copy of evaluate() of "
    "tools/reference_recipe_run.py)   (%.1f x)" % (we, wl, wl / we))
result["full_evaluation"] = dict(evaluate_policy_s=we, tools_loop_s=wl)
say(json.dumps(result))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
