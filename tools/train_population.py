#!/usr/bin/env python3
"""P seeds of one PPO recipe, trained side by side on ONE env with ONE collect launch per round (PopulationPPO ->
qr_rollout_policy_population), ranked on shared starts (GPU box).

    python tools/train_population.py --seeds 0-9 [--envs-per-member 256] [--variant indi|e2e] [--track square|zigzag]
        [--steps 3e6] [--n-steps 32] [--epochs 5] [--minibatches 4] [--lr 3e-4] [--target-kl 0.02] [--curve 20] [--batched-update [--batched-prepare]]
        [--pbt-interval R [--pbt-quantile 0.25] [--pbt-fitness ep_rew_mean|gates|eval] [--pbt-perturb-lr 0.8,1.25] [--pbt-log-std-shift s]]

--steps counts env steps PER MEMBER.  Member p owns envs [p E, (p + 1) E) of a P x E env and differs from the others in its seed only
(network initialisation, minibatch permutations, action noise); the env's own seed is 1, as for tools/train_ppo.py --seed 0.  Every
--curve rounds (training clock stopped) and at the end all members are evaluated in one bank launch on shared starts
(evaluate_policies): one line per member, then the rank_policies table.  --batched-update: the members' updates run as one launch
sequence (PopulationPPO(batched_update=True) -> qr_ppo_population_epoch) instead of one after another; same results, bit for bit.  --batched-prepare (needs --batched-update, implies nothing else): the bank
load, the members' value forwards, slice copies, sanitising and GAE run on the device for all members at once
(PopulationPPO(batched_prepare=True) -> qr_ppo_population_load_bank / qr_ppo_population_prepare); same tensors, bit for bit.  The JSON
line carries round_ms, the mean wall time of a round (collect + train) after the first one (which captures graphs and allocates).
--pbt-interval R: population-based training (PopulationPPO(pbt=PBT(...))): every R rounds the worst --pbt-quantile of the members are
overwritten by copies of the best, their learning rate multiplied by one of --pbt-perturb-lr and their log_std moved by +- --pbt-log-std-shift;
the fitness is a training statistic (ep_rew_mean, gates = gates per episode) or eval = gates per 12 s of the bank evaluation above (training
clock stopped).  The lineage goes into the JSON line.  Without --pbt-interval nothing changes."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_seeds(text):
    """"0-9" -> [0..9]; "3,5,8-10" -> [3, 5, 8, 9, 10]"""
    seeds = []
    for part in text.split(","):
        try:
            lo, hi = (int(x) for x in (part.split("-", 1) if "-" in part else (part, part)))
        except ValueError:
            raise SystemExit("--seeds takes numbers and ranges, e.g. 0-9 or 3,5,8-10 (got %r)" % text)
        if hi < lo:
            raise SystemExit("--seeds: the range %r runs backwards" % part)
        seeds += list(range(lo, hi + 1))
    return seeds


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seeds", default="0-9", help="the members' seeds: numbers and ranges, e.g. 0-9 or 3,5,8-10")
    ap.add_argument("--envs-per-member", type=int, default=256, help="envs each member collects from (a multiple of 256)")
    ap.add_argument("--variant", default="indi")
    ap.add_argument("--track", default="square")
    ap.add_argument("--steps", type=float, default=3e6, help="env steps per member")
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--target-kl", type=float, default=0.02)
    ap.add_argument("--lr-final", type=float, default=0.1)
    ap.add_argument("--ent-coef", type=float, default=0.0)
    ap.add_argument("--gamma", type=float, default=0.999)
    ap.add_argument("--precision", default="f16-operands", choices=("f16-operands", "f32-collect", "f32"))
    ap.add_argument("--no-trunc-bootstrap", action="store_true")
    ap.add_argument("--torch-update", action="store_true", help="update with torch autograd instead of the matrix-core kernels")
    ap.add_argument("--batched-update", action="store_true", help="update all members in one launch sequence (matrix-core update, f16 operands)")
    ap.add_argument("--batched-prepare", action="store_true",
                    help="bank load, values, sanitising and GAE of all members on the device in a fixed number of launches (needs --batched-update)")
    ap.add_argument("--pbt-interval", type=int, default=0, help="population-based training: rounds between decisions (0: off)")
    ap.add_argument("--pbt-quantile", type=float, default=0.25, help="share of the members replaced (and copied from) per decision, at most 0.5")
    ap.add_argument("--pbt-fitness", default="ep_rew_mean", choices=("ep_rew_mean", "gates", "eval"))
    ap.add_argument("--pbt-perturb-lr", default="", help="two factors, e.g. 0.8,1.25: a copy's learning rate is multiplied by one of them")
    ap.add_argument("--pbt-log-std-shift", type=float, default=0.0, help="a copy's log_std is its source's plus or minus this")
    ap.add_argument("--curve", type=int, default=0, help="evaluate every member every this many rounds (training clock stopped)")
    ap.add_argument("--eval-envs-per-member", type=int, default=256)
    ap.add_argument("--out", default="")
    return ap


def fmt(x, spec="%.3f"):
    return "   -  " if x is None else spec % x


def member_line(seed, r):
    w, t = r["window"], r["total"]
    return "seed %4d  gates/12s %6.2f  crashes/12s %6.3f  lap1 %s  flying lap %s" % (
        seed, w["gates_per_window"], w["crashes_per_window"], fmt(t["first_lap_seconds"]), fmt(t["flying_lap_seconds"]))


def main():
    import torch
    from optimal_quad_control_rl_amd import (PopulationPPO, Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES, evaluate_policies,
                                             rank_policies, square_track, zigzag_track)

    ap = parser()
    a = ap.parse_args()
    if a.batched_prepare and not a.batched_update:
        ap.error("--batched-prepare needs --batched-update")
    seeds = parse_seeds(a.seeds)
    P, E = len(seeds), a.envs_per_member
    trk = square_track() if a.track == "square" else zigzag_track()
    cls = Quadcopter3DGates if a.variant == "e2e" else Quadcopter3DGatesINDI

    def make_env(n, seed):
        env = cls(n, *trk, gates_ahead=1, infos_mode="none", seed=seed)
        if a.variant == "e2e":
            env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
        return env

    env = make_env(P * E, 1)
    paused, pbt = [0.0], None
    if a.pbt_interval:
        from optimal_quad_control_rl_amd.population import PBT

        def eval_fitness(p):   # gates per 12 s on the shared starts of the bank evaluation; the training clock does not run
            torch.cuda.synchronize()
            e0 = time.perf_counter()
            fit = [r["window"]["gates_per_window"] for r in evaluate()]
            torch.cuda.synchronize()
            paused[0] += time.perf_counter() - e0
            return fit

        try:
            factors = tuple(float(x) for x in a.pbt_perturb_lr.split(",")) if a.pbt_perturb_lr else None
            pbt = PBT(interval=a.pbt_interval, quantile=a.pbt_quantile,
                      fitness={"ep_rew_mean": "ep_rew_mean", "gates": "gates_per_episode", "eval": eval_fitness}[a.pbt_fitness],
                      perturb={"learning_rate": factors} if factors else None, log_std_shift=a.pbt_log_std_shift)
        except ValueError as e:
            ap.error("--pbt-*: %s" % e)
    pop = PopulationPPO(env, [dict(seed=s) for s in seeds], envs_per_member=E, ent_coef=a.ent_coef, gamma=a.gamma, n_steps=a.n_steps,
                        n_epochs=a.epochs, batch_size=E * a.n_steps // a.minibatches, learning_rate=a.lr, target_kl=a.target_kl,
                        lr_final_frac=a.lr_final, total_timesteps_hint=int(a.steps), native_update=not a.torch_update,
                        truncation_bootstrap=not a.no_trunc_bootstrap, policy_forward="f32class" if a.precision != "f16-operands" else "torch",
                        update_precision="f32" if a.precision == "f32" else "f16-operands", batched_update=a.batched_update,
                        batched_prepare=a.batched_prepare, pbt=pbt)
    # evaluation on a separate env, every member on the same starts: 2000 steps = 20 s of flight, crashes restart the lap count
    ev = make_env(P * a.eval_envs_per_member, 99)
    ev.max_steps = 10 ** 6

    def evaluate():
        return evaluate_policies(pop.members, ev, envs_per_policy=a.eval_envs_per_member, n_eval_steps=2000, window_steps=1200, seed=99)

    curve, rounds, first = [], [0], [0.0]

    def on_round(p):
        rounds[0] += 1
        if rounds[0] == 1:
            torch.cuda.synchronize()
            first[0] = time.perf_counter() - t0
        if rounds[0] % 20 == 0:
            gates = ["%5.2f" % m.stats.get("gates_per_episode", float("nan")) for m in p.members]
            print("round %4d  steps/member %7.2fM  gates/ep by member: %s" % (rounds[0], p.num_timesteps / 1e6, " ".join(gates)), flush=True)
        if a.curve and rounds[0] % a.curve == 0:
            torch.cuda.synchronize()
            e0 = time.perf_counter()
            tsec = e0 - t0 - paused[0]
            res = evaluate()
            torch.cuda.synchronize()
            paused[0] += time.perf_counter() - e0
            print("-- round %d, %.1f s of training" % (rounds[0], tsec), flush=True)
            for s, r in zip(seeds, res):
                print(member_line(s, r), flush=True)
            curve.append(dict(round=rounds[0], train_seconds=tsec, env_steps_per_member=p.num_timesteps,
                              flying_lap=[r["total"]["flying_lap_seconds"] for r in res],
                              crashes_per_12s=[r["window"]["crashes_per_window"] for r in res]))

    decision_ms = []
    if pbt is not None:   # a decision's own wall time (exploit launch + host bookkeeping; an "eval" fitness is on the paused clock)
        step = pop.pbt_step

        def timed_step():
            torch.cuda.synchronize()
            d0, p0 = time.perf_counter(), paused[0]
            entries = step()
            torch.cuda.synchronize()
            decision_ms.append(1e3 * (time.perf_counter() - d0 - (paused[0] - p0)))
            return entries

        pop.pbt_step = timed_step
    t0 = time.perf_counter()
    pop.learn(int(a.steps), callback=on_round)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0 - paused[0]
    res = evaluate()
    order = rank_policies(res)
    print("rank  " + "-" * 70)
    for place, i in enumerate(order):
        print("%3d   %s" % (place + 1, member_line(seeds[i], res[i])), flush=True)
    out = dict(seeds=seeds, envs_per_member=E, variant=a.variant, track=a.track, n_steps=a.n_steps, epochs=a.epochs, minibatches=a.minibatches,
               lr=a.lr, target_kl=a.target_kl, batched_update=bool(a.batched_update), batched_prepare=bool(a.batched_prepare), rounds=rounds[0], round_ms=1e3 * (train_s - first[0]) / (rounds[0] - 1) if rounds[0] > 1 else None, train_steps_per_member=pop.num_timesteps, train_seconds=train_s,
               train_Msteps_per_s=pop.num_timesteps * P / train_s / 1e6, ranking=[seeds[i] for i in order],
               flying_lap_seconds=[r["total"]["flying_lap_seconds"] for r in res],
               crashes_per_12s=[r["window"]["crashes_per_window"] for r in res], curve=curve)
    if pbt is not None:
        out["pbt"] = dict(interval=a.pbt_interval, quantile=a.pbt_quantile, fitness=a.pbt_fitness, perturb_lr=a.pbt_perturb_lr,
                          log_std_shift=a.pbt_log_std_shift, decisions=len(decision_ms),
                          decision_ms=sum(decision_ms) / len(decision_ms) if decision_ms else None)
        out["lineage"] = [dict(round=r, dst=seeds[d], src=seeds[s], fitness=list(f), hyper=h) for r, d, s, f, h in pop.lineage]
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
