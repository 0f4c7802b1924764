"""Evolution strategies on the policy bank (`qr_es_*`, csrc/quadrace_es.hip): optimise what the on-device evaluator MEASURES.

PPO climbs the shaped progress reward; what the user cares about afterwards -- flying-lap time and crash rate -- is counted in integers
by `qr_evaluate_policy_bank` and is not differentiable.  ES perturbs ONE actor parameter vector into P = 2 x pairs antithetic members
straight into bank slots, flies them in one launch on bit-identical starts, disturbances and restarts (common random numbers), scores
every member from its records, and turns the scores into an Adam ascent step with the noise regenerated on the device: a fixed number
of launches per generation whatever P is, and one small host read.

    from optimal_quad_control_rl_amd import EvolutionStrategy
    es = EvolutionStrategy(eval_env, model, pairs=128, envs_per_policy=256)     # eval_env.num_envs == 2 * 128 * 256
    es.learn(50, callback=lambda es, stats: print(stats["generation"], stats["best_flying_lap_seconds"]))
    es.write_back(model); model.save("polished")

The default weights of fitness="lap" (w_lap = -1, a crash costing `DEFAULT_CRASH_STEPS` steps, no_lap_steps = the evaluation length) and
the default sigma and lr are UNTUNED: nobody has measured whether they improve a PPO-trained policy.  No CPU fallback.
"""
import ctypes as C
import math

from . import _lib
from ._closed_loop import _as_actor, _precision_flags, group_size

MAX_PAIRS = 128              # qr_es_create: P = 256 is the pointer table of the one bank-load launch
DEFAULT_CRASH_STEPS = 100.0  # fitness="lap": what one crash per env costs, in steps of mean flying-lap time (untuned)
SHAPINGS = {"centered_rank": _lib.QR_ES_SHAPE_CENTERED_RANK, "none": _lib.QR_ES_SHAPE_NONE}
WEIGHT_NAMES = ("w_gate", "w_crash", "w_timeout", "w_return", "w_lap", "no_lap_steps")
SUMMARY_NAMES = ("gates", "crashes", "timeouts", "first_laps", "first_lap_steps", "flying_laps", "flying_lap_steps", "return_sum")


def num_params(obs_len):
    """length of the actor block pi: w1 b1 w2 b2 w3 b3 w4 b4 (qr_es_num_params)"""
    return 120 * int(obs_len) + 29644


def lap_weights(n_eval_steps, crash_steps=DEFAULT_CRASH_STEPS):
    """the weights of fitness="lap": minus the mean flying-lap steps (the evaluation length where there is no flying lap), minus
    `crash_steps` per crash and env"""
    return dict(w_gate=0.0, w_crash=-float(crash_steps), w_timeout=0.0, w_return=0.0, w_lap=-1.0, no_lap_steps=float(n_eval_steps))


def _check_arguments(num_envs, pairs, envs_per_policy, sigma, lr, betas, weight_decay, fitness, shaping, n_eval_steps, eval_seeds, eps):
    """every argument check of EvolutionStrategy, before the env or the device is touched; returns (pairs, E, weights or None)"""
    pairs = int(pairs)
    if not 1 <= pairs <= MAX_PAIRS:
        raise ValueError("pairs must be in 1..%d (the population is 2 x pairs bank slots of one launch)" % MAX_PAIRS)
    E, slots = group_size(envs_per_policy, num_envs, "envs_per_policy", "policy")
    if slots != 2 * pairs:
        raise ValueError("env.num_envs must equal 2 * pairs * envs_per_policy (%d), not %d" % (2 * pairs * E, int(num_envs)))
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0")
    if not (lr >= 0 and math.isfinite(lr)):
        raise ValueError("lr must be finite and >= 0")
    if len(betas) != 2 or not all(0 <= b < 1 for b in betas):
        raise ValueError("betas must be two values in [0, 1)")
    if not (math.isfinite(weight_decay) and weight_decay >= 0) or not (math.isfinite(eps) and eps > 0):
        raise ValueError("weight_decay must be >= 0 and eps > 0")
    if shaping not in SHAPINGS:
        raise ValueError("shaping must be one of %s" % sorted(SHAPINGS))
    if int(n_eval_steps) < 1:
        raise ValueError("need n_eval_steps >= 1")
    if eval_seeds not in ("fixed", "per_generation"):
        raise ValueError("eval_seeds must be 'fixed' or 'per_generation'")
    if callable(fitness):
        weights = None
    elif fitness == "lap":
        weights = lap_weights(n_eval_steps)
    elif isinstance(fitness, dict):
        unknown = set(fitness) - set(WEIGHT_NAMES)
        if unknown:
            raise ValueError("unknown fitness weight(s) %s; the weights are %s" % (sorted(unknown), list(WEIGHT_NAMES)))
        weights = dict(lap_weights(n_eval_steps, 0.0), w_lap=0.0)
        weights.update({k: float(v) for k, v in fitness.items()})
    else:
        raise ValueError("fitness must be 'lap', a dict of weights or a callable(rec, recf) -> float64 tensor [P]")
    return pairs, E, weights


class EvolutionStrategy:
    """ES on the actor of `model` (anything evaluation._as_actor accepts: a checkpoint path, an SB3-shaped PPO, a native trainer, a bare
    torch actor), flown on `env` (a race env of this package; env.num_envs == 2 * pairs * envs_per_policy).

    fitness: "lap" (see lap_weights), a dict of qr_es_fitness weights (w_gate, w_crash, w_timeout, w_return, w_lap, no_lap_steps; absent
    ones 0, no_lap_steps = n_eval_steps), or a callable(rec, recf) -> float64 CUDA tensor [P] of scores (higher is better); the members
    the scores belong to are the rows of `self.members` [P, n].  shaping: "centered_rank" | "none".  eval_seeds: "fixed" flies every
    generation on the starts of `seed`, "per_generation" on those of seed + generation.  precision: passed to the bank evaluator (None:
    the model's own collect precision).  The defaults of sigma, lr and fitness="lap" are untuned (module text)."""

    def __init__(self, env, model, pairs=64, envs_per_policy=256, sigma=0.02, lr=0.01, betas=(0.9, 0.999), weight_decay=0.0, fitness="lap",
                 shaping="centered_rank", n_eval_steps=1200, gates_per_lap=None, precision=None, seed=0, eval_seeds="fixed", eps=1e-8):
        from .sb3 import _unwrap

        core = _unwrap(env)
        self.pairs, self.E, self.weights = _check_arguments(core.num_envs, pairs, envs_per_policy, sigma, lr, betas, weight_decay, fitness, shaping,
                                                            n_eval_steps, eval_seeds, eps)
        import torch

        from ._closed_loop import _model_precision
        from .evaluation import REC_FLOATS, REC_INTS, default_gates_per_lap
        from .policy import MfmaPolicyBank

        self._L = _lib.load()
        self._h = None
        self.P = 2 * self.pairs
        self.sigma, self.lr, self.betas, self.weight_decay, self.eps = float(sigma), float(lr), (float(betas[0]), float(betas[1])), float(weight_decay), float(eps)
        self.fitness_fn = fitness if callable(fitness) else None
        self.shaping, self.n_eval_steps, self.eval_seeds = shaping, int(n_eval_steps), eval_seeds
        self.seed, self.generation = int(seed), 0
        actor, owner = _as_actor(model)
        self.precision = _model_precision(owner) if precision is None else precision
        _precision_flags(self.precision)
        self.core, self.device = core, core.device
        self.gates_per_lap = default_gates_per_lap(core) if gates_per_lap is None else int(gates_per_lap)
        self.obs_len = int(core.state_len)
        self.n = num_params(self.obs_len)
        h = C.c_void_p()
        _lib.check(_lib.require(self._L, "qr_es_create")(self.obs_len, self.device.index, self.pairs, C.byref(h)))
        self._h = h
        assert self._L.qr_es_num_params(self._h) == self.n
        f32 = dict(dtype=torch.float32, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1).to(**f32) for lin in actor if isinstance(lin, torch.nn.Linear) for p in (lin.weight, lin.bias)])
        if flat.numel() != self.n:
            raise ValueError("the model's actor is not the obs -> 120 -> 120 -> 120 -> 4 network of a %d-long observation" % self.obs_len)
        self.theta = flat.contiguous()
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.members = torch.zeros((self.P, self.n), **f32)
        self.bank = MfmaPolicyBank(self.obs_len, self.P, self.device.index)
        self.rec = torch.zeros((core.num_envs, REC_INTS), dtype=torch.int32, device=self.device)
        self.recf = torch.zeros((core.num_envs, REC_FLOATS), **f32)
        self.scores = torch.zeros(self.P, **f64)          # what qr_es_update reads: qr_es_fitness's scores, or the callable's
        self.summary = torch.zeros((self.P, 8), **f64)    # qr_es_fitness's summary of the last generation

    # ------------------------------------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.qr_es_destroy(self._h)
            self._h = None
            self.bank.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------ one generation
    def _stream(self):
        import torch

        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _weights_struct(self):
        w = self.weights if self.weights is not None else lap_weights(self.n_eval_steps)
        return _lib.QrEsFitnessWeights(*[w[k] for k in WEIGHT_NAMES])

    def eval_seed(self, generation=None):
        g = self.generation if generation is None else int(generation)
        return self.seed if self.eval_seeds == "fixed" else self.seed + g

    def step(self):
        """One generation: perturb into the bank, fly all members on shared starts, score, update.  Returns the stats dict: generation
        (the one just flown), best / mean / worst score, and the best member's index, flying-lap seconds (None without a flying lap),
        crashes per env and summary."""
        L, st, p = self._L, self._stream(), lambda t: C.c_void_p(t.data_ptr())
        g, core = self.generation, self.core
        _lib.check(L.qr_es_perturb(self._h, p(self.theta), self.sigma, self.seed, g, self.bank._h, 0, p(self.members), st))
        core.seed(self.eval_seed())
        core.reset_device()
        core.share_starts(self.E)
        self.rec.zero_()
        self.recf.zero_()
        core.evaluate_bank_device(self.bank, self.P, self.E, self.n_eval_steps, self.gates_per_lap, self.rec, self.recf, precision=self.precision)
        w = self._weights_struct()
        _lib.check(L.qr_es_fitness(self._h, p(self.rec), p(self.recf), self.E, C.byref(w), p(self.summary), p(self.scores), st))
        if self.fitness_fn is not None:
            self.scores.copy_(self.fitness_fn(self.rec, self.recf).reshape(self.P))
        _lib.check(L.qr_es_update(self._h, p(self.theta), p(self.m), p(self.v), p(self.scores), self.sigma, self.seed, g, SHAPINGS[self.shaping],
                                  self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, g + 1, None, st))
        self.generation = g + 1
        import torch

        host = torch.cat([self.scores[:, None], self.summary], dim=1).cpu().numpy()   # the generation's one host read: P x 9 doubles
        return self._stats(g, host[:, 0], host[:, 1:])

    def _stats(self, generation, scores, summary):
        import numpy as np

        finite = np.where(np.isnan(scores), -np.inf, scores)
        best = int(np.argmax(finite))
        s = summary[best]
        return dict(generation=generation, best=float(scores[best]), mean=float(np.mean(scores)), worst=float(np.min(finite)), best_member=best,
                    best_flying_lap_seconds=float(s[6] / s[5] * self.core.dt) if s[5] > 0 else None, best_crashes_per_env=float(s[1] / self.E),
                    best_summary=dict(zip(SUMMARY_NAMES, (float(x) for x in s))))

    def learn(self, generations, callback=None):
        """`generations` calls of step(); callback(self, stats) after each, a true return value stops early.  Returns the list of stats."""
        history = []
        for _ in range(int(generations)):
            stats = self.step()
            history.append(stats)
            if callback is not None and callback(self, stats):
                break
        return history

    # ------------------------------------------------------------------------------------------------ the result
    def actor_layers(self):
        """theta as [(w1, b1), ..., (w4, b4)] views in torch Linear layout"""
        shapes, out, off = [(120, self.obs_len), (120, 120), (120, 120), (4, 120)], [], 0
        for rows, cols in shapes:
            w = self.theta[off:off + rows * cols].view(rows, cols)
            off += rows * cols
            out.append((w, self.theta[off:off + rows]))
            off += rows
        return out

    def write_back(self, model):
        """Copy the actor into `model` (a native trainer, an SB3-shaped PPO or a bare torch actor), in place, so that `model.save`
        keeps it; a trainer's packed operand images are rebuilt."""
        import torch

        actor, owner = _as_actor(model)
        linears = [lin for lin in actor if isinstance(lin, torch.nn.Linear)]
        with torch.no_grad():
            for lin, (w, b) in zip(linears, self.actor_layers()):
                lin.weight.copy_(w)
                lin.bias.copy_(b)
        trainer = getattr(owner, "_trainer", None) or owner
        if hasattr(trainer, "sync_parameters"):
            trainer.sync_parameters()
        return model

    def state_dict(self):
        """theta, both moments, the generation, the seeds and the hyper-parameters: load_state_dict() on an EvolutionStrategy built with the
        same env, pairs and envs_per_policy continues bit for bit."""
        return dict(theta=self.theta.clone(), m=self.m.clone(), v=self.v.clone(), generation=self.generation, seed=self.seed, eval_seeds=self.eval_seeds,
                    sigma=self.sigma, lr=self.lr, betas=tuple(self.betas), eps=self.eps, weight_decay=self.weight_decay, shaping=self.shaping,
                    weights=None if self.weights is None else dict(self.weights), n_eval_steps=self.n_eval_steps, gates_per_lap=self.gates_per_lap,
                    precision=self.precision, pairs=self.pairs, envs_per_policy=self.E, obs_len=self.obs_len)

    def load_state_dict(self, sd):
        if (sd["pairs"], sd["envs_per_policy"], sd["obs_len"]) != (self.pairs, self.E, self.obs_len):
            raise ValueError("the state belongs to another population shape or observation length")
        for name in ("theta", "m", "v"):
            getattr(self, name).copy_(sd[name])
        self.generation, self.seed, self.eval_seeds = int(sd["generation"]), int(sd["seed"]), sd["eval_seeds"]
        self.sigma, self.lr, self.betas, self.eps, self.weight_decay = float(sd["sigma"]), float(sd["lr"]), tuple(sd["betas"]), float(sd["eps"]), float(sd["weight_decay"])
        self.shaping, self.n_eval_steps, self.gates_per_lap, self.precision = sd["shaping"], int(sd["n_eval_steps"]), int(sd["gates_per_lap"]), sd["precision"]
        if self.fitness_fn is None:
            self.weights = dict(sd["weights"])
        return self
