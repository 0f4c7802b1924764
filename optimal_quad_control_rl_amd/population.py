"""A population of PPO learners on ONE env handle, collecting in ONE launch (`qr_rollout_policy_population`,
csrc/quadrace_rollout_population.hip).

Per-seed outcomes of a training run are chaotic: the practical answer is to train several seeds or hyper-parameter
settings and keep the best.  `evaluate_policies` / `rank_policies` rank a bank of policies in one launch; this module is the other
half: P members share an env of P x E envs, member p owns envs [p E, (p + 1) E), and every round's collect phase is one kernel launch
in which each 256-env workgroup stages ITS member's weights and samples with ITS member's log_std and noise seed.  A collect launch of
E = 256 envs alone occupies one of the GPU's 256 CUs.

Each member is an ordinary `ppo.PPO(fused_collect=True)` built on a thin view of the env (`_MemberEnv`): a member
does not know it is one of many.  The kernel's contract (include/quadrace.h) makes member p bit-equal to a standalone PPO on an E-env
handle with env_id_base + p E.  With `batched_update=False` (the default) the P updates still run one after another, each through its
member's own updater; with `batched_update=True` they run as ONE launch sequence for all members (`qr_ppo_population_epoch`,
csrc/quadrace_ppo_population.hip: three launches per minibatch of the whole population), and every member ends bit for bit where its own
update would have left it.  `batched_prepare=True` (with `batched_update=True`) moves the rest of the round to the device as well: the
bank is loaded in one launch from the members' parameter vectors, and the members' value forwards, slice copies, buffer sanitising and GAE
run as four launches and ONE blocking read for the whole population (`qr_ppo_population_prepare`, csrc/quadrace_population_prepare.hip);
`batched_prepare=False` (the default) is the path described above, unchanged.

Selection and mutation: `PopulationPPO.exploit` overwrites members with copies of other members -- parameters, Adam state, operand images,
one launch for all of them with `batched_update=True` (`qr_ppo_population_exploit`) -- and `PBT` is the schedule on top of it
(population-based training: every `interval` rounds the worst quantile is replaced by perturbed copies of the best); pass it as
`PopulationPPO(..., pbt=PBT(...))`.  Without `pbt=` a population is P independent runs, as before.  `.members` are the learners, `.bank`
holds their current actors for `evaluate_policies` / `rank_policies`, and `state_dict` / `load_state_dict` nest the members', so a user
can write another schedule on `exploit`."""
import copy
import math

import numpy as np
import torch

from ._closed_loop import group_size
from .ppo import PPO

# what a destination of exploit() inherits from its source besides parameters and optimiser state (attributes of ppo.PPO) ...
INHERITED = ("lr0", "_kl_lr_scale", "_kl_first_trips", "clip", "ent_coef", "target_kl")
# ... and the ppo.PPO keyword names under which PBT perturbs three of them
PERTURBABLE = {"learning_rate": "lr0", "clip_range": "clip", "ent_coef": "ent_coef"}


def check_exploit(P, src_of, log_std_shift=None):
    """The argument checks of qr_ppo_population_exploit, as ValueErrors -> (src_of as ints, shifts as floats)."""
    src_of = [int(s) for s in src_of]
    shift = [0.0] * P if log_std_shift is None else [float(x) for x in log_std_shift]
    if len(src_of) != P or len(shift) != P:
        raise ValueError("src_of (and log_std_shift) hold one entry per member")
    if any(s < 0 or s >= P for s in src_of):
        raise ValueError("src_of holds an index outside [0, %d)" % P)
    if any(src_of[s] != s for s in src_of):
        raise ValueError("a source is itself a destination: a member that is copied from keeps its own state in the same call")
    if not all(math.isfinite(x) for x in shift):
        raise ValueError("log_std_shift must be finite")
    return src_of, shift


class PBT:
    """A population-based-training schedule: truncation selection every `interval` rounds.

    interval: rounds (collect + train) between decisions; warmup_rounds: rounds before the first interval starts.
    quantile: the bottom ceil(quantile * P) members are overwritten, each by a member drawn uniformly from the top ceil(quantile * P);
    at most 0.5.  A member of the top set is never overwritten, a member without a fitness is never a source.
    fitness: "ep_rew_mean" or "gates_per_episode" -- the episode-weighted mean of that training statistic over the rounds since the last
    decision, counting only rounds in which the member finished episodes -- or a callable f(population) -> P floats (None / NaN: no
    fitness), asked at decision time.  Higher is better.
    perturb: {"learning_rate" | "clip_range" | "ent_coef": (factor, factor)}: each destination multiplies the value it inherits by one of
    the two, drawn per name; the result is clamped to bounds[name] = (low, high).  log_std_shift = s: each destination's log_std is its
    source's plus +s or -s.
    seed: the draws of decision k come from numpy's default_rng((seed, k)) and from nothing else: `plan` is a pure function."""

    def __init__(self, interval=10, quantile=0.25, fitness="ep_rew_mean", perturb=None, bounds=None, log_std_shift=0.0, seed=0, warmup_rounds=0):
        if int(interval) != interval or interval < 1 or int(warmup_rounds) != warmup_rounds or warmup_rounds < 0:
            raise ValueError("interval must be a whole number >= 1 and warmup_rounds one >= 0")
        if not 0.0 < float(quantile) <= 0.5:
            raise ValueError("quantile must lie in (0, 0.5]: above it the sources and the destinations would overlap")
        if not (callable(fitness) or fitness in ("ep_rew_mean", "gates_per_episode")):
            raise ValueError("fitness must be 'ep_rew_mean', 'gates_per_episode' or a callable f(population) -> P floats")
        perturb, bounds = dict(perturb or {}), dict(bounds or {})
        for name, pair in perturb.items():
            if name not in PERTURBABLE or len(pair) != 2 or not all(math.isfinite(f) and f > 0.0 for f in pair):
                raise ValueError("perturb maps %s to a pair of positive factors" % " / ".join(PERTURBABLE))
        for name, (lo, hi) in bounds.items():
            if name not in PERTURBABLE or not lo <= hi:
                raise ValueError("bounds maps %s to (low, high)" % " / ".join(PERTURBABLE))
        if not (math.isfinite(log_std_shift) and log_std_shift >= 0.0):
            raise ValueError("log_std_shift must be finite and >= 0")
        self.interval, self.quantile, self.fitness, self.warmup_rounds = int(interval), float(quantile), fitness, int(warmup_rounds)
        self.perturb = {k: (float(a), float(b)) for k, (a, b) in perturb.items()}
        self.bounds = {k: (float(a), float(b)) for k, (a, b) in bounds.items()}
        self.log_std_shift, self.seed = float(log_std_shift), int(seed)

    def due(self, rounds):
        """Is a decision due after `rounds` rounds of training?"""
        done = rounds - self.warmup_rounds
        return done > 0 and done % self.interval == 0

    def plan(self, fitness, decision_index):
        """fitness: P values (None / NaN: none) -> (src_of, factors): src_of[p] == p leaves member p alone; factors[p] is None for such a
        member and for a destination {name: factor for the names of `perturb`} plus "log_std_shift": +-s.  Ranking: higher fitness first,
        ties by index, members without a fitness last (by index).  The destinations, in index order, each draw a source, then one factor
        per name in sorted order, then (log_std_shift > 0 only) the sign of the shift."""
        P = len(fitness)
        valid = [p for p in range(P) if fitness[p] is not None and not math.isnan(float(fitness[p]))]
        ranked = sorted(valid, key=lambda p: (-float(fitness[p]), p)) + [p for p in range(P) if p not in valid]
        k = int(math.ceil(self.quantile * P))
        top = ranked[:min(k, len(valid))]
        src_of, factors = list(range(P)), [None] * P
        if not top:
            return src_of, factors
        rng = np.random.default_rng((self.seed, int(decision_index)))
        for p in sorted(q for q in ranked[P - k:] if q not in top):
            src_of[p] = top[int(rng.integers(len(top)))]
            f = {name: self.perturb[name][int(rng.integers(2))] for name in sorted(self.perturb)}
            f["log_std_shift"] = (self.log_std_shift if int(rng.integers(2)) else -self.log_std_shift) if self.log_std_shift else 0.0
            factors[p] = f
        return src_of, factors

    def perturbed(self, name, value, factor):
        """value * factor, clamped to bounds[name]"""
        lo, hi = self.bounds.get(name, (-math.inf, math.inf))
        return min(max(float(value) * float(factor), lo), hi)


class _MemberEnv:
    """What ppo.PPO asks of its env, for envs [lo, hi) of the population's handle: num_envs, state_len, device, the member's slices of
    the reset observation, of the state and of the terminal-observation buffer, and a rollout_policy_device that hands back the
    member's slice of the shared launch copied into the member's own contiguous buffers."""

    def __init__(self, owner, index):
        self._owner, self._index = owner, index
        self._lo, self._hi = index * owner.envs_per_member, (index + 1) * owner.envs_per_member
        self.num_envs, self.state_len, self.device = owner.envs_per_member, owner.env.state_len, owner.env.device
        self.VARIANT = owner.env.VARIANT
        self._term = None

    def reset_device(self):
        """The member's rows of the observation of the population's one reset (PopulationPPO.__init__); not a reset of its own."""
        return self._owner._obs0[self._lo:self._hi]

    def set_terminal_obs_buffer(self, buf):
        assert buf is None or (buf.dim() == 3 and tuple(buf.shape[1:]) == (self.num_envs, self.state_len))
        self._term = buf

    def rollout_policy_device(self, policy, num_steps, log_std, noise_seed=0, first_step=0, deterministic=False, out=None,
                              precision="f16-operands"):
        """The member's slice of the launch PopulationPPO.collect() made.  `policy` (the member's own MfmaPolicy) is not flown: the
        launch read the member's bank slot, loaded from the same actor."""
        launch = self._owner._launch
        if launch is None or self._index in launch["taken"]:
            raise RuntimeError("member %d has no collected rollout to take: call PopulationPPO.collect() first" % self._index)
        if (int(num_steps), int(first_step), int(noise_seed), bool(deterministic), precision) != \
                (launch["K"], launch["first_step"], launch["seeds"][self._index], False, launch["precision"]):
            raise RuntimeError("member %d asks for another rollout than the population launched" % self._index)
        launch["taken"].add(self._index)
        lo, hi = self._lo, self._hi
        parts = [t[:, lo:hi] for t in launch["out"][:6]]
        if out is None:
            out = tuple(p.contiguous() for p in parts)
        else:
            for dst, src in zip(out, parts):
                dst.copy_(src)
        if self._term is not None:
            self._term.copy_(self._owner._term_obs[:, lo:hi])
        return (*out, launch["out"][6][lo:hi].contiguous())

    # checkpoints (ppo.PPO.state_dict / load_state_dict)
    def get_state_tensors(self):
        return tuple(None if t is None else t[self._lo:self._hi].contiguous() for t in self._owner.env.get_state_tensors())

    def set_state_tensors(self, world=None, dist=None, target=None, steps=None, episode=None):
        env = self._owner.env
        full = list(env.get_state_tensors())
        for k, part in enumerate((world, dist, target, steps, episode)):
            if part is not None and full[k] is not None:
                full[k][self._lo:self._hi] = torch.as_tensor(part).to(device=full[k].device, dtype=full[k].dtype)
        env.set_state_tensors(*full)

    def update_states(self):
        self._owner._refresh_obs()

    @property
    def states_tensor(self):
        return self._owner.env.states_tensor[self._lo:self._hi]


class PopulationPPO:
    """P = len(members) PPO learners on `env` (P * envs_per_member envs), one collect launch per round.

    members: a list of dicts of per-member `ppo.PPO` keywords (seed, learning_rate, ent_coef, clip_range, target_kl, log_std_init, ...);
    shared_hyper: `ppo.PPO` keywords every member gets (n_steps, batch_size, n_epochs, native_update, policy_forward, ...).  n_steps and
    policy_forward must be the same for all: one launch has one K and one forward.  A member's `seed` seeds its network, its
    minibatch permutations and its action noise, as in ppo.PPO.
    conditions / condition_of_member: a list of conditions.Condition and, per member, the index of the one its envs fly under
    (default: all under the first); without `conditions` the single condition is Condition.from_env(env).
    The env is reset once here (condition_reset with `conditions`), which is every member's start.
    batched_update: train() runs the members' updates through one `ppo.MfmaPpoPopulationUpdater` instead of one after another.  Needs
    native_update=True for every member, the f16-operand kernels (no policy_forward="f32class", no update_precision="f32"), one batch_size and
    one n_epochs for all, and a single process (no data-parallel process group): anything else is a ValueError.
    batched_prepare: collect() fills the bank with ONE device launch (`MfmaPpoPopulationUpdater.load_bank`) and train() replaces the members'
    collect_fused() + buffer sanitising + GAE by ONE `MfmaPpoPopulationUpdater.prepare` for all members; every tensor ends bit for bit where
    the members' own steps leave it, and a member's own MfmaPolicy is no longer loaded.  Needs batched_update=True and the race envs (a
    ValueError otherwise); truncation_bootstrap may differ between members (a member without it passes no term_val).
    pbt: a `PBT` schedule (None: none, and nothing below exists).  train() then ends with the schedule's bookkeeping (the round count and the
    fitness accumulators), learn() applies a decision (`pbt_step`) whenever one is due, `.lineage` lists per replaced member
    (round, dst, src, (fitness of dst, fitness of src), the destination's new hyper-parameters), and state_dict / load_state_dict carry
    the schedule's position, the accumulators, the lineage and each member's clip / ent_coef / target_kl for a bit-for-bit resume.
    A decision that changes a member's clip or ent_coef changes the argument set of `qr_ppo_population_epoch`: the next train() pays one
    table upload and one graph re-capture, once per decision.  A changed learning rate costs nothing: it travels in the arguments of
    ppo_population_lr_kernel every round anyway."""

    def __init__(self, env, members, envs_per_member=256, conditions=None, condition_of_member=None, batched_update=False, batched_prepare=False,
                 pbt=None, **shared_hyper):
        from .conditions import Condition, ConditionBank
        from .policy import MfmaPolicyBank

        members = [dict(m) for m in members]
        if len(members) < 1:
            raise ValueError("members must hold at least one dict of PPO keywords")
        if pbt is not None:
            if not isinstance(pbt, PBT):
                raise ValueError("pbt must be a population.PBT schedule")
            if len(members) < 2:
                raise ValueError("pbt needs at least two members: one to copy from and one to overwrite")
        self.pbt, self.lineage = pbt, []
        self._pbt_round, self._pbt_decisions = 0, 0
        self._pbt_acc = [[0.0, 0.0] for _ in members]   # per member: episodes, sum of episodes x statistic since the last decision
        self.envs_per_member, slots = group_size(envs_per_member, env.num_envs, "envs_per_member", "member")
        if slots != len(members):
            raise ValueError("len(members) * envs_per_member must equal env.num_envs (%d * %d != %d)"
                             % (len(members), self.envs_per_member, env.num_envs))
        hyper = [{**shared_hyper, **m} for m in members]
        for key, default in (("n_steps", 32), ("policy_forward", "torch")):
            if len({h.get(key, default) for h in hyper}) != 1:
                raise ValueError("%s is shared by the whole population (one launch has one K and one forward): give one value" % key)
        if any(not h.get("fused_collect", True) for h in hyper):
            raise ValueError("a population collects in the closed-loop kernel: fused_collect=False is not available")
        if any(h.get("conditions") is not None for h in hyper):
            raise ValueError("give `conditions` to PopulationPPO itself, with condition_of_member")
        self.batched_update, self.batched_prepare = bool(batched_update), bool(batched_prepare)
        if self.batched_prepare:
            if not self.batched_update:
                raise ValueError("batched_prepare needs batched_update=True: it prepares the buffers of the batched update")
            if hasattr(env, "KIND") and hasattr(env, "trainer_state"):
                raise ValueError("batched_prepare is built for the race envs: the predecessor envs keep the members' own prepare steps")
        if self.batched_update:
            from .ppo import MfmaPpoUpdater

            if any(not h.get("native_update", False) for h in hyper):
                raise ValueError("batched_update needs native_update=True for every member: it batches the matrix-core update")
            if any(h.get("policy_forward", "torch") == "f32class" or h.get("update_precision", "f16-operands") == "f32" for h in hyper):
                raise ValueError("batched_update has no f32-class form: policy_forward='f32class' / update_precision='f32' are not available")
            for key in ("batch_size", "n_epochs"):
                if len({h.get(key) for h in hyper}) != 1:
                    raise ValueError("batched_update: %s is shared by the whole population (one launch sequence has one shape)" % key)
            if MfmaPpoUpdater.data_parallel():
                raise ValueError("batched_update is single-process: a data-parallel process group is initialised")
        self.env, self.n_steps = env, int(hyper[0].get("n_steps", 32))
        self.precision = "f32" if hyper[0].get("policy_forward", "torch") == "f32class" else "f16-operands"
        if conditions is None:
            if condition_of_member is not None:
                raise ValueError("condition_of_member needs `conditions`")
            self.conditions, self.condition_of_member = [Condition.from_env(env)], [0] * len(members)
            self._obs0 = env.reset_device().clone()
        else:
            self.conditions = list(conditions)
            self.condition_of_member = [0] * len(members) if condition_of_member is None else [int(c) for c in condition_of_member]
            if len(self.condition_of_member) != len(members) or any(c < 0 or c >= len(self.conditions) for c in self.condition_of_member):
                raise ValueError("condition_of_member must hold one index into `conditions` per member")
            self._obs0 = env.condition_reset(self.conditions, self.condition_of_member, self.envs_per_member).clone()
        self._cond_bank = ConditionBank(env.VARIANT, len(self.conditions), env.device.index)
        for slot, c in enumerate(self.conditions):
            self._cond_bank.set(slot, c)
        self.bank = MfmaPolicyBank(env.state_len, len(members), env.device.index)
        self._launch = None
        self._out = None
        self._views = [_MemberEnv(self, p) for p in range(len(members))]
        self.members = [PPO(view, **{**h, "fused_collect": True}) for view, h in zip(self._views, hyper)]
        # the launch writes terminal observations of all N envs into one buffer; the views hand each member its columns
        self._term_obs = None
        if any(v._term is not None for v in self._views):
            self._term_obs = torch.zeros((self.n_steps, env.num_envs, env.state_len), dtype=torch.float32, device=env.device)
        env.set_terminal_obs_buffer(self._term_obs)
        self._pop_updater = None
        if self.batched_update:
            from .ppo import MfmaPpoPopulationUpdater

            self._pop_updater = MfmaPpoPopulationUpdater([m._updater for m in self.members])
        self.load_bank()

    # ---------------------------------------------------------------------------------------------------------------- rounds
    def load_bank(self):
        """Slot p of `.bank` <- member p's current actor: done by collect(); call it yourself before ranking after a train()."""
        if self.batched_prepare:   # one launch, packed on the device from the members' parameter vectors
            return self._pop_updater.load_bank(self.bank, 0)
        for p, m in enumerate(self.members):
            self.bank.load_torch(p, m.policy.pi)
        return self.bank

    @torch.no_grad()
    def collect(self):
        """Load every member's actor into its bank slot and fly all members' n_steps in one launch.  The members take their slices in
        train() (or through their own collect_fused())."""
        steps = {int(m.noise_step) for m in self.members}
        if len(steps) != 1:
            raise RuntimeError("the members stand at different positions of their noise streams: they no longer share a launch")
        self.load_bank()
        env, K, P = self.env, self.n_steps, len(self.members)
        if self._out is None:
            from ._closed_loop import rollout_outputs

            self._out = rollout_outputs(K, env.num_envs, env.state_len, env.device)
        seeds = [int(m.noise_seed) for m in self.members]
        log_stds = torch.stack([m.policy.log_std.detach() for m in self.members])
        first_step = steps.pop()
        out = env.rollout_policy_population_device(self.bank, list(range(P)), self._cond_bank, self.condition_of_member, self.envs_per_member,
                                                   K, log_stds, seeds, first_step=first_step, out=self._out, precision=self.precision)
        self._launch = dict(K=K, first_step=first_step, seeds=seeds, precision=self.precision, out=out, taken=set())
        return self

    def train(self):
        """Each member in turn: its collect_fused() (takes its slice of the launch, evaluates its values) and its train() -- or, with
        batched_update, every member's part of train() before the launches, ONE update launch sequence for all, every member's part after."""
        if self._launch is None:
            raise RuntimeError("call collect() before train()")
        if self.pbt is not None:   # "episodes" is written only in a round that finished some: taken out, it tells this round from an older one
            held = [m.stats.pop("episodes", None) for m in self.members]
        if self.batched_update:
            self._train_batched()
        else:
            for m in self.members:
                m.collect_fused()
                m.train()
        self._launch = None
        if self.pbt is not None:
            self._pbt_after_round(held)
        return self

    # ------------------------------------------------------------------------------------------------- selection and mutation
    @torch.no_grad()
    def exploit(self, src_of, log_std_shift=None, hyper=None):
        """Every member p with src_of[p] != p becomes a copy of member s = src_of[p]: parameters (log_std plus log_std_shift[p]), Adam
        moments and step count, operand images -- with batched_update ONE device launch for all of them (`MfmaPpoPopulationUpdater.exploit`),
        otherwise copies, `pack()` and the step write through each member's own updater (members without native_update: their torch
        parameters and `opt` state); both leave the same bits.  p then inherits s's lr0, _kl_lr_scale, _kl_first_trips, clip, ent_coef and
        target_kl; hyper[p] (a dict of those names) overrides them.  p keeps its own seed, noise and shuffle streams, envs, episode
        accumulators, num_timesteps and condition.  The bank is reloaded by the next collect().
        ValueError: what qr_ppo_population_exploit refuses (a wrong length, an index outside [0, P), a source that is itself a
        destination, a non-finite shift) and an unknown name in `hyper`; RuntimeError: between collect() and train()."""
        P = len(self.members)
        src_of, shift = check_exploit(P, src_of, log_std_shift)
        hyper = dict(hyper or {})
        for p, h in hyper.items():
            if not (isinstance(p, int) and 0 <= p < P) or any(name not in INHERITED for name in h):
                raise ValueError("hyper maps a member index to a dict of %s" % ", ".join(INHERITED))
        if self._launch is not None:
            raise RuntimeError("a collected rollout is waiting for train(): exploit between rounds")
        dst = [p for p in range(P) if src_of[p] != p]
        if self._pop_updater is not None:
            self._pop_updater.exploit(src_of, shift)
        else:
            for p in dst:
                d, s = self.members[p], self.members[src_of[p]]
                add = torch.tensor(shift[p], dtype=torch.float32, device=d.dev)   # one float32 add, also of 0: what the kernel does
                if d._updater is not None and s._updater is not None:
                    for name in ("theta", "m", "v"):
                        getattr(d._updater, name).copy_(getattr(s._updater, name))
                    d._updater.theta[-4:].add_(add)
                    d._updater.pack()
                    d._updater.step = s._updater.step
                elif d._updater is None and s._updater is None:
                    for pd, ps in zip(d.policy.parameters(), s.policy.parameters()):
                        pd.data.copy_(ps.data)
                    d.policy.log_std.data.add_(add)
                    state = copy.deepcopy(s.opt.state_dict())
                    state["param_groups"] = d.opt.state_dict()["param_groups"]
                    d.opt.load_state_dict(state)
                else:
                    raise ValueError("members %d and %d differ in native_update: their optimiser states have no common form" % (p, src_of[p]))
        for p in dst:
            d, s = self.members[p], self.members[src_of[p]]
            for name in INHERITED:
                setattr(d, name, getattr(s, name))
            for name, value in hyper.get(p, {}).items():
                setattr(d, name, value)
        return self

    def _pbt_after_round(self, held):
        """train()'s last step under a schedule: the round count and, past the warm-up, each member's episodes of THIS round."""
        self._pbt_round += 1
        key = self.pbt.fitness if isinstance(self.pbt.fitness, str) else None
        for m, acc, old in zip(self.members, self._pbt_acc, held):
            if "episodes" not in m.stats:
                if old is not None:
                    m.stats["episodes"] = old
            elif key is not None and self._pbt_round > self.pbt.warmup_rounds:
                n = float(m.stats["episodes"])
                acc[0] += n
                acc[1] += n * float(m.stats[m._gates_key if key == "gates_per_episode" else key])

    def pbt_fitness(self):
        """Per member the fitness the schedule would decide on now (None: none yet)."""
        if callable(self.pbt.fitness):
            return [None if f is None else float(f) for f in self.pbt.fitness(self)]
        return [acc[1] / acc[0] if acc[0] > 0 else None for acc in self._pbt_acc]

    def pbt_step(self):
        """One decision of the schedule: rank, exploit, perturb, record; the accumulators start again.  learn() calls it when
        `pbt.due(rounds)`; a loop of your own calls it between train() and the next collect().  -> the new lineage entries."""
        pbt, fit = self.pbt, self.pbt_fitness()
        src_of, factors = pbt.plan(fit, self._pbt_decisions)
        hyper, entries = {}, []
        for p, f in enumerate(factors):
            if f is None:
                continue
            s = self.members[src_of[p]]
            hyper[p] = {attr: pbt.perturbed(name, getattr(s, attr), f[name]) for name, attr in PERTURBABLE.items() if name in f}
            new = {attr: hyper[p].get(attr, getattr(s, attr)) for attr in ("lr0", "clip", "ent_coef", "target_kl")}
            entries.append((self._pbt_round, p, src_of[p], (fit[p], fit[src_of[p]]), dict(new, log_std_shift=f["log_std_shift"])))
        self.exploit(src_of, [0.0 if f is None else f["log_std_shift"] for f in factors], hyper)
        self.lineage += entries
        self._pbt_decisions += 1
        self._pbt_acc = [[0.0, 0.0] for _ in self.members]
        return entries

    def _prepare_batched(self):
        """What every member's collect_fused() + _train_prepare() does, for all members at once: the host bookkeeping of each member, ONE
        `prepare` (values, slices, sanitising, GAE, episode state on the device) and the statistics from its report -> per member what
        _train_prepare returns."""
        launch, K, E = self._launch, self.n_steps, self.envs_per_member
        out, args = launch["out"], []
        for p, m in enumerate(self.members):
            if p in launch["taken"]:
                raise RuntimeError("member %d has already taken its rollout of this launch" % p)
            if (int(m.noise_step), int(m.noise_seed)) != (launch["first_step"], launch["seeds"][p]):
                raise RuntimeError("member %d asks for another rollout than the population launched" % p)
            launch["taken"].add(p)
            m.noise_step += K
            m.num_timesteps += K * E
            if getattr(m, "_adv_ret", None) is None:   # persistent: the epoch graph's nodes address these buffers
                m._adv_ret = (torch.empty_like(m.buf_rew), torch.empty_like(m.buf_rew))
            if getattr(m, "_last_val_buf", None) is None:
                m._last_val_buf = torch.empty(E, dtype=torch.float32, device=m.dev)
            m.last_val = m._last_val_buf
            args.append(dict(first_env=p * E, gamma=m.gamma, lam=m.lam, obs=m.buf_obs, act=m.buf_act, old_logp=m.buf_lp, rew=m.buf_rew,
                             done=m.buf_done, val=m.buf_val, term_val=m.buf_term_val, last_val=m.last_val, adv=m._adv_ret[0], ret=m._adv_ret[1],
                             ep_ret=m.ep_ret, ep_len=m.ep_len, ep_gates=m.ep_gates))
        shared = dict(E=E, obs=out[0], act=out[1], logp=out[2], rew=out[3], done=out[4], trunc=out[5], last_obs=out[6], term_obs=self._term_obs)
        views = []
        for m, r in zip(self.members, self._pop_updater.prepare(shared, args)):
            if m.truncation_bootstrap:
                m.stats["truncations"] = int(r[1])
            m.stats["non_finite_rows"] = int(r[0])
            m._stats_pending = False
            if r[5] > 0:
                m.stats.update({"ep_rew_mean": r[2] / r[5], "ep_len_mean": r[3] / r[5], m._gates_key: r[4] / r[5], "episodes": r[5]})
            m.stats["reward_per_step"] = r[6] / float(K * E)
            views.append(m._train_views(*m._adv_ret))
        return views

    def _train_batched(self):
        batches, kl = [], []
        prepared = self._prepare_batched() if self.batched_prepare else None
        for p, m in enumerate(self.members):   # slice, values, GAE, sanitising, learning-rate schedule: exactly ppo.PPO.train's own steps
            if prepared is None:
                m.collect_fused()
                obs, act, old_lp, adv, ret, rows = m._train_prepare()
            else:
                obs, act, old_lp, adv, ret, rows = prepared[p]
            lr, kl_stop, perm = m._native_begin(rows)
            kl.append(kl_stop)
            batches.append(dict(obs=obs, act=act, old_lp=old_lp.contiguous(), adv=adv.contiguous(), ret=ret.contiguous(), perm=perm, lr=lr,
                                clip=m.clip, vf_coef=m.vf_coef, ent_coef=m.ent_coef, max_grad_norm=m.max_grad_norm))
        m0 = self.members[0]
        if not any(kl):   # no early stop anywhere: all epochs of all members are one graph launch
            self._pop_updater.epoch(batches, m0.batch_size, num_epochs=m0.n_epochs, device_shuffle=True)
        else:             # one launch per epoch and ONE status read for all members in between
            ran, stopped_at = 0, [None] * len(self.members)
            for _ in range(m0.n_epochs):
                self._pop_updater.epoch(batches, m0.batch_size, num_epochs=1, device_shuffle=True)
                ran += 1
                for p, st in enumerate(self._pop_updater.status()):
                    if st[0] and stopped_at[p] is None:
                        stopped_at[p] = ran
                if all(at is not None for at in stopped_at):
                    break
            # A member that stopped early saw nothing but no-ops afterwards, except that the later epochs still drew its permutations:
            # its own train() would have left the loop, so its shuffle count is put back to where that leaves it.
            for m, at in zip(self.members, stopped_at):
                if at is not None and at < ran:
                    seed, count = m._updater.shuffle_state()
                    m._updater.set_shuffle(seed, count - (ran - at))
        for m, kl_stop in zip(self.members, kl):
            m._native_finish(kl_stop)

    def learn(self, total_timesteps_per_member, callback=None):
        """Rounds of collect() + train() until every member has seen `total_timesteps_per_member` env steps.  callback(self) after each
        round; returning False stops.  Under a `pbt` schedule a due decision is applied after train() and before the callback."""
        while self.members[0].num_timesteps < total_timesteps_per_member:
            self.collect()
            self.train()
            if self.pbt is not None and self.pbt.due(self._pbt_round):
                self.pbt_step()
            if callback is not None and callback(self) is False:
                break
        return self

    @property
    def num_timesteps(self):
        """env steps collected per member"""
        return int(self.members[0].num_timesteps)

    # ----------------------------------------------------------------------------------------------------------- checkpoints
    def _refresh_obs(self):
        self.env._observe_under(self.conditions, self.condition_of_member, self.envs_per_member)

    def state_dict(self):
        """The members' state_dicts (each with its rows of the env state) and their network parameters, nested; under a `pbt` schedule also
        its position, accumulators and lineage and the members' clip / ent_coef / target_kl (which exploit() moves and ppo.PPO does not save)."""
        sd = dict(envs_per_member=int(self.envs_per_member), condition_of_member=list(self.condition_of_member),
                  members=[dict(trainer=m.state_dict(), policy={k: v.detach().cpu().clone() for k, v in m.policy.state_dict().items()})
                           for m in self.members])
        if self.pbt is not None:
            sd["pbt"] = dict(round=int(self._pbt_round), decisions=int(self._pbt_decisions), acc=[list(a) for a in self._pbt_acc],
                             lineage=[(r, d, s, tuple(f), dict(h)) for r, d, s, f, h in self.lineage],
                             hyper=[dict(clip=m.clip, ent_coef=m.ent_coef, target_kl=m.target_kl) for m in self.members])
        return sd

    def load_state_dict(self, sd):
        if len(sd["members"]) != len(self.members) or int(sd["envs_per_member"]) != self.envs_per_member:
            raise ValueError("the checkpoint holds another population shape")
        if list(sd["condition_of_member"]) != list(self.condition_of_member):
            raise ValueError("the checkpoint flies another condition map: construct the population with it")
        if (self.pbt is not None) != ("pbt" in sd):
            raise ValueError("the checkpoint was written %s a pbt schedule and this population is built %s one"
                             % (("with", "without") if "pbt" in sd else ("without", "with")))
        for m, part in zip(self.members, sd["members"]):
            m.policy.load_state_dict(part["policy"])
            m.load_state_dict(part["trainer"])
        if self.pbt is not None:
            st = sd["pbt"]
            self._pbt_round, self._pbt_decisions = int(st["round"]), int(st["decisions"])
            self._pbt_acc = [[float(a), float(b)] for a, b in st["acc"]]
            self.lineage = [(r, d, s, tuple(f), dict(h)) for r, d, s, f, h in st["lineage"]]
            for m, h in zip(self.members, st["hyper"]):
                m.clip, m.ent_coef, m.target_kl = h["clip"], h["ent_coef"], h["target_kl"]
        self._launch = None
        self.load_bank()
        return self

    def close(self):
        if self._pop_updater is not None:
            self._pop_updater.close()
        self.env.set_terminal_obs_buffer(None)
        self.bank.close()
        self._cond_bank.close()
