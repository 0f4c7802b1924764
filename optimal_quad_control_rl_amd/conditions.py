"""Flight conditions for the grid evaluator (`qr_condition_bank_*`, `qr_evaluate_policy_grid`, csrc/quadrace_eval_grid.hip).

A condition is what a user of the reference changes on the test env before flying a trained policy again -- `test_env.disturbance_ranges
= ranges` (R:4006-4017), `env.disturbance_scale` (R:358, 489), another track or start, another `max_steps` -- as one value:

    from optimal_quad_control_rl_amd import ConditionBank, disturbance_sweep
    conds = disturbance_sweep(env, [0, 0.5, 1, 2, 3])          # the env's own configuration, at five disturbance scales
    bank = ConditionBank(env.VARIANT, len(conds), env.device.index)
    for slot, c in enumerate(conds):
        bank.set(slot, c)

`env.evaluate_grid_device(policy_bank, bank, policy_of_group, condition_of_group, E, ...)` then flies every group of E envs under its
own (policy, condition) pair in one launch; `evaluation.evaluate_grid` is the whole robustness table.  Importing this module needs
neither torch nor a GPU; ConditionBank does.
"""
import ctypes as C
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

from ._closed_loop import _f32p


@dataclass(frozen=True, eq=False)
class Condition:
    """One flight condition: the arguments of qr_set_track (gate_pos [G, 3], gate_yaw [G], start_pos [3]), of qr_set_disturbance
    (disturbance_ranges [6, 2] or None, disturbance_scale), the max_steps of qr_set_limits, and the lap length gates_per_lap.
    disturbance_ranges None = a handle whose disturbances were never set (the only form the INDI variant accepts)."""
    name: str
    gate_pos: np.ndarray
    gate_yaw: np.ndarray
    start_pos: np.ndarray
    disturbance_ranges: object
    disturbance_scale: float
    max_steps: int
    gates_per_lap: int

    def __post_init__(self):
        f32 = lambda a, shape: np.array(a, dtype=np.float32).reshape(shape)   # np.array copies: a condition never aliases its source
        object.__setattr__(self, "gate_pos", f32(self.gate_pos, (-1, 3)))
        object.__setattr__(self, "gate_yaw", f32(self.gate_yaw, (-1,)))
        object.__setattr__(self, "start_pos", f32(self.start_pos, (3,)))
        if self.disturbance_ranges is not None:
            object.__setattr__(self, "disturbance_ranges", f32(self.disturbance_ranges, (6, 2)))
        object.__setattr__(self, "disturbance_scale", float(self.disturbance_scale))
        object.__setattr__(self, "max_steps", int(self.max_steps))
        object.__setattr__(self, "gates_per_lap", int(self.gates_per_lap))
        if self.gate_pos.shape[0] != self.gate_yaw.shape[0]:
            raise ValueError("gate_pos and gate_yaw disagree about the number of gates")

    @property
    def num_gates(self):
        return int(self.gate_pos.shape[0])

    @classmethod
    def from_env(cls, env, **overrides):
        """The env's current configuration (track, start, disturbance ranges and scale, max_steps; gates_per_lap =
        evaluation.default_gates_per_lap) as a condition, every array copied; `overrides` replace fields by name.  An INDI env has
        no disturbances: its condition carries disturbance_ranges None."""
        from .evaluation import default_gates_per_lap

        core = getattr(env, "venv", env)
        while hasattr(core, "venv"):
            core = core.venv
        e2e = getattr(core, "VARIANT", 0) == 0
        gate_pos = overrides.get("gate_pos", core.gate_pos)
        gate_yaw = overrides.get("gate_yaw", core.gate_yaw)
        # the lap length of the condition's OWN track (an overridden one included)
        gp32 = np.asarray(gate_pos, dtype=np.float32).reshape(-1, 3)
        gpl = default_gates_per_lap(SimpleNamespace(num_gates=gp32.shape[0], gate_pos=gp32, gate_yaw=np.asarray(gate_yaw, dtype=np.float32).reshape(-1)))
        fields = dict(name="env", gate_pos=gate_pos, gate_yaw=gate_yaw, start_pos=core.start_pos,
                      disturbance_ranges=core.disturbance_ranges if e2e else None,
                      disturbance_scale=core.disturbance_scale if e2e else 1.0, max_steps=core.max_steps, gates_per_lap=gpl)
        fields.update(overrides)
        return cls(**fields)

    def replace(self, **changes):
        return replace(self, **changes)


def disturbance_sweep(env, scales):
    """One Condition.from_env(env) per entry of `scales`, differing in disturbance_scale (and the name "scale=<s>") only: the
    robustness curve of R:358 / R:489 as the conditions of one grid."""
    return [Condition.from_env(env, name="scale=%g" % float(s), disturbance_scale=float(s)) for s in scales]


class ConditionBank:
    """`capacity` conditions of one env variant side by side on the device (`qr_condition_bank_*`): the argument of
    `env.evaluate_grid_device`.  A slot holds the table image and the scalars a handle configured with that condition holds.
    No CPU fallback."""

    def __init__(self, variant, capacity, device=None):
        import torch

        from . import _lib

        self._lib = _lib
        self._L = _lib.load()
        self._h = None
        if not torch.cuda.is_available():
            raise RuntimeError("ConditionBank needs a gfx950 GPU: libquadrace has no CPU fallback")
        create = _lib.require(self._L, "qr_condition_bank_create")
        self.variant, self.capacity = int(variant), int(capacity)
        self.conditions = [None] * self.capacity   # the Condition of every slot set so far (evaluate_grid_device observes under them)
        self._dev_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self._dev_index)
        h = C.c_void_p()
        _lib.check(create(self.variant, self._dev_index, self.capacity, C.byref(h)))
        self._h = h

    def close(self):
        if self._h is not None:
            self._L.qr_condition_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, slot, cond):
        """Slot `slot` in [0, capacity) <- `cond` (a Condition)."""
        gp, gy, sp = (np.ascontiguousarray(a, dtype=np.float32) for a in (cond.gate_pos, cond.gate_yaw, cond.start_pos))
        r = None if cond.disturbance_ranges is None else np.ascontiguousarray(cond.disturbance_ranges, dtype=np.float32)
        self._lib.check(self._L.qr_condition_bank_set(self._h, int(slot), _f32p(gp), _f32p(gy), int(gp.shape[0]), _f32p(sp),
                                                      None if r is None else _f32p(r), float(cond.disturbance_scale),
                                                      int(cond.max_steps), int(cond.gates_per_lap)))
        self.conditions[int(slot)] = cond
        return self


def plan_condition_groups(num_envs, num_conditions, envs_per_group=256, weights=None):
    """The blocked `condition_of_group` map of `env.rollout_policy_conditions_device` / `PPO(conditions=...)`: num_envs // envs_per_group
    groups, condition c holding a contiguous run of them.  weights None: equal shares; otherwise shares proportional to `weights`
    (one non-negative number per condition), rounded by largest remainder.  Groups that do not divide evenly go to the lowest indices
    (ties of the remainders likewise).  ValueError for sizes the library refuses (envs_per_group not a multiple of 256 or below it,
    num_envs not a whole number of groups) and when a condition would get no group (fewer groups than conditions, or a weight too
    small for one): a condition in the list is a condition to train on."""
    n, c, e = int(num_envs), int(num_conditions), int(envs_per_group)
    if c < 1:
        raise ValueError("num_conditions must be >= 1")
    if e < 256 or e % 256 != 0:
        raise ValueError("envs_per_group must be a multiple of 256, at least 256 (one workgroup serves one group)")
    if n < e or n % e != 0:
        raise ValueError("num_envs must be a whole number of groups of envs_per_group envs")
    groups = n // e
    if weights is None:
        w = [1.0] * c
    else:
        w = [float(x) for x in weights]
        if len(w) != c:
            raise ValueError("weights must hold one entry per condition")
        if any(not np.isfinite(x) or x < 0.0 for x in w) or sum(w) <= 0.0:
            raise ValueError("weights must be finite and non-negative, with a positive sum")
    total = sum(w)
    quota = [groups * x / total for x in w]
    share = [int(np.floor(q)) for q in quota]
    # largest remainder, ties to the lowest index (sorted is stable)
    for i in sorted(range(c), key=lambda i: -(quota[i] - share[i]))[:groups - sum(share)]:
        share[i] += 1
    if min(share) < 1:
        raise ValueError("%d group(s) for %d conditions with these weights leave condition %d without a group"
                         % (groups, c, share.index(min(share))))
    return [i for i in range(c) for _ in range(share[i])]
