"""The host code every closed-loop launch shares: what vec_env.py, quad3d.py, evaluation.py, recording.py and blackbox.py would
otherwise each carry a copy of.  Argument conversion and checks for the `*_policy_device` methods of the envs, the reading of a model
(actor, log_std, collect precision), `flying_policy` (one policy on one env: the single-policy evaluators, the recorder, the black box)
and `fly_batches` (the step loop of the banked evaluators).  Nothing here calls the library or knows a kernel: the env methods do.
Importing this module needs neither torch nor a GPU."""
import contextlib
import ctypes as C

import numpy as np


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _precision_flags(precision):
    """Flag bits of the policy forward's precision (QR_ROLLOUT_F32CLASS for "f32")."""
    if precision not in ("f16-operands", "f32"):
        raise ValueError("precision must be 'f16-operands' or 'f32'")
    return 2 if precision == "f32" else 0


def _host(a):
    """tensor, array or None -> NumPy array on the host, or None"""
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def log_std_array(log_std):
    """`log_std` (tensor, array or sequence of 4 values) as the contiguous float32 [4] host array the library reads."""
    return np.ascontiguousarray(_host(log_std), dtype=np.float32).reshape(4)


def log_std_rows(log_stds, num_groups):
    """log_std_array's twin for a population launch: `log_stds` (a [G][4] tensor or array, or a sequence of G entries log_std_array
    takes) as the contiguous float32 [G, 4] host array the library reads, G = num_groups."""
    g = int(num_groups)
    if hasattr(log_stds, "detach") or isinstance(log_stds, np.ndarray):
        rows = np.ascontiguousarray(_host(log_stds), dtype=np.float32)
    else:
        rows = np.stack([log_std_array(r) for r in log_stds]) if len(log_stds) else np.zeros((0, 4), np.float32)
    if rows.shape != (g, 4):
        raise ValueError("log_stds must hold one row of 4 values per group (%d groups)" % g)
    return np.ascontiguousarray(rows)


def noise_seed_array(noise_seeds, num_groups):
    """One action-noise seed per group as the contiguous uint64 [G] host array the library reads."""
    seeds = np.array([int(s) & (2 ** 64 - 1) for s in noise_seeds], dtype=np.uint64)
    if seeds.shape != (int(num_groups),):
        raise ValueError("noise_seeds must hold one seed per group (%d groups)" % int(num_groups))
    return seeds


def rollout_outputs(K, n, obs_len, device):
    """Fresh (obs[K,n,obs_len], actions[K,n,4], logp[K,n], reward[K,n], done[K,n] u8, trunc[K,n] u8) of a closed-loop rollout."""
    import torch

    f32 = dict(dtype=torch.float32, device=device)
    u8 = dict(dtype=torch.uint8, device=device)
    return (torch.empty((K, n, obs_len), **f32), torch.empty((K, n, 4), **f32), torch.empty((K, n), **f32), torch.empty((K, n), **f32),
            torch.empty((K, n), **u8), torch.empty((K, n), **u8))


def zero_records(n, widths, device):
    """Fresh evaluation records (rec int32 [n, widths[0]], recf float32 [n, widths[1]]), zeroed."""
    import torch

    return (torch.zeros((n, widths[0]), dtype=torch.int32, device=device), torch.zeros((n, widths[1]), dtype=torch.float32, device=device))


def check_records(rec, recf, n, widths, exc, device=None):
    """The evaluators' record tensors: `rec` int32 [n, widths[0]], `recf` float32 [n, widths[1]] or None, both contiguous and on the
    device (on `device` itself where one is given).  Raises `exc`."""
    import torch

    for name, t, dtype, width in (("rec", rec, torch.int32, widths[0]), ("recf", recf, torch.float32, widths[1])):
        if t is None and name == "recf":
            continue
        if not (torch.is_tensor(t) and t.is_cuda and (device is None or t.device == device) and t.dtype == dtype and t.is_contiguous()
                and tuple(t.shape) == (n, width)):
            raise exc("%s must be a contiguous %s tensor [num_envs, %d] on the env's device" % (name, dtype, width))


# ---- reading a model ---------------------------------------------------------------------------------------------------------------
def _model_precision(models):
    """The precision a model (or a list of models; None entries are bare actors) collects in: "f32" if any does, else "f16-operands"."""
    if not isinstance(models, (list, tuple)):
        models = [models]
    f32 = any(getattr(m, "precision", None) in ("f32", "f32-collect") or getattr(m, "policy_forward", None) == "f32class" for m in models)
    return "f32" if f32 else "f16-operands"


def _net(model):
    """the torch ActorCritic of the SB3-shaped PPO (sb3.PPO) or of the native trainer (ppo.PPO)"""
    net = getattr(model, "_net", None)
    if net is None:
        net = model.policy
    return getattr(net, "net", net)   # sb3.ActorCriticPolicy wraps the ActorCritic


def _actor(model):
    """the torch actor (Linear, ReLU, ..., Linear) of the SB3-shaped PPO (sb3.PPO) or of the native trainer (ppo.PPO)"""
    return _net(model).pi


def model_log_std(model):
    """The log_std [4] a model samples with; zeros for a net without one and for a bare actor (`model` None)."""
    import torch

    net = None if model is None else _net(model)
    return net.log_std.detach() if hasattr(net, "log_std") else torch.zeros(4)


def _as_actor(entry):
    """(torch actor, model or None) of one policy entry: a checkpoint path written by `model.save`, an SB3-shaped PPO, a native
    trainer, or a bare torch actor (Linear, ReLU, ..., Linear)."""
    import os

    import torch

    if isinstance(entry, (str, os.PathLike)):
        from .sb3 import PPO

        entry = PPO.load(os.fspath(entry))   # needs no env
    if isinstance(entry, torch.nn.Module) and not hasattr(entry, "pi") and not hasattr(entry, "net"):
        return entry, None
    return _actor(entry), entry


# ---- one policy on one env -----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def flying_policy(model, env, precision=None, seed=None):
    """`with flying_policy(model, env, precision, seed) as (core, policy, precision, owner)`: the env inside its wrappers, `model`'s
    actor (any entry _as_actor takes) loaded into an MfmaPolicy on the env's device, the precision resolved (None: the model's own
    collect precision) and the model itself (None for a bare actor).  `seed` not None: the env is reseeded and reset first.  On exit
    the stream is synchronised and the policy closed."""
    import torch

    from .policy import MfmaPolicy
    from .sb3 import _unwrap

    core = _unwrap(env)
    actor, owner = _as_actor(model)
    if precision is None:
        precision = _model_precision(owner)
    policy = MfmaPolicy(core.state_len, core.device.index).load_torch(actor)
    try:
        if seed is not None:
            core.seed(seed)
            core.reset_device()
        yield core, policy, precision, owner
    finally:
        torch.cuda.current_stream(core.device).synchronize()
        policy.close()


# ---- a bank of policies, a launch of `slots` groups at a time ------------------------------------------------------------------------
def group_size(envs_per_group, num_envs, what, unit):
    """E = `envs_per_group` (the caller's argument `what`, serving one `unit` per workgroup) checked against the env; returns (E, slots)."""
    E, n = int(envs_per_group), int(num_envs)
    if E < 256 or E % 256 != 0:
        raise ValueError("%s must be a multiple of 256 (one workgroup serves one %s)" % (what, unit))
    if n % E != 0:
        raise ValueError("env.num_envs must be a multiple of %s" % what)
    return E, n // E


def fly_batches(plan, start, launch, phases, widths, summarise, num_envs, envs_per_group, device):
    """The step loop of the banked evaluators.  Per batch (members, kept) of `plan` (plan_policy_batches / plan_grid_batches):
    `start(members)` loads the slots and gives the env its starts; the records are zeroed (`widths` = their two widths, on `device`);
    then per entry of `phases` (step counts) `launch(members, steps, rec, recf)` continues the same records and
    `summarise(member, rec rows, recf rows)` is taken of each of the `kept` leading groups BEFORE the next launch.  Padded groups fly
    but are never summarised.  Returns [(member, [summary per phase]), ...] in plan order.  Synchronising and closing the banks is
    the caller's; nothing here needs a GPU."""
    E, out = int(envs_per_group), []
    for members, kept in plan:
        start(members)
        rec, recf = zero_records(num_envs, widths, device)
        per_phase = []
        for steps in phases:
            launch(members, steps, rec, recf)
            per_phase.append([summarise(members[g], rec[g * E:(g + 1) * E], recf[g * E:(g + 1) * E]) for g in range(kept)])
        out.extend((members[g], [summaries[g] for summaries in per_phase]) for g in range(kept))
    return out
