"""The COMMAND HISTORY of qr_rollout_policy_history / qr_evaluate_policy_history_grid (include/quadrace.h), restated as pure functions on
the canonical command queue `pending` [n][16]: entry j = columns 4j .. 4j+3 = the clipped command computed j + 1 steps ago in the current
episode, zeros behind max(d, H).  d = the command delay of the env's sensing slot, H = the command history of the launch.

    row(o_tilde, queue, H)                 the policy's row at a step: [ noisy observation | entries 0 .. H-1 of the queue ]
    push(queue, cmd, d, H) -> (fly, q')    the step's clipped command enters in front; `fly` is what the env steps with (cmd itself for
                                           d = 0, else entry d - 1 of the queue BEFORE the push); q' keeps max(d, H) entries
    clear(queue, done)                     the step that ends an episode clears the queue (and with it the history)
    terminal_row(o_clean, queue, H)        the terminal-observation row of a step that ended an episode, from the queue AFTER that step's
                                           push and BEFORE its clear: [ clean terminal observation | u_k, u_{k-1}, ..., u_{k-H+1} ]

One step of the per-step loops in tests/test_gpu_command_history.py:
    seen = row(obs + noise[k], queue, H); cmd = clip(policy(seen)); fly, queue = push(queue, cmd, d, H); step(fly);
    [terminal_row(...) where done]; queue = clear(queue, done)
The functions use slicing and concatenation only, so they take NumPy arrays (tests/test_command_history_host.py) and torch tensors (the GPU
loops) alike and never modify their arguments."""
import numpy as np

QUEUE_FLOATS, MAX_DELAY = 16, 4


def _is_numpy(x):
    return isinstance(x, np.ndarray)


def _copy(x):
    return x.copy() if _is_numpy(x) else x.clone()


def _zeros_like(x):
    if _is_numpy(x):
        return np.zeros_like(x)
    import torch

    return torch.zeros_like(x)


def _cat(parts):
    if _is_numpy(parts[0]):
        return np.concatenate(parts, axis=1)
    import torch

    return torch.cat(parts, dim=1)


def _check(queue, d, H):
    assert queue.shape[1] == QUEUE_FLOATS and 0 <= d <= MAX_DELAY and 0 <= H <= MAX_DELAY, (queue.shape, d, H)


def row(o_tilde, queue, H):
    _check(queue, 0, H)
    return _cat([o_tilde, queue[:, :4 * H]])


def push(queue, cmd, d, H):
    _check(queue, d, H)
    fly = _copy(cmd) if d == 0 else _copy(queue[:, 4 * (d - 1):4 * d])
    m = max(d, H)
    out = _zeros_like(queue)
    if m > 0:
        out[:, 4:4 * m] = queue[:, :4 * (m - 1)]
        out[:, :4] = cmd
    return fly, out


def clear(queue, done):
    out = _copy(queue)
    out[done.astype(bool) if _is_numpy(done) else done.bool()] = 0.0
    return out


def terminal_row(o_clean, queue, H):
    _check(queue, 0, H)
    return _cat([o_clean, queue[:, :4 * H]])


# ---- observation lengths (csrc/quadrace_env_kernels.hpp obs_len<V, GA>, csrc/quadrace_launch.hpp dispatch_L) -----------------------------
def obs_len(variant, gates_ahead):
    """variant 0 = E2E (16 state entries, 4 disturbance columns), 1 = INDI (13 state entries)"""
    return (20 if variant == 0 else 13) + 4 * gates_ahead


POLICY_LENGTHS = frozenset([13 + 4 * g for g in range(5)] + [20 + 4 * g for g in range(5)] + [16])
