"""Plain NumPy restatement of the sensing model of qr_evaluate_policy_sensing_grid (include/quadrace.h), written from the model's text and
not from the kernel: which sigma an observation entry takes, the Philox counter and key of the observation noise on top of
tests/action_noise.py, and the command queue with its clear-on-done rule.

  slot     32 float32: sigma[0..7], the delay as an int32 bit pattern, zeros
  group    0 o[0..2] position | 1 o[3..5] velocity | 2 o[6..8] attitude | 3 o[9..11] rates | 4 o[12..S-1] actuator state |
           5 o[S+4a+0..2] gate a ahead, position | 6 o[S+4a+3] gate a ahead, yaw | 7 o[S+4GA..L-1] disturbance columns (E2E)
           S = 16 (E2E) / 13 (INDI), L = S + 4 GA (+ 4 for E2E)
  noise    o~[j] = o[j] + sigma[group(j)] * eps[j] in float32, the product rounded before the sum
           eps[4q..4q+3] = Box-Muller(uniforms(Philox4x32-10(counter, key)))     (action_noise.uniforms / box_muller)
           counter = (gid lo, gid hi, step lo, (step hi & 0xFFFFFF) | (q << 24)),  gid = env_id_base + index within the group,
           step = first_step + t < 2^56,  q < 9;     key = (seed lo ^ 0x6A09E667, seed hi ^ 0x3C6EF372)
  delay    d in [0, 4]: the env flies the command computed d steps earlier, (0, 0, 0, 0) for the first d steps of an episode; the step that
           ends an episode clears the queue.  Canonical order: queue[:, 4j..4j+3] = the command computed j + 1 steps ago, zeros for j >= d."""
import numpy as np

import action_noise as N

E2E, INDI = 0, 1
STATE_LEN = {E2E: 16, INDI: 13}
SLOT_FLOATS, SIGMAS, MAX_DELAY, QUEUE_FLOATS, MAX_BLOCKS, STEP_LIMIT = 32, 8, 4, 16, 9, 1 << 56
KEY_TWEAK = (0x6A09E667, 0x3C6EF372)


def obs_len(variant, ga):
    return STATE_LEN[variant] + 4 * ga + (4 if variant == E2E else 0)


def group_map(variant, ga):
    """[L] int: the sigma group of every observation entry"""
    S = STATE_LEN[variant]
    g = [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * (S - 12)
    for _ in range(ga):
        g += [5, 5, 5, 6]
    if variant == E2E:
        g += [7] * 4
    assert len(g) == obs_len(variant, ga)
    return np.asarray(g, np.int64)


GROUPS = {(v, ga): group_map(v, ga) for v in (E2E, INDI) for ga in range(5)}


def pack_slot(sigma8, delay):
    slot = np.zeros(SLOT_FLOATS, np.float32)
    slot[:SIGMAS] = np.asarray(sigma8, np.float32)
    slot[SIGMAS:SIGMAS + 1].view(np.int32)[0] = int(delay)
    return slot


def noise_key(noise_seed):
    s = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
    return (s & 0xFFFFFFFF) ^ KEY_TWEAK[0], (s >> 32) ^ KEY_TWEAK[1]


def num_blocks(L):
    return (L + 3) // 4


def noise_counter(E, K, Q, env_id_base=0, first_step=0, q_word=3):
    """The four counter words [K, E, Q] of group-local env e at step k and block q.  q_word: where q << 24 is OR-ed in (3 = the model;
    another word = a wrong neighbour for the tests' sensitivity checks)."""
    if int(first_step) + K > STEP_LIMIT:
        raise ValueError("first_step + num_steps > 2^56")
    g_lo, g_hi, s_lo, s_hi = (w[:, :, None] + np.zeros((K, E, Q), np.uint32) for w in N.noise_counter(E, K, env_id_base, first_step))
    words = [g_lo, g_hi, s_lo, s_hi & np.uint32(0xFFFFFF)]
    words[q_word] = words[q_word] | (np.arange(Q, dtype=np.uint32) << np.uint32(24))[None, None, :]
    return tuple(words)


def noise(L, E, K, noise_seed, env_id_base=0, first_step=0, swap_pairs=False, q_word=3, key=None):
    """eps [K, E, 4 Q] float64 (Q = ceil(L / 4): the entries past L are drawn and unused) and the uniforms (u1a, u2a, u1b, u2b), each
    [K, E, Q].  swap_pairs / q_word / key: wrong neighbours."""
    Q = num_blocks(L)
    assert Q <= MAX_BLOCKS
    k0, k1 = noise_key(noise_seed) if key is None else key
    x = N.philox4x32_10(*noise_counter(E, K, Q, env_id_base, first_step, q_word), k0, k1)
    if swap_pairs:
        x = (x[2], x[3], x[0], x[1])
    u = N.uniforms(x)
    eps, _, _ = N.box_muller(*u)                 # [K, E, Q, 4]
    return eps.reshape(K, E, 4 * Q), u


def perturb(o, sigma8, eps_rows, groups):
    """o~ = o + sigma[group] * eps in float32, two roundings.  o [.., L] float32, eps_rows [.., L] float32"""
    delta = np.asarray(sigma8, np.float32)[groups] * np.asarray(eps_rows, np.float32)
    return (np.asarray(o, np.float32) + delta).astype(np.float32)


class DelayQueue:
    """The command queues of n envs in canonical order, [n, 16] float32."""

    def __init__(self, n, delay, pending=None):
        if not 0 <= int(delay) <= MAX_DELAY:
            raise ValueError("delay outside [0, 4]")
        self.d = int(delay)
        self.q = np.zeros((n, QUEUE_FLOATS), np.float32) if pending is None else np.array(pending, np.float32).reshape(n, QUEUE_FLOATS)
        self.q[:, 4 * self.d:] = 0.0

    def exchange(self, command):
        """The command of this step goes in, the command the env flies this step comes out ([n, 4] each)."""
        a = np.asarray(command, np.float32)
        if self.d == 0:
            return a.copy()
        out = self.q[:, 4 * (self.d - 1):4 * self.d].copy()
        self.q[:, 4:4 * self.d] = self.q[:, :4 * (self.d - 1)].copy()
        self.q[:, :4] = a
        return out

    def clear(self, done):
        """called with the step's done flags, after the step"""
        self.q[np.asarray(done).astype(bool)] = 0.0

    def canonical(self):
        return self.q.copy()
