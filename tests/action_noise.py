"""Plain NumPy restatement of the closed-loop rollout's action noise (qr_rollout_policy, csrc/quadrace_env_kernels.hpp
rollout_policy_kernel), written from the spec and not from the kernel's arithmetic:

  counter = (gid lo, gid hi, step lo, step hi)    gid = env_id_base + i, step = first_step + k (64-bit values)
  key     = (seed lo ^ 0x9E3779B9, seed hi ^ 0x85EBCA6B)
  x       = Philox4x32-10(counter, key)
  u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1],   u2 = (x1 >> 8) * 2^-24 in [0, 1)   (and u1b, u2b from x2, x3; exact in float32)
  angle = float32(2 pi) * u2, ONE float32 product (the kernel's rounding; everything after it in float64)
  eps = (ra cos a, ra sin a, rb cos b, rb sin b),   r = sqrt(-2 ln u1)
  log-prob = -sum(log_std) - 2 ln(2 pi) - 0.5 * sum(eps^2)

Every function is vectorised over uint32 / uint64 arrays; products for mulhi / mullo are taken in uint64."""
import numpy as np

PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
NOISE_KEY_TWEAK = (0x9E3779B9, 0x85EBCA6B)
TWO_PI_F32 = np.float32(6.283185307179586)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on broadcastable uint32 arrays -> four uint32 arrays."""
    c = [np.asarray(x, np.uint32).astype(np.uint64) for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0 = np.asarray(k0, np.uint64) & _M32
    k1 = np.asarray(k1, np.uint64) & _M32
    for _ in range(10):
        p0 = PHILOX_M0 * c0
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0), (p1 & _M32), ((p0 >> _S32) ^ c3 ^ k1), (p0 & _M32)
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def noise_key(noise_seed):
    s = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
    return (s & 0xFFFFFFFF) ^ NOISE_KEY_TWEAK[0], (s >> 32) ^ NOISE_KEY_TWEAK[1]


def noise_counter(n, K, env_id_base=0, first_step=0):
    """The four counter words [K, n] of env i = 0..n-1 at step k = 0..K-1 (64-bit gid / step, split lo / hi)."""
    gid = np.uint64(int(env_id_base)) + np.arange(n, dtype=np.uint64)
    step = np.uint64(int(first_step)) + np.arange(K, dtype=np.uint64)
    lo = lambda v: (v & _M32).astype(np.uint32)
    hi = lambda v: (v >> _S32).astype(np.uint32)
    z = np.zeros((K, n), np.uint32)
    return lo(gid)[None, :] + z, hi(gid)[None, :] + z, lo(step)[:, None] + z, hi(step)[:, None] + z


def uniforms(x):
    """(u1a, u2a, u1b, u2b) from the Philox words; u1 in (0, 1] (no log(0)), u2 in [0, 1).  Exact in float32."""
    x0, x1, x2, x3 = x
    s = np.float32(2.0 ** -24)
    return (((x0 >> 8) + np.uint32(1)).astype(np.float32) * s, (x1 >> 8).astype(np.float32) * s,
            ((x2 >> 8) + np.uint32(1)).astype(np.float32) * s, (x3 >> 8).astype(np.float32) * s)


def box_muller(u1a, u2a, u1b, u2b):
    """eps [..., 4] in float64 and the radii (ra, rb); the angle is the float32 product the kernel forms."""
    def pair(u1, u2):
        r = np.sqrt(-2.0 * np.log(np.asarray(u1, np.float64)))
        a = (TWO_PI_F32 * np.asarray(u2, np.float32)).astype(np.float64)
        return r, r * np.cos(a), r * np.sin(a)
    ra, ca, sa = pair(u1a, u2a)
    rb, cb, sb = pair(u1b, u2b)
    return np.stack([ca, sa, cb, sb], axis=-1), ra, rb


def action_noise(n, K, noise_seed, env_id_base=0, first_step=0, swap_pairs=False):
    """Restated eps [K, n, 4] (float64) plus the uniforms (u1a, u2a, u1b, u2b) [K, n] it came from.
    swap_pairs: the wrong pairing (x0, x1) <-> (x2, x3), for the tests' sensitivity checks."""
    k0, k1 = noise_key(noise_seed)
    x = philox4x32_10(*noise_counter(n, K, env_id_base, first_step), k0, k1)
    if swap_pairs:
        x = (x[2], x[3], x[0], x[1])
    u = uniforms(x)
    eps, _, _ = box_muller(*u)
    return eps, u


def log_prob(eps, log_std):
    """Gaussian log-density of mean + std * eps, float64: -sum(log_std) - 2 ln(2 pi) - 0.5 sum eps^2."""
    ls = np.asarray(log_std, np.float64).reshape(4)
    return -ls.sum() - 2.0 * np.log(2.0 * np.pi) - 0.5 * (np.asarray(eps, np.float64) ** 2).sum(-1)
