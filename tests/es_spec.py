"""Plain NumPy restatement of the evolution-strategies entry points (qr_es_*, include/quadrace.h), written from the header's text and not
from the kernels' arithmetic: the noise stream, the antithetic members, the per-policy summary with its stated summation order, the
score, the ranks and utilities, and the Adam-ascent update.  Every float32 product and sum is a separately rounded NumPy float32
operation in the order the header states; the score is float64 in the order written.

  noise    x = Philox4x32-10(counter = (q, i, g lo, g hi), key = (seed lo ^ 0x2545F491, seed hi ^ 0x4F6CDD1D)) gives parameters
           4q .. 4q + 3 of pair i in generation g; uniforms and Box-Muller are tests/action_noise.py's (float64 from exact float32 uniforms and
           the float32 angle product): the device's float32 eps is held against it with a tolerance, everything after the noise bit for bit
           from the device's own eps
  members  member 2i = theta + (sigma * eps_i), member 2i + 1 = theta - (sigma * eps_i)
"""
import math

import numpy as np

import action_noise as N

ES_KEY_TWEAK = (0x2545F491, 0x4F6CDD1D)
SHAPE_CENTERED_RANK, SHAPE_NONE = 0, 1
REC_INTS, REC_FLOATS = 24, 4
f32 = np.float32


def num_params(obs_len):
    """the actor block pi: w1 b1 w2 b2 w3 b3 w4 b4"""
    return 120 * int(obs_len) + 120 + 2 * (120 * 120 + 120) + 4 * 120 + 4


def es_key(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (s & 0xFFFFFFFF) ^ ES_KEY_TWEAK[0], (s >> 32) ^ ES_KEY_TWEAK[1]


def noise(n, pairs, seed, generation, first_pair=0, swap_pairs=False):
    """eps [pairs, n] float64 and the uniforms (u1a, u2a, u1b, u2b), each [pairs, n / 4], of pairs first_pair .. first_pair + pairs - 1.
    swap_pairs: the wrong pairing (x0, x1) <-> (x2, x3), for the sensitivity checks."""
    assert n % 4 == 0
    g = int(generation) & 0xFFFFFFFFFFFFFFFF
    q = np.arange(n // 4, dtype=np.uint32)[None, :]
    i = (np.arange(pairs, dtype=np.int64) + int(first_pair)).astype(np.uint32)[:, None]
    z = np.zeros((pairs, n // 4), np.uint32)
    k0, k1 = es_key(seed)
    x = N.philox4x32_10(q + z, i + z, z + np.uint32(g & 0xFFFFFFFF), z + np.uint32(g >> 32), k0, k1)
    if swap_pairs:
        x = (x[2], x[3], x[0], x[1])
    u = N.uniforms(x)
    eps, _, _ = N.box_muller(*u)
    return eps.reshape(pairs, n), u


def members(theta, sigma, eps):
    """[2 pairs, n] float32 from theta [n] and eps [pairs, n] (float32: the device's own): two separately rounded operations each"""
    theta, eps = np.asarray(theta, f32), np.asarray(eps, f32)
    d = f32(sigma) * eps
    pop = np.empty((2 * eps.shape[0], theta.size), f32)
    pop[0::2] = theta[None, :] + d
    pop[1::2] = theta[None, :] - d
    return pop


def summary(rec, recf, envs_per_policy):
    """[P, 8] float64 from rec [P E, 24] int32 and recf [P E, 4] float32 or None.  s7: chunks of 256 envs, a halving tree inside a chunk,
    the chunks added in ascending order."""
    E = int(envs_per_policy)
    rec = np.asarray(rec).astype(np.int64).reshape(-1, E, REC_INTS)
    P = rec.shape[0]
    out = np.zeros((P, 8), np.float64)
    out[:, 0], out[:, 1], out[:, 2] = rec[:, :, 0].sum(1), rec[:, :, 1].sum(1), rec[:, :, 2].sum(1)
    out[:, 3], out[:, 4] = rec[:, :, 14].sum(1), rec[:, :, 6].sum(1)
    out[:, 5], out[:, 6] = rec[:, :, 15:22].sum((1, 2)), rec[:, :, 7:14].sum((1, 2))
    if recf is not None:
        recf = np.asarray(recf, f32).reshape(P, E, REC_FLOATS)
        for p in range(P):
            total = np.float64(0.0)
            for c in range(E // 256):
                rows = recf[p, 256 * c:256 * (c + 1)]
                x = rows[:, 1].astype(np.float64) + rows[:, 0].astype(np.float64)
                off = 128
                while off >= 1:
                    x[:off] = x[:off] + x[off:2 * off]
                    off //= 2
                total = total + x[0]
            out[p, 7] = total
    return out


def score(s, w, envs_per_policy):
    """[P] float64: (w_gate s0 + w_crash s1 + w_timeout s2 + w_return s7) / E + w_lap * (s5 > 0 ? s6 / s5 : no_lap_steps).
    w = dict(w_gate, w_crash, w_timeout, w_return, w_lap, no_lap_steps)."""
    s = np.asarray(s, np.float64)
    d = lambda k: np.float64(w[k])
    with np.errstate(divide="ignore", invalid="ignore"):
        lap = np.where(s[:, 5] > 0, s[:, 6] / np.where(s[:, 5] > 0, s[:, 5], 1.0), d("no_lap_steps"))
    acc = d("w_gate") * s[:, 0]
    acc = acc + d("w_crash") * s[:, 1]
    acc = acc + d("w_timeout") * s[:, 2]
    acc = acc + d("w_return") * s[:, 7]
    return acc / np.float64(int(envs_per_policy)) + d("w_lap") * lap


def ranks(F):
    """rank_p = #{q : F_q < F_p} + #{q < p : F_q == F_p}; a NaN ranks below everything, NaNs among themselves by index"""
    F = [float(x) for x in np.asarray(F, np.float64)]
    less = lambda a, b: (not math.isnan(b)) if math.isnan(a) else a < b
    same = lambda a, b: math.isnan(b) if math.isnan(a) else a == b
    return np.array([sum(1 for q in range(len(F)) if less(F[q], F[p]) or (q < p and same(F[q], F[p]))) for p in range(len(F))], np.int64)


def utilities(F, shaping):
    F = np.asarray(F, np.float64)
    if shaping == SHAPE_CENTERED_RANK:
        return ranks(F).astype(f32) / f32(F.size - 1) - f32(0.5)
    assert shaping == SHAPE_NONE
    with np.errstate(over="ignore"):
        return F.astype(f32)


def bias_corrections(beta1, beta2, t):
    c = lambda b: f32(1.0 / (1.0 - math.pow(float(f32(b)), float(int(t)))))
    return c(beta1), c(beta2)


def update(theta, m, v, F, eps, sigma, shaping, lr, beta1, beta2, adam_eps, weight_decay, adam_step):
    """(theta, m, v, u) after one qr_es_update: eps [pairs, n] float32 (the device's own), everything float32, one rounding per operation."""
    theta, m, v, eps = (np.array(a, f32) for a in (theta, m, v, eps))
    pairs = eps.shape[0]
    u = utilities(F, shaping).astype(f32)
    lr, b1, b2, ae, wd = f32(lr), f32(beta1), f32(beta2), f32(adam_eps), f32(weight_decay)
    c1, c2 = bias_corrections(beta1, beta2, adam_step)
    with np.errstate(all="ignore"):
        g = np.zeros_like(theta)
        for i in range(pairs):
            d = f32(u[2 * i] - u[2 * i + 1])
            g = g + d * eps[i]
        g = g * (f32(1.0) / (f32(2 * pairs) * f32(sigma)))
        g = g - wd * theta
        m = b1 * m + (f32(1.0) - b1) * g
        v = b2 * v + ((f32(1.0) - b2) * g) * g
        theta = theta + (lr * (m * c1)) / (np.sqrt(v * c2) + ae)
    assert theta.dtype == f32 and m.dtype == f32 and v.dtype == f32 and g.dtype == f32
    return theta, m, v, u


def lap_weights(n_eval_steps, crash_steps):
    """the weights fitness="lap" stands for: minus the mean flying-lap steps, a crash costing crash_steps steps"""
    return dict(w_gate=0.0, w_crash=-float(crash_steps), w_timeout=0.0, w_return=0.0, w_lap=-1.0, no_lap_steps=float(n_eval_steps))


# ---- the synthetic ascent problem of tests/test_es_host.py and tests/test_gpu_es.py ------------------------------------------------------
# F_p = -|theta_p[:K] - target|^2 with QR_ES_SHAPE_CENTERED_RANK: only the first K parameters carry signal, so 2 x 8 members see it in any
# n.  Settings chosen with this restatement alone, on the CPU: they take |theta[:K] - target| from 3.52 to about 1.3 (theta[:K] = 0 at start).
ASCENT = dict(K=64, pairs=8, sigma=0.1, lr=0.03, generations=40, seed=11, betas=(0.9, 0.999), eps=1e-8)


def ascent_offset():
    """target - theta[:K] at the start"""
    return (0.5 * np.cos(np.arange(ASCENT["K"]) * 1.7)).astype(f32) + f32(0.25)


def ascent_score(pop, target):
    """[P] float64 from the members [P, n]: minus the squared distance of their first K parameters to the target"""
    return -((np.asarray(pop, np.float64)[:, :ASCENT["K"]] - np.asarray(target, np.float64)) ** 2).sum(1)
