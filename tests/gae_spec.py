"""Plain NumPy float64 restatement of what qr_ppo_gae promises in include/quadrace.h, written from that contract (SB3's
RolloutBuffer.compute_returns_and_advantage plus collect_rollouts' time-limit bootstrap, and VecMonitor's episode sums) and not
from the kernel's arithmetic:

  r_t     = rew_t + gamma * term_val_t                    term_val = V(terminal obs) at time-limit ends, 0 elsewhere
  nt_t    = 1 - done_t                                    every done ends the episode: no bootstrap through the reset
  delta_t = r_t + gamma * V_{t+1} * nt_t - V_t            V_T = last_val
  A_t     = delta_t + gamma * lam * nt_t * A_{t+1}        A_T = 0
  ret_t   = A_t + V_t

gamma and lam reach the kernel as float32, so the restatement rounds them to float32 first and then works in float64.

The float32 error bound.  The same recursion on magnitudes,

  m_t = |rew_t| + gamma |term_val_t| + gamma |V_{t+1}| nt_t + |V_t|        M_t = m_t + gamma lam nt_t M_{t+1}

bounds |A_t| and every partial sum that ppo_gae_kernel forms on the way to it, so one float32 rounding of any of them costs at
most 2^-24 M_t, and bound = C * 2^-24 * M_t with C the number of roundings per step of the recursion.  The count, from the
kernel's expressions (nonterminal = 1 - done and every product with it are exact, done being 0 or 1):

  r     = fmaf(gamma, term_val, rew)                       1   (2 as a product and a sum; 0 without term_val)
  delta = r + gamma * next_val * nonterminal - v           3   gamma * next_val, the sum, the difference
                                                               (2 if the sum contracts to fma(gamma * next_val, nonterminal, r))
  last  = delta + gamma * lam * nonterminal * last         3   gamma * lam, the product with last, the sum
                                                               (2 if product and sum contract to one fma)

  contracted 1 + 2 + 2 = 5, uncontracted 2 + 3 + 3 = 8:   C = 8 covers both.   ret = last + v is one more rounding of a value
  no larger than M_t + |V_t|:   bound_ret = bound + 2^-24 (M_t + |V_t|).

This charges step t's roundings against M_t and carries the error of A_{t+1} into A_t through the same gamma lam nt factor as
M_{t+1}; it is first order in 2^-24 (a worst case that piles every rounding of a long episode in one direction grows with the
episode's length and is not what C counts)."""
import numpy as np

U32 = 2.0 ** -24      # unit roundoff of float32
C_ROUNDINGS = 8       # float32 roundings per recursion step of ppo_gae_kernel, uncontracted form (derivation above)
GATE_REWARD = 5.0     # a step reward above this is a gate pass (gate reward 10 - 10 * distance to the gate centre)


def _f64(x):
    return np.asarray(x, np.float64)


def gae(rew, done, val, last_val, term_val, gamma, lam):
    """-> adv [T, N], ret [T, N], bound [T, N] (float32 error bound of adv; see bound_ret for ret).  term_val may be None."""
    rew, done, val, last_val = _f64(rew), _f64(done), _f64(val), _f64(last_val)
    T, N = rew.shape
    tv = np.zeros_like(rew) if term_val is None else _f64(term_val)
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    adv, M = np.empty((T, N)), np.empty((T, N))
    a_next, m_next, v_next = np.zeros(N), np.zeros(N), last_val
    for t in range(T - 1, -1, -1):
        nt = 1.0 - done[t]
        delta = rew[t] + g * tv[t] + g * v_next * nt - val[t]
        a_next = delta + g * l * nt * a_next
        m_next = np.abs(rew[t]) + g * np.abs(tv[t]) + g * np.abs(v_next) * nt + np.abs(val[t]) + g * l * nt * m_next
        adv[t], M[t] = a_next, m_next
        v_next = val[t]
    return adv, adv + val, C_ROUNDINGS * U32 * M


def bound_ret(bound, val):
    """Error bound of ret = adv + val given adv's: one more rounding, of a value no larger than M_t + |V_t|."""
    return bound + U32 * (bound / (C_ROUNDINGS * U32) + np.abs(_f64(val)))


def episode_stats(rew, done, ep_ret, ep_len, ep_gates, ep_abs=None, ep_terms=None):
    """VecMonitor over a rollout [T, N] of RAW rewards, continuing the running episodes (ep_ret, ep_len, ep_gates) [N].
    -> (ep_ret, ep_len, ep_gates), fin[4] = {sum return, sum length, sum gates, episodes} over the episodes that finished,
       (ep_ret_bound [N], fin0_bound, fin0_terms, fin0_abs), (ep_abs, ep_terms).
    A float32 sum of n terms taken in any order is within 2^-24 * n * sum|terms| of the exact one; ep_abs / ep_terms carry
    sum|terms| and n of the running episodes from call to call (default: the carried return as one term).  fin0_terms and
    fin0_abs are those of everything that entered fin[0] in this call (every reward of a finished episode, plus one addition per
    finished episode for the reduction), so that a caller accumulating fin over calls can add them up."""
    rew, done = _f64(rew), _f64(done)
    er, el, eg = _f64(ep_ret).copy(), _f64(ep_len).copy(), _f64(ep_gates).copy()
    ea = np.abs(er) if ep_abs is None else _f64(ep_abs).copy()
    en = (er != 0).astype(np.float64) if ep_terms is None else _f64(ep_terms).copy()
    fin = np.zeros(4)
    fin_terms, fin_abs = 0.0, 0.0
    for t in range(rew.shape[0]):
        r, d = rew[t], done[t]
        er += r; el += 1.0; eg += (r > GATE_REWARD); ea += np.abs(r); en += 1.0
        fin += [np.sum(er * d), np.sum(el * d), np.sum(eg * d), np.sum(d)]
        fin_terms += np.sum((en + 1.0) * d); fin_abs += np.sum(ea * d)
        keep = 1.0 - d
        er *= keep; el *= keep; eg *= keep; ea *= keep; en *= keep
    return (er, el, eg), fin, (U32 * en * ea, U32 * fin_terms * fin_abs, fin_terms, fin_abs), (ea, en)


# ---- the input sets of tests/test_gpu_gae.py (the CPU test shows that they give every mutation of the rule room to show)
SHAPES = [(1, 1), (1, 257), (7, 63), (3, 64), (32, 1000), (48, 4096), (512, 100), (32, 65536)]
GAMMAS = [0.99, 0.999, 1.0]
LAMS = [0.0, 0.95, 1.0]
DONE_PATTERNS = ["none", "all", "row0", "rowlast", "random"]


def make_inputs(T, N, pattern, with_term, seed):
    """float32 rollout buffers: rewards ~ 0.3 N(0, 1) with 2 % gate passes at 9.5, values ~ 5 N(0, 1), V(terminal obs) uniform
    in +-50 on a random half of the dones (so that the bootstrap term dominates the reward), 0 elsewhere."""
    rng = np.random.default_rng([seed, T, N, DONE_PATTERNS.index(pattern), int(with_term)])
    rew = (0.3 * rng.standard_normal((T, N))).astype(np.float32)
    rew[rng.random((T, N)) < 0.02] = 9.5
    val = (5.0 * rng.standard_normal((T, N))).astype(np.float32)
    last_val = (5.0 * rng.standard_normal(N)).astype(np.float32)
    done = np.zeros((T, N), np.float32)
    if pattern == "all":
        done[:] = 1.0
    elif pattern == "row0":
        done[0] = 1.0
    elif pattern == "rowlast":
        done[T - 1] = 1.0
    elif pattern == "random":
        done[rng.random((T, N)) < 0.05] = 1.0
    term_val = None
    if with_term:
        trunc = (done > 0) & (rng.random((T, N)) < 0.5)
        term_val = np.where(trunc, rng.uniform(-50.0, 50.0, (T, N)), 0.0).astype(np.float32)
    return rew, done, val, last_val, term_val
