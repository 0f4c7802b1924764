"""CPU checks of the GAE restatement (tests/gae_spec.py) that tests/test_gpu_gae.py pins qr_ppo_gae to: the recursion equals the
definition A_t = sum_l (gamma lam)^l delta_{t+l} summed episode by episode, the episode statistics equal a per-env walk, and
every way the rule is commonly got wrong moves some element by more than the float32 bound on the GPU test's own inputs --
so a kernel with that mistake cannot hide inside the bound."""
import numpy as np
import pytest

import gae_spec as G


def _brute_force(rew, done, val, last_val, term_val, gamma, lam):
    """The definition, one (t, env) at a time: the discounted sum of TD residuals up to the end of the episode t lies in."""
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    T, N = rew.shape
    adv = np.zeros((T, N))
    for i in range(N):
        for t in range(T):
            acc, w = 0.0, 1.0
            for s in range(t, T):
                ended = done[s, i] > 0
                v_next = 0.0 if ended else (float(last_val[i]) if s == T - 1 else float(val[s + 1, i]))
                r = float(rew[s, i]) + (g * float(term_val[s, i]) if term_val is not None else 0.0)
                acc += w * (r + g * v_next - float(val[s, i]))
                if ended:
                    break
                w *= g * l
            adv[t, i] = acc
    return adv


@pytest.mark.parametrize("T,N", [(1, 1), (1, 5), (7, 6), (12, 9)])
@pytest.mark.parametrize("pattern", G.DONE_PATTERNS)
def test_recursion_equals_the_definition(T, N, pattern):
    for gamma, lam in [(0.99, 0.95), (1.0, 1.0), (0.999, 0.0)]:
        for with_term in (False, True):
            rew, done, val, last_val, tv = G.make_inputs(T, N, pattern, with_term, seed=3)
            if pattern == "random":
                done = (np.random.default_rng(T * N).random((T, N)) < 0.3).astype(np.float32)   # several ends per env at this size
                tv = None if tv is None else np.where(done > 0, np.float32(7.5), np.float32(0))
            adv, ret, bound = G.gae(rew, done, val, last_val, tv, gamma, lam)
            ref = _brute_force(rew, done, val, last_val, tv, gamma, lam)
            assert np.abs(adv - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
            assert np.array_equal(ret, adv + val.astype(np.float64))
            assert (bound > 0).all() and (G.bound_ret(bound, val) > bound).all()
            assert (np.abs(adv) <= bound / (G.C_ROUNDINGS * G.U32) * (1 + 1e-12)).all()   # M_t bounds |A_t|


def test_episode_stats_equal_a_per_env_walk():
    rng = np.random.default_rng(11)
    T, N = 40, 23
    rew = rng.standard_normal((T, N)).astype(np.float32)
    rew[rng.random((T, N)) < 0.1] = 9.5
    done = (rng.random((T, N)) < 0.15).astype(np.float32)
    state = (np.zeros(N), np.zeros(N), np.zeros(N))
    aux, total = (None, None), np.zeros(4)
    walk = np.zeros(4)
    run = [[0.0, 0, 0] for _ in range(N)]
    for call in range(2):                                   # state carried across calls
        state, fin, (b_ret, b_fin, n_fin, a_fin), aux = G.episode_stats(rew, done, *state, *aux)
        total += fin
        for i in range(N):
            for t in range(T):
                run[i][0] += float(rew[t, i]); run[i][1] += 1; run[i][2] += int(rew[t, i] > 5.0)
                if done[t, i] > 0:
                    walk += [run[i][0], run[i][1], run[i][2], 1]
                    run[i] = [0.0, 0, 0]
        assert np.allclose(state[0], [r[0] for r in run], atol=1e-12)
        assert np.array_equal(state[1], [r[1] for r in run]) and np.array_equal(state[2], [r[2] for r in run])
        assert abs(total[0] - walk[0]) < 1e-9 and np.array_equal(total[1:], walk[1:])
        assert (b_ret >= 0).all() and b_fin > 0 and n_fin >= fin[1] and a_fin >= abs(fin[0])
    quiet = np.zeros((T, N), np.float32)
    _, fin, (_, b_fin, n_fin, a_fin), _ = G.episode_stats(rew, quiet, *state, *aux)
    assert not fin.any() and b_fin == 0 and n_fin == 0 and a_fin == 0     # nothing finished: nothing to accumulate


# ---- the rule, got wrong five ways
def _mutated(which, rew, done, val, last_val, term_val, gamma, lam):
    rew, done, val, last_val = (np.asarray(x, np.float64) for x in (rew, done, val, last_val))
    tv = np.zeros_like(rew) if term_val is None else np.asarray(term_val, np.float64)
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    if which == "lam_gamma_swapped":
        g, l = l, g
    T, N = rew.shape
    adv = np.empty((T, N))
    a_next = np.zeros(N)
    v_next = np.zeros(N) if which == "last_val_ignored" else last_val
    for t in range(T - 1, -1, -1):
        d = done[t]
        if which == "done_of_next_row":
            d = done[t + 1] if t + 1 < T else np.zeros(N)
        if which == "truncation_continues":          # a time-limit end bootstraps through the reset instead of from term_val
            d = np.where(tv[t] != 0, 0.0, d)
            r = rew[t]
        elif which == "term_val_without_gamma":
            r = rew[t] + tv[t]
        else:
            r = rew[t] + g * tv[t]
        nt = 1.0 - d
        a_next = r + g * v_next * nt - val[t] + g * l * nt * a_next
        adv[t] = a_next
        v_next = val[t]
    return adv


def _observable(which, T, done, term_val, gamma, lam):
    """Whether the inputs give the mistake anything to act on (a rule about truncations cannot show without one, ...)."""
    g, l = np.float32(gamma), np.float32(lam)
    if which == "truncation_continues":
        return term_val is not None and bool((term_val != 0).any())
    if which == "term_val_without_gamma":
        return term_val is not None and bool((term_val != 0).any()) and g != 1
    if which == "done_of_next_row":
        shifted = np.vstack([done[1:], np.zeros((1, done.shape[1]), done.dtype)])
        return bool((shifted != done).any())
    if which == "last_val_ignored":
        return bool((done[T - 1] == 0).any())
    if which == "lam_gamma_swapped":
        return g != l and (bool((done == 0).any()) or (term_val is not None and bool((term_val != 0).any())))
    raise KeyError(which)


MUTATIONS = ["truncation_continues", "term_val_without_gamma", "done_of_next_row", "last_val_ignored", "lam_gamma_swapped"]


@pytest.mark.parametrize("T,N", [s for s in G.SHAPES if s[0] * s[1] <= 48 * 4096])
def test_every_mutation_leaves_the_bound_on_the_gpu_tests_inputs(T, N):
    """On each input set of test_gpu_gae.py where a mistake has something to act on, it moves at least one element by more than
    that element's bound; and each mistake is observable on at least one set per shape with T > 1."""
    seen = dict.fromkeys(MUTATIONS, 0)
    for pattern in G.DONE_PATTERNS:
        for with_term in (False, True):
            rew, done, val, last_val, tv = G.make_inputs(T, N, pattern, with_term, seed=0)
            for gamma in G.GAMMAS:
                for lam in G.LAMS:
                    adv, _, bound = G.gae(rew, done, val, last_val, tv, gamma, lam)
                    for which in MUTATIONS:
                        if not _observable(which, T, done, tv, gamma, lam):
                            continue
                        bad = _mutated(which, rew, done, val, last_val, tv, gamma, lam)
                        excess = (np.abs(bad - adv) / bound).max()
                        assert excess > 1.0, (which, pattern, with_term, gamma, lam, excess)
                        seen[which] += 1
    if T > 1 and N > 1:
        assert all(seen.values()), seen
