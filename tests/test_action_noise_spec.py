"""CPU checks of the action-noise restatement (tests/action_noise.py) that the GPU tests pin the closed-loop rollout kernel to:
the vectorised Philox is Philox4x32-10 (Random123 known answers, the oracle's scalar C implementation on random and all-ones
words), the stream it defines is standard normal and independent across neighbouring envs and steps, and no two (gid, step)
share a counter, across the 2^32 carries included."""
import numpy as np

import action_noise as N
from oracle import oracle as O

KAT = [  # Random123 kat_vectors for philox4x32-10 (the same three as test_oracle_golden.py)
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_vectorised_philox_known_answers():
    ctr = np.array([c for c, _, _ in KAT], np.uint32)
    key = np.array([k for _, k, _ in KAT], np.uint32)
    out = np.stack(N.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    assert out.tolist() == [x for _, _, x in KAT]


def test_vectorised_philox_matches_oracle_on_random_words():
    rng = np.random.default_rng(20261016)
    m = 3000
    ctr = rng.integers(0, 2 ** 32, size=(m, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, size=(m, 2), dtype=np.uint64).astype(np.uint32)
    # all-ones and zero words in every position (the mulhi / carry extremes)
    ctr[:64] = np.where(rng.random((64, 4)) < 0.5, 0xFFFFFFFF, ctr[:64])
    key[:64] = np.where(rng.random((64, 2)) < 0.5, 0xFFFFFFFF, key[:64])
    ctr[64:96] = np.where(rng.random((32, 4)) < 0.5, 0, ctr[64:96])
    out = np.stack(N.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    ref = np.stack([O.philox(ctr[j], key[j]) for j in range(m)])
    assert np.array_equal(out, ref)


def test_key_and_counter_layout():
    k0, k1 = N.noise_key(7)
    assert (k0, k1) == (7 ^ 0x9E3779B9, 0x85EBCA6B)
    assert N.noise_key(2 ** 32 + 7) == (7 ^ 0x9E3779B9, 1 ^ 0x85EBCA6B)
    c0, c1, c2, c3 = N.noise_counter(3, 2, env_id_base=2 ** 32 - 2, first_step=2 ** 32 - 1)
    assert c0.tolist() == [[2 ** 32 - 2, 2 ** 32 - 1, 0]] * 2 and c1.tolist() == [[0, 0, 1]] * 2
    assert c2.tolist() == [[2 ** 32 - 1] * 3, [0] * 3] and c3.tolist() == [[0] * 3, [1] * 3]


def test_uniforms_are_exact_and_in_range():
    x = [np.array([0, 0xFF, 0xFFFFFFFF, 0x100], np.uint32)] * 4
    u1a, u2a, u1b, u2b = N.uniforms(x)
    assert u1a.dtype == np.float32 and u2a.dtype == np.float32
    assert u1a.tolist() == [2.0 ** -24, 2.0 ** -24, 1.0, 2.0 * 2.0 ** -24]
    assert u2a.tolist() == [0.0, 0.0, 1.0 - 2.0 ** -24, 2.0 ** -24]
    assert np.array_equal(u1a, u1b) and np.array_equal(u2a, u2b)


def test_restated_stream_is_standard_normal_and_independent():
    n, K = 65536, 16                                    # 4M draws
    eps, _ = N.action_noise(n, K, noise_seed=11, env_id_base=123, first_step=1000)
    e = eps.reshape(-1, 4)
    assert abs(e.mean()) < 2e-3 and abs(e.var() - 1.0) < 3e-3
    assert abs((e ** 4).mean() / e.var() ** 2 - 3.0) < 0.03          # Gaussian kurtosis
    assert abs(e.max()) < 6.0 and abs(e.min()) < 6.0               # r <= sqrt(-2 ln 2^-24) = 5.77
    c = np.corrcoef(e.T)
    assert np.abs(c - np.eye(4)).max() < 3e-3                       # components
    for c_ in range(4):
        assert abs(np.corrcoef(eps[:, :-1, c_].ravel(), eps[:, 1:, c_].ravel())[0, 1]) < 3e-3   # neighbouring env ids
        assert abs(np.corrcoef(eps[:-1, :, c_].ravel(), eps[1:, :, c_].ravel())[0, 1]) < 3e-3   # neighbouring steps
        assert abs(np.corrcoef(eps[:-1, :-1, c_].ravel(), eps[1:, 1:, c_].ravel())[0, 1]) < 3e-3
    # squares too: a shared uniform between neighbours would show in the radii, not in the signed values
    assert abs(np.corrcoef(eps[:, :-1, 0].ravel() ** 2 + eps[:, :-1, 1].ravel() ** 2,
                           eps[:, 1:, 0].ravel() ** 2 + eps[:, 1:, 1].ravel() ** 2)[0, 1]) < 3e-3


def test_log_prob_formula():
    rng = np.random.default_rng(3)
    eps = rng.standard_normal((1000, 4))
    ls = np.array([0.0, -0.5, 0.3, -3.0])
    std = np.exp(ls)
    x = std * eps
    ref = (-0.5 * (x / std) ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)).sum(-1)
    assert np.allclose(N.log_prob(eps, ls), ref, rtol=0, atol=1e-12)


def _pack(c):
    c0, c1, c2, c3 = (np.asarray(x, np.uint64).ravel() for x in c)
    return (c1 << np.uint64(32) | c0), (c3 << np.uint64(32) | c2)


def test_distinct_gid_step_never_share_a_counter():
    """The counter is (gid, step) as two 64-bit words: 64 x 64 (gid, step) pairs around each 2^32 carry map to distinct
    counters that decode back to the pair; a dropped carry would map gid 2^32 onto gid 0 (and step likewise)."""
    for base, first in [(0, 0), (2 ** 32 - 32, 0), (0, 2 ** 32 - 32), (2 ** 32 - 32, 2 ** 32 - 32), (2 ** 64 - 64, 2 ** 64 - 64)]:
        g, s = _pack(N.noise_counter(64, 64, base, first))
        assert len(set(zip(g.tolist(), s.tolist()))) == 64 * 64
        assert np.array_equal(g.reshape(64, 64)[0], (np.uint64(base) + np.arange(64, dtype=np.uint64)))
        assert np.array_equal(s.reshape(64, 64)[:, 0], (np.uint64(first) + np.arange(64, dtype=np.uint64)))
    # ... so the streams across a carry are distinct too: gid 2^32 vs gid 0, step 2^32 vs step 0
    a, _ = N.action_noise(4, 4, 5, env_id_base=2 ** 32)
    b, _ = N.action_noise(4, 4, 5, env_id_base=0)
    c, _ = N.action_noise(4, 4, 5, first_step=2 ** 32)
    assert not np.isclose(a, b).any() and not np.isclose(c, b).any()
    # and equal (gid, step) from different (base, first) splits give equal noise
    d, _ = N.action_noise(8, 4, 5, env_id_base=2 ** 32 - 4, first_step=2 ** 32 - 2)
    e, _ = N.action_noise(4, 2, 5, env_id_base=2 ** 32, first_step=2 ** 32)
    assert np.array_equal(d[2:, 4:], e)
