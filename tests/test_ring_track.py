"""CPU: the machinery tests/test_gpu_table_edges.py and the lock-step tests rest on, checked on the oracle alone --
the ring track's straddle states do what they are built for (every gate index passed, the G-1 -> 0 wrap taken), and
parity.knife_edge_margin measures the distance from a termination threshold it is trusted to measure."""
import numpy as np
import pytest

import parity as P
from oracle_adapter import OracleAdapter

E2E, INDI = 0, 1


@pytest.mark.parametrize("G", [9, 31, 32])
@pytest.mark.parametrize("variant", [E2E, INDI])
def test_ring_straddle_states_pass_every_gate_and_wrap(variant, G, residual_blob):
    """n = 293 envs, one zero-action step, E2E with the residual model and the training disturbance ranges, and INDI, for
    gates_ahead 0 and 4: no env terminates, every target becomes (t + 1) % G, every gate index is passed, envs at gate G-1 wrap to 0;
    the next-gate block of the new observation is the relative table row of (t + 2 + a) % G -- a read across the wrap."""
    n = 293
    trk = P.ring_track(G)
    for ga in (0, 4):
        o = OracleAdapter(variant, n, trk, gates_ahead=ga, residual=residual_blob if variant == E2E else None,
                          dist_ranges=P.TRAIN_DIST_RANGES if variant == E2E else None, seed=1)
        w, d, t, s = P.ring_straddle_states(trk, n, o.env.state_len, seed=G)
        o.set_state(w, d, t, s)
        obs, rew, done, trunc = o.step(np.zeros((n, 4), np.float32))
        passes, wraps = P.ring_pass_census(trk, t, o.get_state()[2], done, rew)
        assert passes.sum() == n and wraps == len(range(G - 1, n, G)) and not trunc.any()
        pr, yr = o.env.track_tables()
        S = o.env.state_len
        for a in range(ga):
            idx = (t + 2 + a) % G
            np.testing.assert_array_equal(obs[:, S + 4 * a:S + 4 * a + 3], pr[idx])
            np.testing.assert_array_equal(obs[:, S + 4 * a + 3], yr[idx])


def _placed(variant, base, k, thr, away, eps, far):
    """A resting state whose coordinate k lies eps from `thr` on the `away` side, as float32: nudged by single float32 steps until
    the distance really is >= eps (far) or <= eps (near)."""
    s = np.zeros(16 if variant == E2E else 13, np.float32)
    s[0:3] = base
    s[k] = np.float32(thr + away * eps)
    while far and abs(float(s[k]) - thr) < eps:
        s[k] = np.nextafter(s[k], np.float32(away * np.inf))
    while not far and abs(float(s[k]) - thr) > eps:
        s[k] = np.nextafter(s[k], np.float32(thr))
    return s, abs(float(s[k]) - thr)


@pytest.mark.parametrize("variant", [E2E, INDI])
def test_knife_edge_margin_measures_the_distance_from_a_threshold(variant, residual_blob):
    """States at rest (an Euler step leaves a resting position unchanged: p_new = p + dt * 0), placed 1e-3 and 1e-6 from ONE
    threshold and far from every other: the margin is the placed distance -- >= 1e-3 there, <= 1e-6 here -- for the ground plane,
    the gate plane, the gate window and the position bound.  So the 1e-5 bound separates the two."""
    gate = (2.0, 1.0, -1.5, 0.0)                      # normal = +x; window |p - gate| < 0.5 per axis
    blob = residual_blob if variant == E2E else None
    a, d = np.zeros(4, np.float32), np.zeros(6, np.float32)
    cases = {"ground": ((0.0, 0.0, 0.0), 2, 0.0, -1), "plane": ((0.0, 3.0, -3.0), 0, 2.0, -1),
             "window": ((4.0, 0.0, -3.0), 1, 1.5, +1), "bound": ((5.0, 0.0, -3.0), 1, 10.0, -1)}
    for eps, far in ((1e-3, True), (1e-6, False)):
        for name, (base, k, thr, away) in cases.items():
            s, placed = _placed(variant, base, k, thr, away, eps, far)
            m = P.knife_edge_margin(variant, s, a, d, blob, gate)
            assert abs(m - placed) <= 1e-12, (name, eps, m, placed)      # it IS that distance
            assert (m >= 1e-3) if far else (0.0 < m <= 1e-6), (name, eps, m)
    assert 1e-6 < P.KNIFE_EDGE < 1e-3
