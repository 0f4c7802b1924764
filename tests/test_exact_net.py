"""CPU checks of the exact-arithmetic network fixture (tests/exact_net.py) that the bit-exact GPU forward tests rest on: its results do
not depend on the summation order, its networks are non-degenerate, and its float64 restatement tells apart the kernel bugs the GPU
tests are meant to catch."""
import numpy as np
import pytest

import exact_net as E

SEEDS = (1, 2, 3)


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_float32_accumulation_in_any_order_equals_float64(L):
    rng = np.random.default_rng(L)
    for seed, out in ((1, 4), (2, 1)):
        net, obs = E.make_net(L, seed, out), E.make_obs(257, L, seed)
        want = E.forward64(net, obs)
        assert np.array_equal(want, want.astype(np.float32).astype(np.float64))   # the float32 output is the exact value
        for _ in range(3):
            got = E.forward32_in_order(net, obs, rng)
            assert np.array_equal(got, want)
        # the guarantee behind it: every term on the layer's grid, sum |terms| well inside 2^24 grid steps (65 536 rows)
        for k, (margin, on_grid) in enumerate(E.exactness_margin(net, E.make_obs(65536, L, seed))):
            assert on_grid and margin < 0.75, (k, margin)


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_operands_are_f16_exact_normal_and_layers_two_and_three_round(L):
    for seed, out in ((1, 4), (2, 1)):
        net, obs = E.make_net(L, seed, out), E.make_obs(1000, L, seed)
        for k in range(4):
            xa, wa = E.layer_terms(net, obs, k)
            for a in (xa, wa):
                assert np.array_equal(E.to_f16(a), a)                        # f16-exact (hidden operands: after the kernel's rounding)
                nz = np.abs(a[a != 0])
                assert nz.min() >= E.F16_MIN_NORMAL and nz.max() <= E.F16_MAX   # no f16 subnormal, no saturation
            if k in (1, 2):
                pre = E.layer_terms(net, obs, k + 1)[0][:, :-1]
                raw = (xa @ wa.T)
                rounded = (E.to_f16(raw) != raw) & (raw > 0)
                assert rounded.mean() > 0.05, (k, rounded.mean())              # the rounding mode matters
                assert np.array_equal(pre, E.relu_pack(raw))


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_relu_activity_and_output_scale(L):
    for seed, out in ((1, 4), (2, 1)):
        net, obs = E.make_net(L, seed, out), E.make_obs(4096, L, seed)
        for k in range(3):
            xa, wa = E.layer_terms(net, obs, k)
            active = float(((xa @ wa.T) > 0).mean())
            assert 0.2 <= active <= 0.8, (k, active)
        y = E.forward64(net, obs)
        assert 0.2 <= y.std() <= 3.0 and np.abs(y).max() <= 16.0, (y.std(), np.abs(y).max())


def test_every_weight_and_bias_position_is_nonzero():
    for L in E.OBS_LENS:
        for out in (4, 1):
            nz = [[(w != 0, b != 0) for w, b in E.make_net(L, s, out)] for s in SEEDS]
            for k in range(4):
                assert np.logical_or.reduce([n[k][0] for n in nz]).all() and np.logical_or.reduce([n[k][1] for n in nz]).all()


def test_restatement_semantics_of_the_pack_instructions():
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0, -70000.0, np.nan, -3.0, 2.0 ** -20, np.inf, -np.inf])
    assert E.sat_pack(x).tolist() == [1.0, 1.0 + 2 * 2.0 ** -10, 65504.0, -65504.0, 0.0, -3.0, 2.0 ** -20, 65504.0, -65504.0]
    assert E.relu_pack(x).tolist() == [1.0, 1.0 + 2 * 2.0 ** -10, 65504.0, 0.0, 0.0, 0.0, 2.0 ** -20, 65504.0, 0.0]
    assert E.to_f16(np.array([1.0 + 3 * 2.0 ** -11]), "rtz").tolist() == [1.0 + 2.0 ** -10]


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_teeth(L):
    """Each of these kernel bugs changes the output of the restatement on the fixture: round-toward-zero instead of RNE, one weight moved
    to a neighbouring position (in every layer), the bias column dropped, a kernel for L - 1 on an L image."""
    for seed, out in ((1, 4), (2, 1)):
        net, obs = E.make_net(L, seed, out), E.make_obs(256, L, seed)
        want = E.forward64(net, obs)
        assert not np.array_equal(E.forward64(net, obs, rounding="rtz"), want)
        assert not np.array_equal(E.forward64(net, obs, drop_bias=True), want)
        assert not np.array_equal(E.forward64(net, obs, obs_len_shift=-1), want)
        for k in range(4):
            w, b = net[k]
            xa, wa = E.layer_terms(net, obs, k)
            # the output unit of layer k that is active most often (a dead unit hides any weight), and the neighbouring pair of its
            # weights that holds two different values whose inputs differ most often
            r = int(((xa @ wa.T) > 0).mean(axis=0).argmax()) if k < 3 else 0
            differs = (xa[:, :-2] != xa[:, 1:-1]).mean(axis=0) * (w[r, :-1] != w[r, 1:])
            c = int(differs.argmax())
            moved = [(ww.copy(), bb) for ww, bb in net]
            moved[k][0][r, c], moved[k][0][r, c + 1] = w[r, c + 1], w[r, c]
            assert not np.array_equal(E.forward64(moved, obs), want), k
