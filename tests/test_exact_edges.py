"""CPU checks of the EDGE fixtures (tests/exact_net.py: make_edge_net / make_edge_obs; tests/exact_grad.py: the edge batches) that
tests/test_gpu_operand_edges.py rests on: operands at the edges of f16 -- saturation, NaN, subnormals, rounding ties, the two zeros --
with every partial sum still exact in float32 in any order, and a restatement that tells the mis-models apart on the rows built for them."""
import numpy as np
import pytest

import exact_grad as G
import exact_net as E

LENS = E.OBS_LENS + (16,)
SHAPES = (4, 1)


@pytest.mark.parametrize("L", LENS)
def test_edge_fixture_is_exact_in_any_order_and_finite(L):
    obs, _ = E.make_edge_obs(L)
    assert obs.shape == (65, L)
    for out in SHAPES:
        net = E.make_edge_net(L, out)
        want = E.forward64(net, obs)
        assert np.isfinite(want).all()
        assert np.array_equal(want, want.astype(np.float32).astype(np.float64))
        for k, (margin, finite) in enumerate(E.exactness_margin(net, obs)):
            assert finite and margin < 1.0, (k, margin)
        for s in range(8):
            assert np.array_equal(E.forward32_in_order(net, obs, np.random.default_rng([L, s])), want), s


def _pre(net, obs, k):
    xa, wa = E.layer_terms(net, obs, k)
    return xa @ wa.T


@pytest.mark.parametrize("L", LENS)
def test_edge_values_are_where_the_fixture_says(L):
    """The edge observations, weights and hidden pre-activations the fixture promises, each hidden edge in all three hidden layers."""
    obs, rows = E.make_edge_obs(L)
    x = obs.astype(np.float64)
    assert len(rows["nan"]) == 2 and np.signbit(x[rows["nan"], 0]).tolist() == [False, True]
    assert set(obs[rows["nan"], 0].view(np.uint32).tolist()) == set(E.NAN_BITS)
    assert len(rows["subnormal_obs"]) == 7 and len(rows["inf_or_beyond"]) == 8 and len(rows["plain"]) == 36
    assert np.signbit(x[:, E.C_SUB]).sum() == 2                               # -2^-24 and -0
    for out in SHAPES:
        net = E.make_edge_net(L, out)
        for k, (w, b) in enumerate(net):
            wa = np.abs(E.weights_f16(w, b))
            raw = np.abs(np.concatenate([w, b[:, None]], axis=1).astype(np.float64))
            assert ((wa > 0) & (wa < E.F16_MIN_NORMAL)).any(), k               # subnormal weights in every layer
            assert ((raw > 0) & (raw < E.T24) & (wa != raw)).any() or k == 0 or k == 3   # ... some of them rounded on the subnormal grid
            assert (raw == E.W_BIG).any() and wa.max() == E.F16_MAX, k         # 65519.996 -> 65504
            assert ((wa != raw) & (raw > 0.1) & (raw < 4)).any(), k            # ties
            if k < 3:
                bb = np.abs(b.astype(np.float64))
                assert ((bb > 0) & (bb < E.F16_MIN_NORMAL)).any(), k           # subnormal biases
        for k in range(3):
            pre = _pre(net, obs, k)[:, :E.EDGE_P]
            h = E.to_f16(pre)
            assert ((pre > 65504) & (pre < 65520)).any() and (pre > 65520).any(), k
            assert ((pre == 0) & (np.abs(E.layer_terms(net, obs, k)[1][:E.EDGE_P, :-1]).sum(axis=1) > 0)[None, :]).any(), k
            assert ((pre > 0) & (pre <= 2.0 ** -25)).any() and ((pre < 0) & (pre > -2.0 ** -25)).any(), k
            assert (np.signbit(h) & (h == 0)).any(), k                         # f16 -0
            assert ((h > 0) & (h < E.F16_MIN_NORMAL)).any(), k                 # f16 subnormal activation


@pytest.mark.parametrize("L", LENS)
def test_edge_teeth(L):
    """Each mis-model of the restatement changes the output bits of the rows built for it -- and of no other row where that is
    decidable: flushed subnormal observations (exactly the 7 rows), NaN -> -65504 (exactly the 2 NaN rows), no saturation (exactly the
    rows with |x| >= 65520 or a hidden pre-activation beyond 65520).  Flushed subnormal weights or hidden activations and
    round-toward-zero change every row (every row carries such a weight and a rounding)."""
    obs, rows = E.make_edge_obs(L)
    for out in SHAPES:
        net = E.make_edge_net(L, out)
        want = E.forward64(net, obs)

        def changed(**kw):
            got = E.forward64(net, obs, **kw)
            return set(np.nonzero((got != want).any(axis=1) | np.isnan(got).any(axis=1))[0].tolist())

        assert changed(model="flush_obs") == set(rows["subnormal_obs"].tolist())
        assert changed(model="nan_neg") == set(rows["nan"].tolist())
        assert changed(model="no_sat") == set(rows["inf_or_beyond"].tolist()) | set(rows["hidden_beyond_65520"].tolist())
        everything = set(range(E.EDGE_ROWS))
        assert changed(model="flush_weights") == everything
        assert changed(model="flush_hidden") >= set(rows["hidden_subnormal"].tolist())
        assert changed(rounding="rtz") == everything


@pytest.mark.parametrize("L", LENS)
def test_dropping_the_low_piece_of_the_split_rows_exceeds_the_f32class_bound(L):
    """tests/test_gpu_operand_edges.py compares the f32-class forward with the float64 evaluation of the float32 parameters within
    4e-6 of the output scale.  On the rows whose low piece X1 = f16(x - X0) is an f16 subnormal, a forward that lost X1 (flushed it)
    would miss that bound more than tenfold."""
    obs = E.split_obs_rows(L)
    net = E.make_edge_net(L, f32class=True)
    ref = E.forward_plain64(net, obs)
    scale = max(1.0, float(np.abs(ref).max()))
    x = obs.astype(np.float64)
    x0 = E.sat_pack(x)
    x1 = E.sat_pack(x - x0)
    sub = (np.abs(x1) > 0) & (np.abs(x1) < E.F16_MIN_NORMAL)
    assert sub[:, E.C_SUB].sum() >= 20
    assert float(np.abs(E.forward_plain64(net, x0 + x1) - ref).max()) <= 4e-6 * scale        # the two pieces carry these rows
    err = float(np.abs(E.forward_plain64(net, x0 + np.where(sub, 0.0, x1)) - ref).max())
    assert err > 10 * 4e-6 * scale, (err, scale)


# ---- the gradient edge batches (tests/exact_grad.py: edge_nets, make_edge_batch) ------------------------------------------------------
GRAD_LENS = (13, 16, 36)
GRAD_BS = (64, 100)


@pytest.mark.parametrize("kind", tuple(G.EDGE_E))
@pytest.mark.parametrize("L", GRAD_LENS)
def test_gradient_edge_batches_are_exact_and_hold_their_edges(L, kind):
    pi, vf = G.edge_nets(L)
    for B in GRAD_BS:
        ls = G.LOG_STDS[B == 100]
        b = G.make_edge_batch(L, B, 3, pi, vf, ls, kind)
        assert G.edge_grad_exactness_margin(b, pi, vf, 0.2) < 1.0
        m_dout, m_ratio = G.loss_row_margins(b, pi, vf, 0.2)
        assert m_dout < 0.25 and m_ratio < 0.05
        want, bound = G.restate(b, pi, vf, 0.2, "f32")
        assert np.isfinite(want).all()
        q = G.loss_rows(b, pi, vf, 0.2)
        special = np.asarray(G.EDGE_E[kind][0])
        assert np.array_equal(q["err"][:len(special)], special)                 # v - ret in float64 = e: ret is exact in float32
        ret32 = b["ret"][b["idx"]][:len(special)]
        assert np.array_equal((q["v"][:len(special), 0].astype(np.float32) - ret32).astype(np.float64), special)   # ... and so is the kernel's float32 v - ret
        d4 = G.deltas(q["acts"][1], vf, q["dout"][1])[3][:len(special), 0]
        if kind == "sat":
            assert d4.tolist() == [65504.0, -65504.0, 65504.0, -65504.0] and bound[-3] > 0
        elif kind == "sub":
            assert d4.tolist() == [2.0 ** -15, -3 * 2.0 ** -22, 0.0, -0.0, 0.0, 2.0 ** -23]
        else:
            assert d4.tolist() == [1.0, 1 + 2.0 ** -9, -1 - 2.0 ** -9, 0.0]
        for net, layers in enumerate((pi, vf)):                                 # the mask edges, in two hidden layers each
            pre = []
            G.forward(layers, b["obs"][b["idx"]].astype(np.float64), pre)
            for k in (0, 1):
                p, h = pre[k][:, :G.N_PROBES], E.relu_pack(pre[k][:, :G.N_PROBES])
                assert (p >= 65504).any() and (p > 65520).any() and (h == E.F16_MAX).any()
                assert ((p > 0) & (p <= 2.0 ** -25)).any() and ((p < 0) & (p > -2.0 ** -25)).any() and (p[:, 2:] == 0).any()
                assert ((h > 0) & (h < E.F16_MIN_NORMAL)).any()


@pytest.mark.parametrize("L", GRAD_LENS)
def test_gradient_edge_teeth(L):
    """On the edge batches the restatement tells apart: -0 counted as an active unit, a saturated unit counted as inactive, flushed
    subnormal deltas (most of the "sub" kind's value-net entries), unsaturated loss deltas (the "sat" kind only), round-toward-zero."""
    pi, vf = G.edge_nets(L)
    for kind in G.EDGE_E:
        b = G.make_edge_batch(L, 100, 3, pi, vf, G.LOG_STDS[1], kind)
        want, _ = G.restate(b, pi, vf, 0.2, "bf16")
        n_pi = sum(w.size + c.size for w, c in pi)

        def changed(bug):
            with np.errstate(all="ignore"):
                got, _ = G.restate(b, pi, vf, 0.2, "bf16", bug=bug)
            return np.nonzero(~(got == want))[0]

        for bug in ("neg_zero_active", "saturated_inactive", "flush_delta", "rtz", "wrong_mask"):
            assert changed(bug).size > 0, (kind, bug)
        assert (changed("neg_zero_active") < n_pi).any()       # policy-net entries (the value head does not read the N and S chains)
        assert (changed("no_sat_delta").size > 0) == (kind == "sat")
        if kind == "sub":
            assert (changed("flush_delta") >= n_pi).sum() > 1000
