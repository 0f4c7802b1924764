"""CPU checks of the exact-arithmetic gradient fixture (tests/exact_grad.py) that the bit-exact GPU gradient tests rest on: its sums are
exact in float32 in any order, its loss rows sit far from every rounding boundary and clip edge, its restatement agrees with float64
autograd, and the restatement tells apart the kernel bugs the GPU tests are meant to catch."""
import numpy as np
import pytest
import torch

import exact_grad as G
import exact_net as E


def _case(L, B, ls=1, seed=3):
    pi, vf = G.nets(L, 1)
    return pi, vf, G.make_batch(L, B, seed, pi, vf, G.LOG_STDS[ls])


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_fixture_margins(L):
    """Every per-workgroup weight-gradient sum, every delta product and every forward product below 2^24 grid steps (float32-exact in any
    order); the float32 dout error bound far inside the f16 rounding distance; the ratio far from the clip edges; non-degenerate rows."""
    for B, ls in ((64, 0), (100, 1), (5000, 1)):
        pi, vf, b = _case(L, B, ls)
        assert G.grad_exactness_margin(b, pi, vf, 0.2) < 0.25, B
        for clip in G.CLIPS:
            m_dout, m_ratio = G.loss_row_margins(b, pi, vf, clip)
            assert m_dout < 0.25 and m_ratio < 0.05, (B, clip, m_dout, m_ratio)
        q = G.loss_rows(b, pi, vf, 0.2)
        A, fl = q["A"], q["flows"]
        for sel in (A > 0, A < 0):   # both signs of A, on both sides of the clip
            assert fl[sel].any() and (~fl[sel]).any(), B
        assert (q["gl"][~fl] == 0).all()
        dpi = G.deltas(q["acts"][0], pi, q["dout"][0])
        assert not np.array_equal(E.sat_pack(q["dout"][0]), q["dout"][0])       # dout is not exact before its f16 rounding
        assert (np.abs(dpi[3][dpi[3] != 0]) >= E.F16_MIN_NORMAL).all() and np.abs(dpi[0]).max() < 2048
        for net, layers in ((0, pi), (1, vf)):
            acts = q["acts"][net]
            for l in range(3):
                pre = acts[l] @ np.concatenate([layers[l][0], layers[l][1][:, None]], 1).astype(np.float64).T
                assert (pre == 0).any() and 0.25 < (pre > 0).mean() < 0.75, (net, l)   # exact zeros (inactive: d = 0) and dead rows


@pytest.mark.parametrize("L", (13, 36))
def test_large_minibatch_margins(L):
    """B = 16 448 (129 pairs: two passes on workgroup 0) and 65 536: 512 rows per workgroup (four passes)."""
    for B in (16448, 65536):
        pi, vf, b = _case(L, B, 1)
        assert G.grad_exactness_margin(b, pi, vf, 0.2) < 0.25
        assert max(G.loss_row_margins(b, pi, vf, 0.2)) < 0.25


def test_float32_sums_in_any_order_are_exact():
    pi, vf, b = _case(21, 5000)
    q = G.loss_rows(b, pi, vf, 0.2)
    wg, wgs = G.position_workgroup(5000)
    rng = np.random.default_rng(0)
    for net, layers in ((0, pi), (1, vf)):
        d = G.deltas(q["acts"][net], layers, q["dout"][net])
        for l in range(4):
            S64 = G.workgroup_sums(d[l], q["acts"][net][l], wg, wgs, dtype=np.float64)
            perm = rng.permutation(5000)
            S32 = G.workgroup_sums(d[l][perm], q["acts"][net][l][perm], wg[perm], wgs)
            assert np.array_equal(S32.astype(np.float64), S64), (net, l)


def test_position_to_workgroup_map():
    assert G.position_workgroup(64)[1] == 1 and G.position_workgroup(100)[1] == 1
    wg, wgs = G.position_workgroup(32768)          # 256 pairs: two passes per workgroup
    assert wgs == 128 and wg[128 * 130] == 2 and np.bincount(wg).tolist() == [256] * 128
    wg, wgs = G.position_workgroup(5000)           # 79 groups -> 40 pairs, the last one ragged
    assert wgs == 40 and wg[-1] == 39 and np.bincount(wg)[-1] == 5000 - 39 * 128


def _autograd(b, pi, vf, clip):
    """float64 autograd of the PPO loss (SB3 conventions) on the fixture's networks: flat [n] gradient and the 4 statistics."""
    idx = torch.from_numpy(b["idx"].astype(np.int64))
    x = torch.from_numpy(b["obs"]).double()[idx]
    params = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for net in (pi, vf) for w_b in net for t in w_b]
    ls = torch.tensor(b["log_std"], dtype=torch.float64, requires_grad=True)

    def run(ps, h):
        for k in range(4):
            h = h @ ps[2 * k].T + ps[2 * k + 1]
            h = torch.relu(h) if k < 3 else h
        return h

    mean, v = run(params[:8], x), run(params[8:], x)[:, 0]
    a = torch.from_numpy(b["adv"]).double()[idx]
    A = torch.from_numpy(G.normalised_advantage(b["adv"][idx])[0]).double()
    assert float((A - (a - a.mean()) / (a.std() + 1e-8)).abs().max()) < 1e-6
    act = torch.from_numpy(b["act"]).double()[idx]
    lp = (-0.5 * ((act - mean) / ls.exp()) ** 2 - ls - G.C_NORM).sum(-1)
    ratio = (lp - torch.from_numpy(b["old_logp"]).double()[idx]).exp()
    pg = -torch.min(A * ratio, A * ratio.clamp(1 - clip, 1 + clip)).mean()
    vl = ((v - torch.from_numpy(b["ret"]).double()[idx]) ** 2).mean()
    loss = pg + G.VF_COEF * vl - G.ENT_COEF * ls.sum()
    loss.backward()
    return torch.cat([p.grad.reshape(-1) for p in params] + [ls.grad]).numpy()


@pytest.mark.parametrize("L,B,clip", [(13, 64, 0.2), (24, 100, 50.0), (36, 5000, 0.2), (29, 4096, 50.0)])
def test_restatement_matches_float64_autograd(L, B, clip):
    """The restatement before its partial rounding (per-workgroup sums / B) equals float64 autograd up to the f16 rounding of the
    output deltas (~1e-6: autograd sees the unrounded dout); the f32 and bf16 vectors within their partial rounding; log_std within bound."""
    pi, vf, b = _case(L, B)
    ref = _autograd(b, pi, vf, clip)
    out, q, sums = G.restate(b, pi, vf, clip, partial=("bf16", "f32"), return_sums=True)
    flat = np.concatenate([np.concatenate([s[:layers[l][0].shape[0], :-1].reshape(-1), s[:layers[l][0].shape[0], -1]])
                           for k, layers in enumerate((pi, vf)) for l, s in enumerate(sums[4 * k:4 * k + 4])])
    n = flat.size
    scale = np.abs(ref[:n]).max()
    assert np.abs(flat - ref[:n]).max() <= 1e-5 * scale
    for fmt, tol in (("f32", 1e-5), ("bf16", 2.0 ** -7)):
        want, bound = out[fmt]
        assert np.abs(want[:n] - ref[:n]).max() <= tol * scale, fmt
        assert (np.abs(want[n:n + 4] - ref[n:]) <= bound[n:n + 4] + 2e-6 * np.abs(ref[n:])).all()   # + autograd's unrounded dout
    assert np.array_equal(out["f32"][0][n:], out["bf16"][0][n:])


def _moved(want, bound, other):
    exact = bound == 0
    return bool((want[exact] != other[exact]).any() or (np.abs(want - other)[~exact] > bound[~exact]).any())


@pytest.mark.parametrize("L", (13, 24, 36))
@pytest.mark.parametrize("bug", G.BUGS)
def test_teeth(L, bug):
    """Each modelled kernel bug moves at least one element of the restated vector beyond the comparison's tolerance (exact entries: any
    change; bounded entries: beyond the bound) at B = 100 (one workgroup, a ragged tail of 28 positions) and B = 5000 (40 workgroups).
    A biased variance scales A by ~1 + 1/(2B): at B = 5000 that is below half an f16 ulp of the output deltas (2^-12) and inside the
    log-std bound, so it is shown at B = 100 only (the GPU tests cover both sizes)."""
    for B in ((100,) if bug == "biased_var" else (100, 5000)):
        pi, vf, b = _case(L, B)
        for fmt in ("bf16", "f32"):
            if bug == "bf16_trunc" and fmt == "f32":
                continue
            want, bound = G.restate(b, pi, vf, 0.2, partial=fmt)
            other, _ = G.restate(b, pi, vf, 0.2, partial=fmt, bug=bug)
            assert _moved(want, bound, other), (bug, B, fmt)


def test_f32class_restatement():
    """The f32-class restatement: value-net entries exact (bound 0) and equal to float64 autograd up to float32 rounding; the policy
    entries' per-element bound (gamma_kps sum |terms|: at most ~1e-3 of the largest entry where a slice's terms cancel) stays below the
    old aggregate tolerance of 5e-3 of a tensor norm."""
    for L, B in ((17, 2), (17, 3), (25, 5000)):
        pi, vf, b = _case(L, B)
        want, bound = G.restate_f32class(b, pi, vf, 0.2)
        ref = _autograd(b, pi, vf, 0.2)
        n = ref.size - 4
        npi = sum(w.size + bb.size for w, bb in pi)
        assert (bound[npi:n] == 0).all()
        assert np.abs(want[:n] - ref[:n]).max() <= 1e-5 * np.abs(ref[:n]).max()
        assert bound[:npi].max() <= 2e-3 * np.abs(ref[:npi]).max()
